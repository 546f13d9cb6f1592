"""Validation panels: ``starcop/plot.py`` (``plot_batch``, ``mask_to_rgb``, ``COLORS_DIFFERENCES``, the ``PLOTTING_FUNCTIONS``
registry) with the image panels of a figure drawn on the GPU.

The reference hands every tensor of ``batch_with_preds`` to matplotlib on the host, one ``imshow`` per panel and one ``savefig``
per tile.  Here ``render_batch`` leaves the tensors where they are: ``sc_panel_minmax`` finds the range of the panels the reference
draws without limits, ``sc_render_panels`` colours and enlarges every panel of the figure in one launch and writes PNG scanlines,
and only that 8-bit canvas crosses to the host (``Panels.image`` / ``Panels.save``).  The canvas holds image panels only: no text,
legends or colour bars; the panel names and ranges travel in ``Panels`` and in the PNG's tEXt chunk.  The per-pixel arithmetic is
written out in DESIGN.md ("Validation panels") and include/starcop_hip.h.

``select_panels`` is the tensor-selection logic of ``plot_batch`` (plot.py:201-245) as host code over tensor metadata;
``plot_batch`` itself keeps the reference's signature and needs matplotlib only for the figure it returns.
"""
import json
import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, stream

_HERE = os.path.dirname(os.path.abspath(__file__))

COLORS_DIFFERENCES = np.array([[0, 0, 0],         # correct no-plume
                               [255, 0, 0],       # plume missed (red)
                               [220, 220, 0],     # plume overpredicted (yellow)
                               [0, 200, 0]        # correct plume (green)
                               ]) / 255

INTERPRETATION_DIFFERENCES = ["correct no-plume", "false plume", "false no-plume", "correct plume"]


def viridis8() -> np.ndarray:
    """(256, 3) uint8: matplotlib's ``(viridis.colors * 255).astype(uint8)`` (data/viridis8.txt, the table the kernel is built with)"""
    return np.loadtxt(os.path.join(_HERE, "data", "viridis8.txt"), dtype=np.uint8).reshape(256, 3)


def _band(products, vmin=None, vmax=None, tensor="input_norm"):
    d = {"tensor": tensor, "kind": "band", "vmin": vmin, "vmax": vmax}
    if products is not None:
        d = {"input_products": list(products), **d}
    return d


def _rgb(products):
    return {"input_products": list(products), "tensor": "input_norm", "kind": "rgb", "vmin": None, "vmax": None}


# plot.py:98-188 as data.  kind "band" with vmin = vmax = None is what the reference shows with a colour bar and no limits: the
# range is the data's own (autoscale).  The reference's quirks stay: pred_binary shows "prediction", s2_b2..s2_b4 name TOA_S2B_B1.
PLOTTING_FUNCTIONS: Dict[str, Dict[str, Any]] = {
    "rgb_aviris": _rgb(["TOA_AVIRIS_460nm", "TOA_AVIRIS_550nm", "TOA_AVIRIS_640nm"]),
    "rgb_s2a": _rgb(["TOA_S2A_B4", "TOA_S2A_B3", "TOA_S2A_B2"]),
    "swirnirred_s2a": _rgb(["TOA_S2A_B11", "TOA_S2A_B8", "TOA_S2A_B4"]),
    "aviris_ratios_first": _band(["ratio_aviris_2350_2310_out"]),
    "aviris_ratios_second": _band(["ratio_aviris_2350_2360_out"]),
    "aviris_ratios_third": _band(["ratio_aviris_2360_2310_out"]),
    "wv3_ratios_varon_b7b5": _band(["ratio_wv3_B7_B5_varon21_sum_c_out"]),
    "wv3_ratios_varon_b8b5": _band(["ratio_wv3_B8_B5_varon21_sum_c_out"]),
    "wv3_ratios_varon_b7b6": _band(["ratio_wv3_B7_B6_varon21_sum_c_out"]),
    "wv3_ratios_sanchez_b7b7mlr": _band(["ratio_wv3_B7_B7MLR_SanchezGarcia22_sum_c_out"]),
    "wv3_ratios_sanchez_b8b8mlr": _band(["ratio_wv3_B8_B8MLR_SanchezGarcia22_sum_c_out"]),
    "wv3_ratios_sanchez_b7b7mlr_v2": _band(["ratio_wv3_B7_B7MLR_SanchezGarcia22_simplediv"]),
    "wv3_ratios_sanchez_b8b8mlr_v2": _band(["ratio_wv3_B8_B8MLR_SanchezGarcia22_simplediv"]),
    "wv3_lrn_bands2band8only_60ep_512_l1": _band(["ratio_lrn_bands2band8only_60ep_512_l1"]),
    "wv3_mixSanchez_b7b7mlr_fromS2_9b": _band(["ratio_wv3_B7_B7MLR_fromS2_9bands_sum_c_out"]),
    "wv3_mixSanchez_b7b7mlr_fromS2_5b": _band(["ratio_wv3_B7_B7MLR_fromS2_5bands_sum_c_out"]),
    "wv3_mixSanchez_b8b8mlr_fromS2_9b": _band(["ratio_wv3_B8_B8MLR_fromS2_9bands_sum_c_out"]),
    "wv3_mixSanchez_b8b8mlr_fromS2_5b": _band(["ratio_wv3_B8_B8MLR_fromS2_5bands_sum_c_out"]),
    "s2_b1": _band(["TOA_S2B_B1"]),
    "s2_b2": _band(["TOA_S2B_B1"]),
    "s2_b3": _band(["TOA_S2B_B1"]),
    "s2_b4": _band(["TOA_S2B_B1"]),
    "wv3_b1": _band(["TOA_WV3_SWIR1"]),
    "wv3_b2": _band(["TOA_WV3_SWIR2"]),
    "wv3_b3": _band(["TOA_WV3_SWIR3"]),
    "wv3_b4": _band(["TOA_WV3_SWIR4"]),
    "wv3_b5": _band(["TOA_WV3_SWIR5"]),
    "wv3_b6": _band(["TOA_WV3_SWIR6"]),
    "wv3_b7": _band(["TOA_WV3_SWIR7"]),
    "wv3_b8": _band(["TOA_WV3_SWIR8"]),
    "mag1c": _band(["mag1c"], 0, 2),
    "label": _band(None, 0, 1, tensor="output_norm"),
    "pred": _band(None, 0, 1, tensor="prediction"),
    "pred_binary": _band(None, 0, 1, tensor="prediction"),
    "weight_loss": _band(None, 0, 1, tensor="weight_loss"),
    "differences": {"tensor": "differences", "kind": "categorical", "vmin": None, "vmax": None},
}


def mask_to_rgb(mask, values, colors_cmap: np.ndarray) -> np.ndarray:
    """(H, W, 3) or (H, W, 4) uint8: every pixel of the 2D ``mask`` equal to ``values[i]`` gets ``round(colors_cmap[i] * 255)``
    (colours are floats in [0, 1]; later entries win, no match is 0), plot.py:13-38.  A device tensor is coloured by the
    categorical path of ``sc_render_panels`` (at most 8 values); numpy input needs no GPU."""
    colors_cmap = np.asarray(colors_cmap)
    assert len(values) == len(colors_cmap), f"Values and colors should have same length {len(values)} {len(colors_cmap)}"
    assert len(mask.shape) == 2, f"Expected only 2D array found {mask.shape}"
    colores = np.array(np.round(colors_cmap * 255), dtype=np.uint8)
    if torch.is_tensor(mask) and mask.is_cuda:
        if len(values) > _lib.PANEL_MAX_CAT:
            raise ValueError(f"mask_to_rgb: {len(values)} values, the categorical kernel takes {_lib.PANEL_MAX_CAT}")
        plane = _as_planes(mask, 1, squeeze=False)
        groups = [colores[:, :3]] + ([np.repeat(colores[:, 3:4], 3, axis=1)] if colores.shape[1] == 4 else [])
        specs = [PanelSpec(f"mask{k}", "categorical", plane, categories=[(float(v), tuple(int(x) for x in c)) for v, c in zip(values, g)])
                 for k, g in enumerate(groups)]
        img = _render([specs], panel_px=1, gap=0).image
        H, W = mask.shape
        if len(groups) == 1:
            return img.copy()
        return np.concatenate([img[:, :W], img[:, W:, :1]], axis=2)
    if hasattr(mask, "cpu"):
        mask = mask.cpu()
    mask = np.asanyarray(mask)
    mask_return = np.zeros((colors_cmap.shape[1],) + mask.shape[:2], dtype=np.uint8)
    for i, c in enumerate(colores):
        for _j in range(len(c)):
            mask_return[_j][mask == values[i]] = c[_j]
    return np.transpose(mask_return, (1, 2, 0))


@dataclass
class PanelSpec:
    """one column of a figure: what ``select_panels`` picked for a product (``tensor`` keeps the batch dimension)"""
    name: str
    kind: str                                   # "band" | "rgb" | "categorical"
    tensor: Any
    key: Optional[str] = None                   # the batch key the tensor came from
    channels: Optional[Tuple[int, ...]] = None  # channels picked from it (None: all of it)
    vmin: Optional[float] = None
    vmax: Optional[float] = None
    autoscale: bool = False
    div: float = 1.0
    categories: Optional[List[Tuple[float, Tuple[int, int, int]]]] = None


_DIFF_CATEGORIES = [(float(v), tuple(int(x) for x in np.round(c * 255))) for v, c in enumerate(COLORS_DIFFERENCES)]


def select_panels(batch_with_preds: Dict[str, Any], input_products: Sequence[str], products_plot: Sequence[str]) -> List[PanelSpec]:
    """The tensor each product of ``products_plot`` shows (plot.py:201-245): a registered product comes from its own batch key,
    from the keys of its ``input_products``, or from the channels of its registered tensor; an unregistered one from its batch
    key or from its channel of ``input_norm``.  ``mag1c`` taken from its own key is divided by 1750 (here: by the kernel)."""
    input_products = list(input_products)
    out = []
    for p in products_plot:
        key, channels, div = None, None, 1.0
        if p not in PLOTTING_FUNCTIONS:
            if p not in batch_with_preds:
                assert p in input_products, f"{p} not registered in {PLOTTING_FUNCTIONS.keys()} and not in {input_products}"
                key, channels = "input_norm", (input_products.index(p),)
                tensor = batch_with_preds[key][:, channels[0]]
            else:
                key, tensor = p, batch_with_preds[p]
            entry = {"kind": "band", "vmin": None, "vmax": None}
        else:
            entry = PLOTTING_FUNCTIONS[p]
            if p not in batch_with_preds:
                ips = entry.get("input_products", [])       # note, we may not have "input_products" at all!
                if len(ips) > 0 and all(ip in batch_with_preds for ip in ips):
                    if len(ips) > 1:
                        # the reference concatenates along dim 0, which its own show_3_bands then rejects for any batch; the
                        # products are (B, 1, H, W) or (B, H, W) planes, stacked here as the channels they are
                        parts = [batch_with_preds[ip] for ip in ips]
                        tensor = torch.cat(parts, dim=1) if parts[0].dim() == 4 else torch.stack(parts, dim=1)
                        key = tuple(ips)
                    else:
                        key, tensor = ips[0], batch_with_preds[ips[0]]
                        if p == "mag1c":
                            div = 1750.0
                else:
                    key = entry["tensor"]
                    assert key in batch_with_preds, f"Batch does not have keys: {p} {key}. Keys in batch: {batch_with_preds.keys()}"
                    tensor = batch_with_preds[key]
                    if key.startswith("input"):
                        idx_show = [idx for idx, ip in enumerate(input_products) if ip in entry["input_products"]]
                        assert len(entry["input_products"]) == len(idx_show), "Unexpected number of products"
                        channels = tuple(idx_show)
                        c0, nc = channels[0], len(channels)
                        consecutive = channels == tuple(range(c0, c0 + nc))          # then a view, else a gather
                        tensor = tensor[:, c0:c0 + nc] if consecutive else tensor[:, channels, ...]
            else:
                key, tensor = p, batch_with_preds[p]
                if p == "mag1c":
                    div = 1750.0
        band_free = entry["kind"] == "band" and entry["vmin"] is None
        out.append(PanelSpec(p, entry["kind"], tensor, key, channels, entry["vmin"], entry["vmax"], band_free, div,
                             _DIFF_CATEGORIES if entry["kind"] == "categorical" else None))
    return out


_DTYPES = {torch.float32: _lib.PANEL_F32, torch.int64: _lib.PANEL_I64, torch.uint8: _lib.PANEL_U8}
_KINDS = {"band": _lib.PANEL_BAND, "rgb": _lib.PANEL_RGB, "categorical": _lib.PANEL_CATEGORICAL}


def _as_planes(item: torch.Tensor, n: int, squeeze: bool = True) -> List[torch.Tensor]:
    """``n`` 2D planes of a kernel dtype with unit column stride out of one batch item (views where the tensor allows it)"""
    if squeeze:
        item = item.squeeze()
    if n == 3:
        assert item.dim() == 3 and item.shape[0] == 3, f"Expected (C, H, W) tensor found {item.shape}"
        planes = [item[c] for c in range(3)]
    else:
        assert item.dim() == 2, f"Expected (H, W) tensor found {item.shape}"
        planes = [item]
    out = []
    for pl in planes:
        if pl.dtype not in _DTYPES:
            pl = pl.to(torch.uint8) if pl.dtype == torch.bool else (pl.float() if pl.is_floating_point() else pl.long())
        if pl.stride(1) != 1 or pl.stride(0) < pl.shape[1]:
            pl = pl.contiguous()
        out.append(pl)
    return out


class Panels:
    """A rendered figure.  ``canvas``: the PNG scanlines on the device (``height`` rows of ``1 + 3 * width`` uint8); ``names``:
    the panel names of a row; ``rects[b][p]``: ``(y, x, h, w)`` of panel ``p`` of batch item ``b`` on the canvas."""

    def __init__(self, canvas, height, width, names, rects, minmax, kinds):
        self.canvas, self.height, self.width, self.names, self.rects = canvas, height, width, list(names), rects
        self._minmax, self._kinds, self._host, self._ranges = minmax, kinds, None, None

    @property
    def scanlines(self) -> np.ndarray:
        """the canvas on the host, (height, 1 + 3 * width) uint8: the one read-back"""
        if self._host is None:
            self._host = self.canvas.cpu().numpy().reshape(self.height, 1 + 3 * self.width)
        return self._host

    @property
    def image(self) -> np.ndarray:
        """(height, width, 3) uint8 view of the host canvas"""
        return self.scanlines[:, 1:].reshape(self.height, self.width, 3)

    @property
    def ranges(self) -> List[Optional[Tuple[float, float]]]:
        """(vmin, vmax) each panel was drawn with, row by row; None for panels that have no range (rgb, categorical)"""
        if self._ranges is None:
            mm = self._minmax.cpu().numpy()
            self._ranges = [(float(mm[i, 0]), float(mm[i, 1])) if k == "band" else None for i, k in enumerate(self._kinds)]
        return self._ranges

    def panel(self, b: int, p: int) -> np.ndarray:
        y, x, h, w = self.rects[b][p]
        return self.image[y:y + h, x:x + w]

    def save(self, path):
        from .io_formats import write_png
        text = json.dumps({"names": self.names, "rows": len(self.rects), "ranges": self.ranges, "rects": self.rects})
        write_png(path, self.scanlines, self.width, self.height, text=text)


def _layout(rows: List[List[PanelSpec]], panel_px: int, gap: int):
    """(table, rects, Hc, Wc) of a figure; rows[b][p]: specs whose ``tensor`` is the list of planes of one batch item.  Every
    panel is enlarged by ``max(1, panel_px // max(H, W))``; a column is as wide as its widest panel, a row as high as its highest."""
    n = sum(len(r) for r in rows)
    table = (_lib.sc_panel * n)()
    sizes = []
    for r in rows:
        for s in r:
            H, W = s.tensor[0].shape
            scale = max(1, int(panel_px) // max(H, W))
            sizes.append((H * scale, W * scale, scale))
    ncols = len(rows[0])
    assert all(len(r) == ncols for r in rows)
    colw = [max(sizes[b * ncols + p][1] for b in range(len(rows))) for p in range(ncols)]
    i, y, rects = 0, 0, []
    for r in rows:
        x, rowh, rr = 0, 0, []
        for p, s in enumerate(r):
            h, w, scale = sizes[i]
            t, planes = table[i], s.tensor
            for c, pl in enumerate(planes):
                t.src[c] = pl.data_ptr()
            t.row_stride, t.dtype, t.kind = planes[0].stride(0), _DTYPES[planes[0].dtype], _KINDS[s.kind]
            t.H, t.W, t.scale, t.dst_y, t.dst_x = planes[0].shape[0], planes[0].shape[1], scale, y, x
            t.autoscale, t.div = int(s.autoscale), float(s.div)
            t.vmin, t.vmax = (0.0, 1.0) if s.vmin is None else (float(s.vmin), float(s.vmax))
            cats = s.categories or []
            t.n_cat = len(cats)
            for k, (v, rgb) in enumerate(cats[:_lib.PANEL_MAX_CAT]):
                t.cat_value[k] = v
                for j in range(3):
                    t.cat_rgb[k][j] = rgb[j]
            rr.append((y, x, h, w))
            x += colw[p] + gap
            rowh = max(rowh, h)
            i += 1
        rects.append(rr)
        y += rowh + gap
    return table, rects, y - gap, sum(colw) + gap * (ncols - 1)


def _check_planes(rows: List[List[PanelSpec]]) -> torch.device:
    """The one device every plane of the figure lives on.  The kernels dereference the planes' addresses, and the C side cannot
    tell a host pointer or another GPU's from a good one, so a plane anywhere else is an error here, before any address is taken."""
    dev = None
    for b, r in enumerate(rows):
        for s in r:
            for pl in s.tensor:
                if not getattr(pl, "is_cuda", False):
                    where = getattr(pl, "device", type(pl).__name__)
                    raise _lib.StarcopHipError(f"panel {s.name!r} of batch item {b} is on {where}: the panels are drawn from device "
                                               "tensors only (move the batch with validation.to_device first)")
                dev = pl.device if dev is None else dev
                if pl.device != dev:
                    raise _lib.StarcopHipError(f"panel {s.name!r} of batch item {b} is on {pl.device}, the figure's first panel on {dev}")
    return dev


def _render(rows: List[List[PanelSpec]], panel_px: int, gap: int) -> Panels:
    dev = _check_planes(rows)
    with torch.cuda.device(dev):                # the launches, their stream and the allocations belong to the planes' device
        _lib.require_device(rows[0][0].tensor[0])
        lib = _lib.load()
        table, rects, Hc, Wc = _layout(rows, panel_px, gap)
        n = len(table)
        table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        minmax = torch.empty((n, 2), dtype=torch.float32, device=dev)
        canvas = torch.empty(Hc * (1 + 3 * Wc), dtype=torch.uint8, device=dev)
        check(lib.sc_panel_minmax(table_dev.data_ptr(), table, n, minmax.data_ptr(), stream()))
        check(lib.sc_render_panels(table_dev.data_ptr(), table, n, minmax.data_ptr(), canvas.data_ptr(), Hc, Wc, stream()))
    return Panels(canvas, Hc, Wc, [s.name for s in rows[0]], rects, minmax, [s.kind for r in rows for s in r])


def _item_rows(specs: List[PanelSpec], batch_size: int) -> List[List[PanelSpec]]:
    """the specs of ``select_panels`` per batch item, their tensors cut into the planes the kernel reads"""
    rows = []
    for b in range(batch_size):
        row = []
        for s in specs:
            item = s.tensor[b]
            if not torch.is_tensor(item):
                raise _lib.StarcopHipError(f"panel {s.name!r} is a {type(s.tensor).__name__}, not a tensor: the panels are drawn from "
                                           "device tensors only")
            planes = _as_planes(item, 3 if s.kind == "rgb" else 1)
            row.append(PanelSpec(s.name, s.kind, planes, s.key, s.channels, s.vmin, s.vmax, s.autoscale, s.div, s.categories))
        rows.append(row)
    return rows


@torch.no_grad()
def render_batch(batch_with_preds: Dict[str, Any], input_products: Sequence[str], products_plot: Sequence[str],
                 panel_px: int = 512, gap: int = 4) -> Panels:
    """The figure of ``plot_batch`` as image panels: row ``b`` is batch item ``b``, column ``p`` is ``products_plot[p]``, each
    panel enlarged by ``max(1, panel_px // max(H, W))``, ``gap`` white pixels apart.  Two launches, no host synchronisation."""
    specs = select_panels(batch_with_preds, input_products, products_plot)
    assert len(specs) > 0, "render_batch: products_plot is empty"
    rows = _item_rows(specs, len(batch_with_preds["input"]))
    return _render(rows, panel_px, gap)


@torch.no_grad()
def plot_batch(batch_with_preds: Dict[str, Any], input_products: List[str], products_plot: List[str],
               figsize_ax: Tuple[int, int] = (2, 2), add_id_to_title: bool = False):
    """``(fig, ax)`` of the reference (plot.py:190-255): one ``ax.imshow`` per GPU-rendered panel with the reference's titles.
    matplotlib is needed for the figure only and imported here; without it this raises ImportError (use ``render_batch``)."""
    import matplotlib.pyplot as plt
    panels = render_batch(batch_with_preds, input_products, products_plot)
    batch_size = len(panels.rects)
    fig, ax = plt.subplots(batch_size, len(products_plot), figsize=(figsize_ax[0] * len(products_plot), figsize_ax[1] * batch_size),
                           tight_layout=True, squeeze=False)
    for idx_product_plot, p in enumerate(products_plot):
        for idx_batch in range(batch_size):
            ax[idx_batch, idx_product_plot].imshow(panels.panel(idx_batch, idx_product_plot), interpolation="nearest")
            if add_id_to_title:
                ax[idx_batch, idx_product_plot].set_title(f"{p} {batch_with_preds['id'][idx_batch]}")
            elif idx_batch == 0:
                ax[idx_batch, idx_product_plot].set_title(p)
    return fig, ax
