"""The feature transform on the device against the brute-force oracle of nearest_util.py: sc_edt_nearest through both row passes
(index, squared distance, gathered planes), expand_labels, fill_nearest, background_rings, the ring columns of plume_table and
the plume_background= argument of products.annotate and pipeline.aviris_scene_predict.  Every comparison is exact except the
float64 ring means, whose tolerance is that of plumes_util.py.  skimage is not installed here: expand_labels is compared with
its restatement (nearest_util.expand_labels_ref)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import morphology_util as U
import nearest_util as NU
import plumes_util as PU

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = dict(U.case_table() + NU.tie_cases())
NAMES = list(CASES)
CAPS = (1, 5, 64)
BERN = [n for n in NAMES if n.startswith("bern") and CASES[n].size <= U.BRUTE_MAX_PIXELS and CASES[n].any()]


@functools.lru_cache(maxsize=None)
def oracle(name, to):
    """(index, d2) of a case, computed once and never modified"""
    m = CASES[name]
    index, d2 = NU.nearest_brute(m != 0 if to == "set" else m == 0)
    index.setflags(write=False)
    d2.setflags(write=False)
    return index, d2


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                       # a copy: the cached cases are read-only


def host(t):
    return t.cpu().numpy()


def equal(got, want):
    """a device int32 result == an int64 oracle"""
    got = host(got)
    return got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got.astype(np.int64), want)


@pytest.mark.parametrize("to", ("set", "unset"))
@pytest.mark.parametrize("name", NAMES)
def test_nearest_index(hip, name, to):
    """unbounded (envelope); caps 1, 5 and 64 through both row passes, equal to each other and to the oracle; cap 0; the squared
    distance bit-equal to distance_transform's"""
    from starcop_amd import morphology as mo
    m = dev(CASES[name])
    index, d2 = oracle(name, to)
    gi, gd = mo.nearest_index(m, to=to, return_distance=True)
    assert gi.is_cuda and gd.is_cuda
    assert equal(gi, index), f"{int((host(gi) != index).sum())} indices differ"
    assert equal(gd, d2)
    assert torch.equal(gd, mo.distance_transform(m, to=to, squared=True))
    assert torch.equal(mo.nearest_index(m, to=to), gi)                          # the index alone
    for r in CAPS:
        wi, wd = NU.capped(index, d2, r * r)
        res = {v: mo.nearest_index(m, to=to, max_distance=r, return_distance=True, variant=v) for v in ("window", "envelope")}
        for v, (ci, cd) in res.items():
            assert equal(ci, wi), (r, v, int((host(ci) != wi).sum()))
            assert equal(cd, wd), (r, v)
        assert torch.equal(res["window"][0], res["envelope"][0]) and torch.equal(res["window"][1], res["envelope"][1])
        assert torch.equal(res["window"][1], mo.distance_transform(m, to=to, max_distance=r, squared=True))
        ri, rd = mo.nearest_index(m, to=to, max_distance=r, return_distance=True)   # the rule's own choice
        assert torch.equal(ri, res["window"][0]) and torch.equal(rd, res["window"][1])
    # a cap whose floor(sqrt) is the window's but which is no square: 5.5 -> 30, R = 5
    wi, wd = NU.capped(index, d2, 30)
    for v in ("window", "envelope"):
        ci, cd = mo.nearest_index(m, to=to, max_distance=5.5, return_distance=True, variant=v)
        assert equal(ci, wi) and equal(cd, wd), v
    zi, zd = mo.nearest_index(m, to=to, max_distance=0, return_distance=True)
    wi, wd = NU.capped(index, d2, 0)
    assert equal(zi, wi) and equal(zd, wd)
    assert torch.equal(zd, mo.distance_transform(m, to=to, max_distance=0, squared=True))


def test_four_symmetric_targets(hip):
    from starcop_amd import morphology as mo
    m, index, d2 = NU.four_symmetric()
    for kw in ({}, {"max_distance": 2, "variant": "window"}, {"max_distance": 2, "variant": "envelope"}):
        gi, gd = mo.nearest_index(m, return_distance=True, **kw)
        assert isinstance(gi, np.ndarray) and gi.dtype == np.int32 and np.array_equal(gi, index) and np.array_equal(gd, d2), kw


def test_batches_and_input_forms(hip):
    from starcop_amd import morphology as mo
    rng = np.random.default_rng(17)
    batch = (rng.random((3, 70, 131)) < np.array([0.01, 0.3, 0.0])[:, None, None]).astype(np.uint8)
    batch[2] = 0                                                       # an image without a target inside a batch
    for kw in ({}, {"max_distance": 7}, {"max_distance": 7, "variant": "envelope"}, {"to": "unset"}):
        gi, gd = mo.nearest_index(dev(batch), return_distance=True, **kw)
        for n in range(3):
            oi, od = mo.nearest_index(dev(batch[n]), return_distance=True, **kw)
            assert torch.equal(gi[n], oi) and torch.equal(gd[n], od), (kw, n)
        ai, ad = mo.nearest_index(dev(batch), return_distance=True, **kw)    # two calls, identical bytes
        assert torch.equal(ai, gi) and torch.equal(ad, gd)
        ni, nd = mo.nearest_index(batch, return_distance=True, **kw)         # numpy in, numpy out
        assert isinstance(ni, np.ndarray) and ni.dtype == np.int32 and np.array_equal(ni, host(gi)) and np.array_equal(nd, host(gd))
    assert (host(mo.nearest_index(dev(batch)))[2] == -1).all()
    want = NU.nearest_brute(batch[0] != 0)
    assert equal(mo.nearest_index(dev(batch[0])), want[0])
    # read in place: a [:, ::2] view and one band of an (H, W, 4) image; bool as it is
    wide = dev(rng.random((40, 140)) < 0.05).to(torch.uint8)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    assert torch.equal(mo.nearest_index(view), mo.nearest_index(view.contiguous()))
    assert torch.equal(mo.nearest_index(view, max_distance=4), mo.nearest_index(view.contiguous(), max_distance=4))
    rgba = dev((rng.random((40, 70, 4)) < 0.05).astype(np.uint8))
    assert torch.equal(mo.nearest_index(rgba[:, :, 2], to="unset"), mo.nearest_index(rgba[:, :, 2].contiguous(), to="unset"))
    assert torch.equal(mo.nearest_index(view != 0), mo.nearest_index(view.contiguous()))
    assert torch.equal(mo.nearest_index(view.float() * 2.5), mo.nearest_index(view.contiguous()))


@functools.lru_cache(maxsize=None)
def label_image(name):
    """random labels 1..7 on the set pixels of a Bernoulli case"""
    m = CASES[name]
    lab = np.where(m != 0, np.random.default_rng(len(name) + int(m.sum())).integers(1, 8, size=m.shape), 0).astype(np.int32)
    lab.setflags(write=False)
    return lab


@pytest.mark.parametrize("name", BERN)
def test_expand_labels(hip, name):
    from starcop_amd import morphology as mo
    lab = label_image(name)
    for distance in (0, 1, 2.5, 40):
        got = mo.expand_labels(dev(lab), distance)
        assert got.dtype == torch.int32 and np.array_equal(host(got), NU.expand_labels_ref(lab, distance)), distance
    got = mo.expand_labels(lab.astype(np.int64), 2.5)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, NU.expand_labels_ref(lab, 2.5))
    H, W = lab.shape
    assert (host(mo.expand_labels(dev(lab), math.hypot(H, W) + 1)) != 0).all()


def test_expand_labels_of_components(hip):
    """a connected_components label image, in a batch with an image without a label"""
    from starcop_amd import morphology as mo
    from starcop_amd.mask_creation import connected_components
    m = np.stack([plume_mask(), np.zeros((96, 160), dtype=np.uint8)])
    labels, _ = connected_components(dev(m))
    lab = host(labels)
    for distance in (0, 1, 2.5, 40):
        got = host(mo.expand_labels(labels, distance))
        assert np.array_equal(got[0], NU.expand_labels_ref(lab[0], distance)) and not got[1].any(), distance
    big = host(mo.expand_labels(labels, 200))
    assert (big[0] != 0).all() and not big[1].any()
    same = mo.expand_labels(labels, 0)
    assert torch.equal(same, labels) and same.data_ptr() != labels.data_ptr()


def _value_planes(shape, n, seed):
    """float32 planes with NaN, -0.0, inf and a NaN with a payload scattered over them"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        p = rng.standard_normal(shape).astype(np.float32)
        flat = p.reshape(-1)
        at = rng.choice(flat.size, size=min(flat.size, 40), replace=False)
        special = np.array([np.nan, -0.0, np.inf, 0.0], dtype=np.float32).view(np.uint32).tolist() + [0x7FC01234 + k, 0xFFC00001]
        flat.view(np.uint32)[at] = np.array([special[i % len(special)] for i in range(at.size)], dtype=np.uint32)
        out.append(p)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", ["bern0.05_37x53", "bern0.5_64x130", "bern0.002_9x257", "checker_37x53", "full_37x53", "empty_37x53"])
def test_fill_nearest(hip, name):
    """``invalid`` is the case's mask: the targets are its unset pixels; compared as bits"""
    from starcop_amd import morphology as mo
    inv = CASES[name]
    data = _value_planes(inv.shape, 1, 5)[0]
    got = mo.fill_nearest(dev(data), dev(inv))
    assert got.dtype == torch.float32 and np.array_equal(bits(host(got)), bits(NU.fill_nearest_ref(data, inv)))
    assert np.array_equal(bits(host(got))[inv == 0], bits(data)[inv == 0])            # valid pixels keep their bits
    if name.startswith("full"):                                                      # all invalid: returned unchanged
        assert np.array_equal(bits(host(got)), bits(data))
    for cap in (0, 1, 3.5):
        got = mo.fill_nearest(dev(data), dev(inv), max_distance=cap)
        want = NU.fill_nearest_ref(data, inv, max_distance=cap)
        assert np.array_equal(bits(host(got)), bits(want)), cap
        far = (inv != 0) & (NU.nearest_brute(inv == 0)[1] > int(cap * cap))
        assert np.array_equal(bits(host(got))[far], bits(data)[far])                  # far pixels unchanged
    got = mo.fill_nearest(data, inv)
    assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(NU.fill_nearest_ref(data, inv)))


def test_fill_nearest_planes_and_batches(hip):
    from starcop_amd import morphology as mo
    rng = np.random.default_rng(23)
    inv = (rng.random((2, 50, 77)) < 0.6).astype(np.uint8)
    inv[1] = 1                                                                       # an image with no valid pixel
    planes = _value_planes(inv.shape, 8, 9)
    many = mo.fill_nearest([dev(p) for p in planes], dev(inv))
    assert isinstance(many, list) and len(many) == 8
    for p, g in zip(planes, many):
        assert torch.equal(mo.fill_nearest(dev(p), dev(inv)).view(torch.int32), g.view(torch.int32))
        assert np.array_equal(bits(host(g))[0], bits(NU.fill_nearest_ref(p[0], inv[0])))
        assert np.array_equal(bits(host(g))[1], bits(p[1]))
    again = mo.fill_nearest([dev(p) for p in planes], dev(inv))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again, many))
    with pytest.raises(ValueError):
        mo.fill_nearest([dev(p) for p in planes] + [dev(planes[0])], dev(inv))
    # a channel of an (N, C, H, W) tensor is gathered in place; a bool mask view is read through its strides
    stack = dev(np.stack(planes[:3], 1))
    got = mo.fill_nearest(stack[:, 1], dev(inv) != 0)
    assert torch.equal(got.view(torch.int32), many[1].view(torch.int32))


# ------------------------------------------------------------------------------------------------ rings and the plume table
@functools.lru_cache(maxsize=None)
def _plume_mask():
    m = np.zeros((96, 160), dtype=np.uint8)
    y, x = np.mgrid[0:96, 0:160]
    m[(y - 20) ** 2 + (x - 30) ** 2 <= 36] = 1                    # 1: a disc
    m[40:52, 60:75] = 1                                           # 2 and 3: three pixels apart, their rings compete
    m[40:50, 78:90] = 1
    m[(y - 75) ** 2 + (x - 130) ** 2 <= 25] = 1                   # its whole ring will be NaN
    m[90:96, 5:12] = 1                                            # at the border: a clipped ring
    rng = np.random.default_rng(3)
    m[60:66, 95:103] = rng.random((6, 8)) < 0.7                   # a ragged blob
    m.setflags(write=False)
    return m


def plume_mask():
    return np.array(_plume_mask())


RING, GAP = 6.0, 1.5


@functools.lru_cache(maxsize=None)
def ring_case():
    """(labels, count, reference rings, mag1c with NaNs in the ring of plume 1 and an all-NaN ring of the second disc, prob)"""
    lab, n = PU.scipy_label(_plume_mask() != 0, 2)
    rings = NU.rings_ref(lab, RING, GAP)
    rng = np.random.default_rng(41)
    mf = (600.0 * rng.standard_normal(lab.shape) + 200.0).astype(np.float32)
    disc2 = int(lab[75, 130])
    first = np.flatnonzero(rings.reshape(-1) == int(lab[20, 30]))
    mf.reshape(-1)[first[::3]] = np.nan
    mf[rings == disc2] = np.nan
    mf[44, 62], mf[46, 66] = np.inf, np.nan                       # non-finite values inside a plume
    prob = rng.random(lab.shape).astype(np.float32)
    for a in (lab, rings, mf, prob):
        a.setflags(write=False)
    return lab, n, rings, mf, prob


def test_background_rings(hip):
    from starcop_amd import plumes
    lab, n, rings, _, _ = ring_case()
    assert n == 6 and all((rings == k).any() for k in range(1, n + 1))
    between = rings[40:50, 75:78]                                  # the three columns between plumes 2 and 3: gap, then both rings
    assert set(np.unique(between).tolist()) <= {0, int(lab[45, 65]), int(lab[45, 80])}
    got = plumes.background_rings(dev(lab), RING, GAP)
    assert got.dtype == torch.int32 and np.array_equal(host(got), rings)
    for ring_px, gap_px in ((3, 0), (16, 2), (70, 8.5), (1, 0)):
        assert np.array_equal(host(plumes.background_rings(dev(lab), ring_px, gap_px)), NU.rings_ref(lab, ring_px, gap_px)), (ring_px, gap_px)
    pair = np.stack([lab, np.zeros_like(lab)])
    got = plumes.background_rings(pair.astype(np.int64), RING, GAP)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got[0], rings) and not got[1].any()


def _ring_columns(lab, n, rings, mf, table, pixel_area_m2):
    """the ring columns of the rows of ``table`` and their tolerances, from float64 sums over the reference ring"""
    cols = {c: [] for c in ("bg_px", "mag1c_bg_mean", "mag1c_sum_bgsub", "ime_bgsub_ppmm_m2")}
    tol = {c: [] for c in cols}
    for k in table["plume_id"].to_numpy():
        v = mf[rings == k].astype(np.float64)
        area = v.size
        v = v[np.isfinite(v)]
        inside = mf[lab == k].astype(np.float64)
        pa = inside.size
        inside = inside[np.isfinite(inside)]
        s, sa = math.fsum(inside), math.fsum(np.abs(inside))
        tol_s = pa * 2.0 ** -50 * sa
        mean = math.fsum(v) / v.size if v.size else np.nan
        tol_mean = (area * 2.0 ** -50 * math.fsum(np.abs(v)) / v.size + 2.0 ** -52 * abs(mean)) if v.size else 0.0
        sub = s - mean * inside.size
        tol_sub = tol_s + inside.size * tol_mean + 2.0 ** -52 * abs(mean * inside.size) + 2.0 ** -52 * abs(sub) if v.size else 0.0
        for c, val, t in (("bg_px", v.size, 0), ("mag1c_bg_mean", mean, tol_mean), ("mag1c_sum_bgsub", sub, tol_sub),
                          ("ime_bgsub_ppmm_m2", sub * pixel_area_m2, tol_sub * pixel_area_m2 + 2.0 ** -52 * abs(sub * pixel_area_m2) if v.size else 0.0)):
            cols[c].append(val)
            tol[c].append(t)
    return {c: np.asarray(v) for c, v in cols.items()}, {c: np.asarray(v) for c, v in tol.items()}


def test_plume_table_background_ring(hip):
    from starcop_amd import plumes
    lab, n, rings, mf, prob = ring_case()
    mask = plume_mask()
    gt, area = (500000.0, 5.0, 0.0, 4100000.0, 0.0, -5.0), 25.0
    kw = dict(mag1c=dev(mf), prob=dev(prob), geotransform=gt, pixel_area_m2=area)
    today = plumes.plume_table(dev(mask), **kw)
    PU.assert_table(today, PU.oracle_table(mask, mag1c=mf, prob=prob, geotransform=gt, pixel_area_m2=area))
    assert plumes.plume_table(dev(mask), background_ring_px=None, **kw).equals(today)
    table = plumes.plume_table(dev(mask), background_ring_px=RING, background_gap_px=GAP, **kw)
    new = ["bg_px", "mag1c_bg_mean", "mag1c_sum_bgsub", "ime_bgsub_ppmm_m2"]
    at = list(today.columns).index("ime_ppmm_m2") + 1
    assert list(table.columns) == list(today.columns)[:at] + new + list(today.columns)[at:]
    assert table.drop(columns=new).equals(today)
    want, tol = _ring_columns(lab, n, rings, mf, table, area)
    assert len(table) == n
    for c in new:
        got = table[c].to_numpy()
        print(c, got, want[c], tol[c])
        if c == "bg_px":
            assert got.dtype == np.int64 and np.array_equal(got, want[c])
            continue
        assert np.array_equal(np.isnan(got), np.isnan(want[c])), c
        ok = ~np.isnan(want[c])
        assert (np.abs(got[ok] - want[c][ok]) <= tol[c][ok]).all(), (c, got, want[c], tol[c])
    disc2 = int(lab[75, 130]) - 1
    assert table["bg_px"][disc2] == 0 and np.isnan(table["mag1c_bg_mean"][disc2]) and np.isnan(table["mag1c_sum_bgsub"][disc2])
    assert 0 < table["bg_px"][int(lab[20, 30]) - 1] < int((rings == lab[20, 30]).sum())
    no_area = plumes.plume_table(mask, mag1c=np.array(mf), background_ring_px=RING, background_gap_px=GAP)       # numpy in
    assert "ime_bgsub_ppmm_m2" not in no_area.columns and no_area["mag1c_sum_bgsub"].equals(table["mag1c_sum_bgsub"])
    with pytest.raises(ValueError):
        plumes.plume_table(dev(mask), prob=dev(prob), background_ring_px=RING)


# ------------------------------------------------------------------------------------------------ products and pipeline
def test_annotate_plume_background(hip):
    from starcop_amd import plumes, products
    lab, n, rings, mf, prob = ring_case()
    mask = dev(plume_mask())
    plain, ringed = {}, {}
    products.annotate(plain, mask, dev(mf), dev(prob), plumes=True)
    products.annotate(ringed, mask, dev(mf), dev(prob), plumes=True, plume_background={"ring_px": RING, "gap_px": GAP})
    assert plain["plumes"].equals(plumes.plume_table(mask, mag1c=dev(mf), prob=dev(prob)))
    assert ringed["plumes"].equals(plumes.plume_table(mask, mag1c=dev(mf), prob=dev(prob), background_ring_px=RING, background_gap_px=GAP))
    assert "bg_px" in ringed["plumes"].columns and "bg_px" not in plain["plumes"].columns
    with pytest.raises(ValueError):
        products.annotate({}, mask, dev(mf), dev(prob), plumes=True, plume_background={"ring": 4})
    with pytest.raises(ValueError):
        products.annotate({}, mask, None, dev(prob), plumes=True, plume_background={"ring_px": 4})


def test_aviris_scene_predict_plume_background(hip, tmp_path):
    """a 70 x 100 ENVI flight line with a mag1c.tif beside it: plumes.csv gains the ring columns, and without the keyword no
    byte of any file changes"""
    import pandas as pd
    import plume_scene_util as SU
    from starcop_amd import io_formats, pipeline, plumes
    from test_gpu_plume_scene import _model
    H, W = 70, 100
    model = _model(bias=-0.93)
    valid = SU.strip_mask(H, W, centre=30.0, slope=0.3, half_width=25.0)
    planes = SU.flight_line(H, W, 61, valid=valid)[0]
    cube = np.stack([planes[3], planes[2], planes[1]], axis=-1)
    folder = SU.write_flight_line(str(tmp_path / "ang20190101t180000_rdn"), cube, np.array([460.0, 550.0, 640.0]))
    io_formats.write_tiff(os.path.join(folder, "mag1c.tif"), planes[0], blocksize=128, extra_tags={42113: (2, ("-9999",))})
    kw = dict(toa_correction_factor=1.037, tile=32, halo=32, plumes=True)
    names = ("plumes.csv", "pred.tif", "predbinary.tif")

    def read(sub):
        return [open(str(tmp_path / sub / n), "rb").read() for n in names]
    before = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "before"), **kw)
    bg = {"ring_px": 8, "gap_px": 1}
    out = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "ring"), plume_background=bg, **kw)
    pipeline.aviris_scene_predict(model, folder, str(tmp_path / "after"), plume_background=None, **kw)
    assert read("after") == read("before")
    assert read("ring")[1:] == read("before")[1:]
    assert sorted(os.path.basename(p) for p in out["files"]) == sorted(names)
    csv = pd.read_csv(str(tmp_path / "ring" / "plumes.csv"))
    old = pd.read_csv(str(tmp_path / "before" / "plumes.csv"))
    new = ["bg_px", "mag1c_bg_mean", "mag1c_sum_bgsub", "ime_bgsub_ppmm_m2"]
    assert len(csv) >= 1 and [c for c in csv.columns if c not in old.columns] == new
    assert csv.drop(columns=new).equals(old) and before["plumes"].equals(out["plumes"].drop(columns=new))
    table = plumes.plume_table(out["pred_binary"], mag1c=out["mf"], prob=out["prediction"], geotransform=(500000.0, 5.0, 0.0, 4100000.0, 0.0, -5.0),
                               pixel_area_m2=25.0, background_ring_px=8, background_gap_px=1)
    assert table.equals(out["plumes"])
    plumes.write_plumes(table, str(tmp_path / "want.csv"))
    assert open(str(tmp_path / "ring" / "plumes.csv")).read() == open(str(tmp_path / "want.csv")).read()
    with pytest.raises(ValueError):
        pipeline.aviris_scene_predict(model, folder, str(tmp_path / "bad"), plume_background={"ring_px": 8, "width": 2}, **kw)
    assert not os.path.exists(str(tmp_path / "bad"))
