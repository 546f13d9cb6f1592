"""Whole AVIRIS-NG flight lines through the binary plume model on the GPU: sc_scene_gather_planes (windows of the virtual
reflect-padded scene cut from the products' own planes, fill -> 0 / scale / clip), sc_scene_core_counts (which cores hold data),
sc_head_conv_fwd_mosaic_prob (the 1-class head writing sigmoid and mask of the cores into mosaics), ModelModule.predict_scene and
pipeline.aviris_scene_predict against their numpy restatements (tests/plume_scene_util.py), the float64 CPU oracle and
ModelModule.predict."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import plume_scene_util as U  # noqa: E402
from hip_ops import DEV, dev  # noqa: E402
from oracle import host_ref  # noqa: E402
from oracle.unet_ref import UnetMobileNetV2  # noqa: E402
from scene_util import padded_scene  # noqa: E402
from starcop_amd import io_formats, model_module as mm, pipeline, plumes, sentinel2  # noqa: E402
from starcop_amd._lib import check, ptr, stream  # noqa: E402
from test_gpu_multiclass import _head_inputs  # noqa: E402

FILL = U.FILL


def _table(offsets, cores=None, dests=None):
    t = np.zeros((len(offsets), 8), dtype=np.int32)
    t[:, 0:2] = offsets
    if cores is not None:
        t[:, 2:6], t[:, 6:8] = cores, dests
    return t


# ------------------------------------------------------------------------------------------------ gather
def _gather(planes, pads, offsets, window, fills=None, scales=None, clips=None):
    """the call through a NaN-filled buffer with a guard vector on either side of the output"""
    n, P = len(offsets), len(planes)
    numel = n * P * window[0] * window[1]
    buf = torch.full((numel + 8,), float("nan"), device=DEV)
    out = buf[4:4 + numel].view(n, P, *window)
    tab = _table(offsets)
    got = sentinel2.scene_gather_planes(planes, pads, dev(torch.from_numpy(tab)), tab, 0, n, window, fills, scales, clips, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.isnan(buf[:4]).all() and torch.isnan(buf[4 + numel:]).all()
    assert not torch.isnan(out).any()
    return out.cpu().numpy()


def _product_planes(H, W, seed):
    """plane 0 dense (mag1c-like: fill + clip), planes 1-3 one (H, W, 3) buffer (column stride 3: fill + scale); ~10 % fill"""
    rng = np.random.default_rng(seed)
    mf = (600.0 * rng.standard_normal((H, W)) + 200.0).astype(np.float32)
    mf[0, 0], mf[H - 1, W - 1] = 20000.0, -0.0                  # above the clip; a negative zero is no fill and clips to itself
    rgb = rng.uniform(0.5, 12.0, size=(H, W, 3)).astype(np.float32)
    mf[rng.random((H, W)) < 0.1] = FILL
    rgb[rng.random((H, W, 3)) < 0.1] = FILL
    host = [mf, rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2]]
    cube = dev(torch.from_numpy(rgb))
    device = [dev(torch.from_numpy(mf)), cube[:, :, 0], cube[:, :, 1], cube[:, :, 2]]
    assert device[1].stride() == (3 * W, 3)
    return host, device, [FILL] * 4, [None, 1.037, 1.037, 1.037], [(0.0, 10000.0), None, None, None]


CASES = {"50x77": ((50, 77), ((7, 7), (9, 10)), [(0, 0)], (64, 96)),                                   # every fringe in one window
         "40x45": ((40, 45), ((12, 12), (9, 10)), [(0, 0), (0, 32), (32, 0), (32, 32), (16, 16)], (32, 32))}     # odd pad_left


@pytest.mark.parametrize("case", list(CASES))
def test_gather_planes(hip, case):
    """bit-equal to np.where(bits == fill, 0, x * float32(s)), np.clip, np.pad(reflect), slices"""
    (H, W), (pr, pc), offsets, window = CASES[case]
    assert (sentinel2.find_padding(H, 32), sentinel2.find_padding(W, 32)) == (pr, pc)
    host, device, fills, scales, clips = _product_planes(H, W, 41)
    got = _gather(device, (pr[0], pc[0]), offsets, window, fills, scales, clips)
    want = U.gather_planes_ref(host, fills, scales, clips, pr, pc, offsets, window)
    assert got.dtype == want.dtype == np.float32 and np.array_equal(U.bits(got), U.bits(want))
    assert (got[:, 0] == 10000.0).any() and (got == 0).any() and float(got[:, 0].min()) == 0.0


@pytest.mark.parametrize("case", list(CASES))
def test_gather_planes_without_ops_equals_scene_gather(hip, case):
    (H, W), (pr, pc), offsets, window = CASES[case]
    _, device, _, _, _ = _product_planes(H, W, 42)
    got = _gather(device[1:], (pr[0], pc[0]), offsets, window)
    tab = _table(offsets)
    src = torch.stack(device[1:])
    want = sentinel2.scene_gather(src, (pr[0], pc[0]), dev(torch.from_numpy(tab)), tab, 0, len(offsets), window)
    assert np.array_equal(U.bits(got), U.bits(want.cpu().numpy()))
    assert (got == FILL).any()


# ------------------------------------------------------------------------------------------------ core counts
STRIP = dict(centre=70.0, slope=0.25, half_width=60.0)         # at 150 x 217: empty cores at the right, a full one in the middle


@pytest.mark.parametrize("layout", ["dense", "interleaved"])
def test_core_counts(hip, layout):
    H, W = 150, 217
    plan = sentinel2.scene_windows(H, W, 64, 32)
    assert plan.offsets.shape[0] == 12
    valid = U.strip_mask(H, W, **STRIP)
    x = np.random.default_rng(43).standard_normal((H, W)).astype(np.float32)
    x[~valid] = FILL
    if layout == "dense":
        plane = dev(torch.from_numpy(x))
    else:
        cube = np.full((H, W, 3), 7.0, dtype=np.float32)
        cube[:, :, 1] = x
        plane = dev(torch.from_numpy(cube))[:, :, 1]
    tab = sentinel2.scene_table(plan)
    out = torch.full((14,), -7, dtype=torch.int32, device=DEV)
    got = sentinel2.scene_core_counts(plane, FILL, dev(torch.from_numpy(tab)), tab, out=out[1:13])
    torch.cuda.synchronize()
    assert out[0] == -7 and out[13] == -7
    want = U.core_counts_ref(x, FILL, plan)
    areas = (plan.cores[:, 1] - plan.cores[:, 0]) * (plan.cores[:, 3] - plan.cores[:, 2])
    print("core counts:", want.tolist(), "areas:", areas.tolist())
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want == 0).any() and (want == areas).any() and int(want.sum()) == int(valid.sum())


# ------------------------------------------------------------------------------------------------ mosaic head
def _head_reference(hip, src, wd, bd, N, Cin, H, W):
    """sc_head_conv_fwd followed by sc_threshold_masks(ge0 = 0) on the same inputs"""
    logits = torch.full((N, 1, H, W), float("nan"), device=DEV)
    check(hip.sc_head_conv_fwd(C.byref(src), ptr(wd), ptr(bd), ptr(logits), N, Cin, H, W, stream()))
    pred = torch.empty((N, 1, H, W), device=DEV)
    pb = torch.empty((N, 1, H, W), dtype=torch.int64, device=DEV)
    check(hip.sc_threshold_masks(ptr(logits), None, 0, ptr(pred), ptr(pb), None, None, N, H * W, stream()))
    torch.cuda.synchronize()
    return pred[:, 0].cpu(), pb[:, 0].cpu().to(torch.uint8)


@pytest.mark.parametrize("Cin", [16, 8])
def test_mosaic_prob_head(hip, Cin):
    """N = 3, 32 x 64 windows: a ragged core at the origin, one that ends at the window's far corner and an empty one, into
    40 x 101 mosaics with odd pitches (element stores next to the wide ones): the bits of sc_head_conv_fwd + sc_threshold_masks,
    nothing else touched; with a valid plane, prob only, mask only; bad tables refused"""
    N, H, W, NODATA = 3, 32, 64, -9999.0
    x, w, b, src_of, _ = _head_inputs(N, Cin, 1, H, W, "affine")
    src, wd, bd = src_of(dev(x)), dev(w), dev(b)
    pred, pb = _head_reference(hip, src, wd, bd, N, Cin, H, W)
    assert 0 < int(pb.sum()) < pb.numel()
    cores = [(0, 19, 0, 37), (5, 32, 3, 64), (7, 7, 0, 64)]
    dests = [(0, 0), (13, 40), (0, 0)]
    tab = _table([(0, 0)] * N, cores, dests)
    tdev = dev(torch.from_numpy(tab))
    want_p = torch.full((40, 101), float("nan"))
    want_m = torch.full((40, 101), 255, dtype=torch.uint8)
    want_p[0:19, 0:37], want_m[0:19, 0:37] = pred[0, 0:19, 0:37], pb[0, 0:19, 0:37]
    want_p[13:40, 40:101], want_m[13:40, 40:101] = pred[1, 5:32, 3:64], pb[1, 5:32, 3:64]
    valid_h = np.random.default_rng(44).standard_normal((40, 101)).astype(np.float32)
    valid_h[np.random.default_rng(45).random((40, 101)) < 0.3] = FILL
    hole = torch.from_numpy(valid_h == FILL)
    valid = dev(torch.from_numpy(valid_h))

    def run(with_prob, with_mask, with_valid, table=tab, table_dev=tdev, n=N):
        pbuf = torch.full((40, 103), float("nan"), device=DEV)
        mbuf = torch.full((40, 105), 255, dtype=torch.uint8, device=DEV)
        check(hip.sc_head_conv_fwd_mosaic_prob(C.byref(src), ptr(wd), ptr(bd), ptr(pbuf) if with_prob else None, 103,
                                               ptr(mbuf) if with_mask else None, 105, 40, 101, ptr(valid) if with_valid else None,
                                               valid.stride(0), valid.stride(1), U.fill_bits(FILL), NODATA, ptr(table_dev),
                                               table.ctypes.data, n, Cin, H, W, stream()))
        torch.cuda.synchronize()
        assert torch.isnan(pbuf[:, 101:]).all() and bool((mbuf[:, 101:] == 255).all())
        return pbuf[:, :101].cpu(), mbuf[:, :101].cpu()

    def same(a, b_):
        return torch.equal(a.view(torch.int32), b_.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b_)
    p, m = run(True, True, False)
    assert same(p, want_p) and same(m, want_m)
    p, m = run(True, False, False)
    assert same(p, want_p) and bool((m == 255).all())
    p, m = run(False, True, False)
    assert torch.isnan(p).all() and same(m, want_m)
    written = ~torch.isnan(want_p)
    assert int((written & hole).sum()) > 50 and int((written & ~hole).sum()) > 50
    vp = torch.where(written & hole, torch.tensor(NODATA), want_p)
    vm = torch.where(written & hole, torch.tensor(0, dtype=torch.uint8), want_m)
    p, m = run(True, True, True)
    assert same(p, vp) and same(m, vm)
    # a core that leaves the plane / a destination that leaves the mosaic: refused before anything is launched
    for bad_core, bad_dest in (((0, 33, 0, 37), (0, 0)), ((0, 19, 0, 37), (22, 0)), ((0, 19, 0, 37), (0, 65))):
        t2 = _table([(0, 0)], [bad_core], [bad_dest])
        with pytest.raises(ValueError, match="sc_head_conv_fwd_mosaic_prob"):
            run(True, True, False, t2, dev(torch.from_numpy(t2)), 1)


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _oracle():
    """the 4-band / 1-class oracle with seeded weights and the BatchNorm recipe of test_gpu_multiclass._oracle_case (seeds 0 / 1),
    head bias 0; float32 and float64 copies.  Computed once, never modified."""
    torch.manual_seed(0)
    ref = UnetMobileNetV2(4, 1).eval()
    g = torch.Generator().manual_seed(1)
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    with torch.no_grad():
        ref.segmentation_head[0].bias.zero_()
    return ref, copy.deepcopy(ref).double()


def _model(bias=0.0):
    torch.manual_seed(0)
    model = mm.ModelModule(mm.default_settings(pos_weight=1))
    sd = {k: v.clone() for k, v in _oracle()[0].state_dict().items()}
    sd["segmentation_head.0.bias"] = torch.tensor([bias], dtype=torch.float32)
    model.network.load_state_dict(sd, strict=True)
    return model.to(DEV).eval()


def _forward_one(model):
    def forward(w):
        with torch.no_grad():
            m = mm.masks_from_logits(model(torch.from_numpy(w).to(DEV)))
        return m["prediction"][0, 0].cpu().numpy(), m["pred_binary"][0, 0].cpu().numpy()
    return forward


def _same_bits(a, b):
    return np.array_equal(U.bits(a), U.bits(b))


def test_predict_scene_small_halo(hip):
    """(4, 150, 217), tile 64, halo 32, batch 4: 3 x 4 windows of 128 x 128 against the restatement that cuts the same windows in
    numpy, runs the eval forward one window at a time, applies masks_from_logits, pastes the cores and sets the fill pixels to
    nodata / 0.  The batch size and skipping the empty windows change no bit."""
    model = _model(bias=-0.93)
    H, W = 150, 217
    planes, fills, scales, clips, valid = U.flight_line(H, W, 51, valid=U.strip_mask(H, W, **STRIP))
    plan = sentinel2.scene_windows(H, W, 64, 32)
    assert plan.window == (128, 128) and plan.offsets.shape[0] == 12
    got = model.predict_scene(planes, fill_value=FILL, scales=scales, clips=clips, tile=64, halo=32, batch=4)
    assert isinstance(got["prediction"], np.ndarray) and got["prediction"].shape == (H, W) and got["prediction"].dtype == np.float32
    assert got["pred_binary"].shape == (H, W) and got["pred_binary"].dtype == np.uint8
    want_p, want_m = U.predict_scene_ref(_forward_one(model), planes, fills, scales, clips, plan)
    share = float(want_m[valid].mean())
    differ = U.bits(got["prediction"]) != U.bits(want_p)
    print(f"windows {got['windows']}, run {got['windows_run']}; plume share of the valid pixels {share:.3f}; "
          f"{int(differ.sum())} probabilities differ in their bits, max |diff| {float(np.abs(got['prediction'] - want_p).max()):.3e}; "
          f"{int((got['pred_binary'] != want_m).sum())} mask pixels differ")
    assert 0.02 < share < 0.98
    assert (got["prediction"][~valid] == FILL).all() and not got["pred_binary"][~valid].any()
    assert _same_bits(got["prediction"], want_p) and np.array_equal(got["pred_binary"], want_m)
    assert got["windows"] == 12 and got["windows_run"] < 12
    assert got["windows_run"] == int((U.core_counts_ref(planes[0], FILL, plan) > 0).sum())
    b5 = model.predict_scene(planes, fill_value=FILL, scales=scales, clips=clips, tile=64, halo=32, batch=5)
    assert _same_bits(b5["prediction"], got["prediction"]) and np.array_equal(b5["pred_binary"], got["pred_binary"])
    full = model.predict_scene(planes, fill_value=FILL, scales=scales, clips=clips, tile=64, halo=32, batch=4, skip_empty=False)
    assert full["windows_run"] == full["windows"] == 12
    assert _same_bits(full["prediction"], got["prediction"]) and np.array_equal(full["pred_binary"], got["pred_binary"])
    # device planes in (the three bands read in place from one (H, W, 3) buffer) -> device tensors out
    cube = torch.from_numpy(np.stack(planes[1:], axis=-1)).to(DEV)
    d = model.predict_scene([torch.from_numpy(planes[0]).to(DEV), cube[:, :, 0], cube[:, :, 1], cube[:, :, 2]], fill_value=FILL,
                            scales=scales, clips=clips, tile=64, halo=32, batch=4)
    assert d["prediction"].is_cuda and d["pred_binary"].is_cuda and d["pred_binary"].dtype == torch.uint8
    assert _same_bits(d["prediction"].cpu().numpy(), got["prediction"]) and np.array_equal(d["pred_binary"].cpu().numpy(), got["pred_binary"])


def test_predict_scene_equals_the_whole_scene_forward(hip):
    """the exactness claim: (4, 790, 500), tile 96, halo 320 -> nine shifted 736 x 512 windows over the 800 x 512 padded scene (the
    padded scene is no wider than a window, so a core is a band of 96 rows), against the float64 oracle on the whole reflect-padded,
    normalised scene.  On the valid pixels
        |prediction - sigmoid(z64)| <= 0.25 * 1e-4 * max|z64| + 2^-23
    (the 1e-4 logit contract through the sigmoid's slope bound 1/4, plus one float32 rounding of a value <= 1),
    pred_binary == (z64 > 0) wherever |z64| >= 1e-4 max|z64|, and pred_binary == (ModelModule.predict > 0.5) outside those near
    ties.  Scene: seeds 0 / 1 (weights, BatchNorm) / 31 (data), valid where |x - (120 + 0.35 y)| < 110 from row 100 on (the line
    begins below the top of its rectangle, so the first core is empty), mag1c ~ 600 N(0, 1) + 200, radiance ~ U(0.5, 12) x 1.037;
    head bias = minus the median logit of the image.  Measured with these inputs (oracle on the CPU): 38.4 % of the pixels are valid, max|z64| = 0.577, 0.30 % of the valid
    pixels are near ties, 33.1 % are plume pixels, 1 of the 9 cores is empty."""
    H, W = 790, 500
    planes, fills, scales, clips, valid = U.flight_line(H, W, 31, valid=U.strip_mask(H, W, first_row=100))
    plan = sentinel2.scene_windows(H, W, 96, 320)
    assert plan.padded == (800, 512) and plan.window == (736, 512) and plan.offsets.shape[0] == 9
    x = U.prepare_planes(planes, fills, scales, clips)
    xn = host_ref.normalize_x(x[None], mm.default_settings().dataset.input_products)[0]
    with torch.no_grad():
        z0 = _oracle()[1](torch.from_numpy(padded_scene(xn, plan)).double()[None])[0, 0]
    z0 = z0[plan.pad_rows[0]:plan.pad_rows[0] + H, plan.pad_cols[0]:plan.pad_cols[0] + W]
    bias = np.float32(-float(z0.median()))
    z64 = (z0 + float(bias)).numpy()
    model = _model(bias=float(bias))
    zmax = float(np.abs(z64).max())
    sure = np.abs(z64) >= 1e-4 * zmax
    near = 1.0 - float(sure[valid].mean())
    share = float((z64 > 0)[valid].mean())
    empty = int((U.core_counts_ref(planes[0], FILL, plan) == 0).sum())
    print(f"valid share {float(valid.mean()):.3f}; max|z64| {zmax:.4f}; near ties {100 * near:.3f} % of the valid pixels; "
          f"plume share {100 * share:.1f} %; {empty} of {plan.offsets.shape[0]} cores are empty")
    assert near <= 0.01 and 0.05 <= share <= 0.95 and empty >= 1
    got = model.predict_scene(planes, fill_value=FILL, scales=scales, clips=clips, tile=96, halo=320)
    assert got["windows"] == 9 and got["windows_run"] == 9 - empty
    p64 = 1.0 / (1.0 + np.exp(-z64))
    err = np.abs(got["prediction"].astype(np.float64) - p64)[valid]
    bound = 0.25 * 1e-4 * zmax + 2.0 ** -23
    wrong = int((got["pred_binary"].astype(bool) != (z64 > 0))[valid & sure].sum())
    print(f"max |prediction - sigmoid(z64)| {float(err.max()):.3e} (bound {bound:.3e}); {wrong} mask pixels differ outside the near ties")
    assert float(err.max()) <= bound
    assert wrong == 0
    assert (got["prediction"][~valid] == FILL).all() and not got["pred_binary"][~valid].any()
    whole = model.predict(x) > 0.5
    differ = (got["pred_binary"].astype(bool) != whole) & valid
    print(f"predict_scene vs predict: {int(differ.sum())} valid pixels differ, {int((differ & sure).sum())} of them outside the near ties")
    assert int((differ & sure).sum()) == 0


# ------------------------------------------------------------------------------------------------ file to file
def test_aviris_scene_predict_files(hip, tmp_path):
    """a 70 x 100 ENVI flight line with a mag1c.tif beside it -> pred.tif / predbinary.tif / plumes.csv"""
    H, W = 70, 100
    model = _model(bias=-0.93)
    wl = np.array([440.0, 461.0, 500.0, 549.0, 600.0, 641.0, 700.0])
    valid = U.strip_mask(H, W, centre=30.0, slope=0.3, half_width=25.0)        # the last 32-column core band holds no data
    rng = np.random.default_rng(61)
    cube = rng.uniform(0.5, 12.0, size=(H, W, wl.size)).astype(np.float32)
    cube[~valid] = FILL
    mf = (600.0 * rng.standard_normal((H, W)) + 200.0).astype(np.float32)
    mf[~valid] = FILL
    folder = U.write_flight_line(str(tmp_path / "ang20190101t180000_rdn"), cube, wl)
    io_formats.write_tiff(os.path.join(folder, "mag1c.tif"), mf, blocksize=128, extra_tags={42113: (2, ("-9999",))})
    out_folder = str(tmp_path / "out")
    kw = dict(toa_correction_factor=1.037, tile=32, halo=32)
    out = pipeline.aviris_scene_predict(model, folder, out_folder, plumes=True, **kw)
    assert sorted(os.path.basename(p) for p in out["files"]) == ["plumes.csv", "pred.tif", "predbinary.tif"]
    planes = [mf, cube[:, :, 5], cube[:, :, 3], cube[:, :, 1]]            # the bands nearest to 640 / 550 / 460 nm
    want = model.predict_scene(planes, fill_value=FILL, scales=[None, 1.037, 1.037, 1.037], clips=[(0.0, 10000.0), None, None, None],
                               tile=32, halo=32)
    pred, mask = out["prediction"].cpu().numpy(), out["pred_binary"].cpu().numpy()
    assert _same_bits(pred, want["prediction"]) and np.array_equal(mask, want["pred_binary"])
    assert out["windows"] == want["windows"] and out["windows_run"] == want["windows_run"] < out["windows"]
    assert 0 < int(mask.sum()) < int(valid.sum()) and np.array_equal(out["mf"].cpu().numpy(), mf)
    geo = io_formats.envi_geo_tags(io_formats.read_envi_header(os.path.join(folder, os.path.basename(folder) + "_img.hdr")))
    assert set(geo) == {33550, 33922, 34735}
    for name, arr, dtype in (("pred.tif", pred, np.float32), ("predbinary.tif", mask, np.uint8)):
        info = io_formats.tiff_info(os.path.join(out_folder, name))
        back = io_formats.read_tiff(os.path.join(out_folder, name), info=info)
        assert back.shape == (1, H, W) and back.dtype == dtype and info.tiled and info.block == (128, 128)
        assert _same_bits(back[0], arr) if dtype == np.float32 else np.array_equal(back[0], arr)
        for t, v in geo.items():
            assert info.tags[t][1] == v[1], (name, t)
        assert ("Plume probability" if name == "pred.tif" else "Plume mask") in info.tags[42112][1][0]
        assert (float(info.tags[42113][1][0]) == FILL) if name == "pred.tif" else (42113 not in info.tags)
    table = plumes.plume_table(mask, mag1c=mf, prob=pred, geotransform=(500000.0, 5.0, 0.0, 4100000.0, 0.0, -5.0), pixel_area_m2=25.0)
    assert len(table) >= 1 and "x" in table.columns and "ime_ppmm_m2" in table.columns
    plumes.write_plumes(table, str(tmp_path / "want.csv"))
    assert open(os.path.join(out_folder, "plumes.csv")).read() == open(str(tmp_path / "want.csv")).read()
    # existing files are skipped without overwrite
    stamp = {p: os.stat(p).st_mtime_ns for p in out["files"]}
    again = pipeline.aviris_scene_predict(model, folder, out_folder, plumes=True, **kw)
    assert again["files"] == [] and {p: os.stat(p).st_mtime_ns for p in stamp} == stamp
    os.remove(os.path.join(out_folder, "pred.tif"))
    again = pipeline.aviris_scene_predict(model, folder, out_folder, plumes=True, **kw)
    assert [os.path.basename(p) for p in again["files"]] == ["pred.tif"]
    # the acquisition-date factor from the folder name and a solar altitude
    import datetime
    from starcop_amd import aviris
    when = datetime.datetime(2019, 1, 1, 18, 0, 0, tzinfo=datetime.timezone.utc)
    f = float(aviris.observation_date_correction_factor(when, 50.0))
    a = pipeline.aviris_scene_predict(model, folder, solar_altitude=50.0, tile=32, halo=32)
    b = pipeline.aviris_scene_predict(model, folder, toa_correction_factor=f, tile=32, halo=32)
    assert "files" not in a and torch.equal(a["prediction"], b["prediction"]) and not torch.equal(a["prediction"], out["prediction"])


def test_aviris_scene_predict_computes_and_writes_mag1c(hip, tmp_path):
    """no mag1c.tif beside the cube: the matched filter runs from ``<name>_glt`` (96 x 40 x 101 bands, 23 detector groups: every
    group has more pixels than the 74 kept bands; tile 32 / halo 32 cut it into 3 x 2 cores of one 96 x 64 window) and ``{out_folder}/mag1c.tif`` is the
    file ``aviris_scene_mag1c`` writes, byte for byte, plain; as a COG the same pixels and tags"""
    from test_gpu_cog import _same_product
    folder = U.write_mag1c_flight_line(tmp_path)[0]
    assert not os.path.exists(os.path.join(folder, "mag1c.tif"))
    model = _model(bias=-0.93)
    kw = dict(toa_correction_factor=1.037, tile=32, halo=32)
    want_path = str(tmp_path / "want_mag1c.tif")
    want_mf, _ = pipeline.aviris_scene_mag1c(folder, want_path)
    names = ["mag1c.tif", "pred.tif", "predbinary.tif"]

    def read(sub):
        return [open(str(tmp_path / sub / n), "rb").read() for n in names]
    out = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "a"), **kw)
    assert out["files"] == [str(tmp_path / "a" / n) for n in names]
    first = read("a")
    assert first[0] == open(want_path, "rb").read()
    assert out["mf"].dtype == want_mf.dtype == torch.float32 and torch.equal(out["mf"].view(torch.int32), want_mf.view(torch.int32))
    stamp = {p: os.stat(p).st_mtime_ns for p in out["files"]}
    again = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "a"), **kw)
    assert again["files"] == [] and {p: os.stat(p).st_mtime_ns for p in stamp} == stamp
    c = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "c"), cog=dict(overview_min_size=32), **kw)
    assert c["files"] == [str(tmp_path / "c" / n) for n in names]
    info = _same_product(str(tmp_path / "c" / "mag1c.tif"), str(tmp_path / "a" / "mag1c.tif"))
    plain = io_formats.tiff_info(str(tmp_path / "a" / "mag1c.tif"))
    assert info.tags[42113] == plain.tags[42113] and info.tags[42113][1] == ("-9999",)
    assert info.tags[42112] == plain.tags[42112] and '<Item name="mag1c">acfwl1mf</Item>' in info.tags[42112][1][0]
    pipeline.aviris_scene_predict(model, folder, str(tmp_path / "b"), **kw)
    assert read("b") == first
