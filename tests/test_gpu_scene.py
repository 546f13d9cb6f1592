"""Whole-scene cloud masking on the GPU: sc_scene_gather (windows of the virtual reflect-padded scene, uint16 / float32 -> float32),
sc_head_conv_fwd_k_mosaic (the class-index head writing cores into a mosaic) and CDModel.predict_scene / cloud_mask_file against
their numpy restatements (tests/scene_util.py), the float64 CPU oracle and CDModel.predict."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hip_ops import DEV, dev  # noqa: E402
from scene_util import gather_ref, padded_scene, paste_cores  # noqa: E402
from starcop_amd import io_formats, sentinel2  # noqa: E402
from starcop_amd._lib import check, ptr, stream  # noqa: E402
from test_gpu_multiclass import _check_classes, _head_inputs, _oracle_case, _run_head  # noqa: E402


# ------------------------------------------------------------------------------------------------ gather
def _table(offsets, cores=None, dests=None):
    n = len(offsets)
    t = np.zeros((n, 8), dtype=np.int32)
    t[:, 0:2] = offsets
    if cores is not None:
        t[:, 2:6], t[:, 6:8] = cores, dests
    return t


def _gather(src, pads, offsets, window, scale):
    """the call through a NaN-filled buffer with a guard vector on either side of the output"""
    n, Cn = len(offsets), src.shape[0]
    numel = n * Cn * window[0] * window[1]
    buf = torch.full((numel + 8,), float("nan"), device=DEV)
    out = buf[4:4 + numel].view(n, Cn, *window)
    tab = _table(offsets)
    got = sentinel2.scene_gather(src, pads, dev(torch.from_numpy(tab)), tab, 0, n, window, scale, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.isnan(buf[:4]).all() and torch.isnan(buf[4 + numel:]).all()
    assert not torch.isnan(out).any()
    return out.cpu().numpy()


@pytest.mark.parametrize("scale", [1.0, 1e-4])
def test_gather_uint16_whole_padded_scene(hip, scale):
    """(13, 50, 77) -> pads (7, 7) / (9, 10), one 64 x 96 window: every fringe, 8-byte loads where a row's columns line up"""
    dn = np.random.default_rng(11).integers(0, 65536, size=(13, 50, 77)).astype(np.uint16)
    pr, pc = sentinel2.find_padding(50, 32), sentinel2.find_padding(77, 32)
    assert (pr, pc) == ((7, 7), (9, 10))
    src = dev(torch.from_numpy(dn.view(np.int16)))
    got = _gather(src, (pr[0], pc[0]), [(0, 0)], (64, 96), scale)
    want = gather_ref(dn, pr, pc, [(0, 0)], (64, 96), scale)
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want)


@pytest.mark.parametrize("scale", [1.0, 1e-4])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
def test_gather_float32_five_windows(hip, layout, scale):
    """(3, 40, 45) read in place through an (H, W, C) buffer (column stride 3) and as dense planes (odd pad_left: unaligned source
    columns); the four corner windows and the interior one of the 64 x 64 padded scene"""
    x = np.random.default_rng(12).standard_normal((3, 40, 45)).astype(np.float32)
    pr, pc = sentinel2.find_padding(40, 32), sentinel2.find_padding(45, 32)
    assert (pr, pc) == ((12, 12), (9, 10))
    if layout == "interleaved":
        src = dev(torch.from_numpy(np.ascontiguousarray(x.transpose(1, 2, 0)))).permute(2, 0, 1)
        assert src.stride() == (1, 135, 3)
    else:
        src = dev(torch.from_numpy(x))
    offsets = [(0, 0), (0, 32), (32, 0), (32, 32), (16, 16)]
    got = _gather(src, (pr[0], pc[0]), offsets, (32, 32), scale)
    assert np.array_equal(got, gather_ref(x, pr, pc, offsets, (32, 32), scale))


def test_gather_64bit_channel_stride(hip):
    """a (2, 40, 45) uint16 view whose channel stride is 2^31 + 64 elements: only the two planes of the 4.3 GB buffer are written"""
    cs = 2 ** 31 + 64
    big = torch.empty(cs + 40 * 45, dtype=torch.int16, device=DEV)
    src = big.as_strided((2, 40, 45), (cs, 45, 1))
    dn = np.random.default_rng(13).integers(0, 65536, size=(2, 40, 45)).astype(np.uint16)
    src.copy_(torch.from_numpy(dn.view(np.int16)))
    pr, pc = sentinel2.find_padding(40, 32), sentinel2.find_padding(45, 32)
    got = _gather(src, (pr[0], pc[0]), [(0, 0)], (64, 64), 1.0)
    assert np.array_equal(got, gather_ref(dn, pr, pc, [(0, 0)], (64, 64)))
    del src, big


def test_gather_argument_checks(hip):
    src = dev(torch.zeros(3, 40, 45))
    tab = _table([(0, 0), (64, 32)])                    # the second window's last row would need a second reflection (84 > 2 * 40 - 1)
    tdev = dev(torch.from_numpy(tab))
    with pytest.raises(ValueError, match="leaves the reflect-padded scene"):
        sentinel2.scene_gather(src, (12, 9), tdev, tab, 0, 2, (32, 32))
    with pytest.raises(ValueError, match="larger than the pad"):
        sentinel2.scene_gather(src, (40, 9), tdev, tab, 0, 1, (32, 32))
    with pytest.raises(ValueError, match="multiple of 4"):
        sentinel2.scene_gather(src, (12, 9), tdev, tab, 0, 1, (32, 30))
    with pytest.raises(TypeError):
        sentinel2.scene_gather(src.to(torch.int32), (12, 9), tdev, tab, 0, 1, (32, 32))


# ------------------------------------------------------------------------------------------------ mosaic head
@pytest.mark.parametrize("Cin", [16, 8])
def test_mosaic_head(hip, Cin):
    """N = 3, K = 4, 32 x 64 windows: a ragged core at the origin, one that ends at the window's far corner and an empty one, into a
    40 x 101 mosaic (odd pitch: byte stores next to the 4-byte ones); the classes are those of sc_head_conv_fwd_k, nothing else is
    touched"""
    N, K, H, W = 3, 4, 32, 64
    x, w, b, src_of, _ = _head_inputs(N, Cin, K, H, W, "affine")
    src, wd, bd = src_of(dev(x)), dev(w), dev(b)
    _, classes = _run_head(hip, src, wd, bd, N, Cin, K, H, W, False, True)
    cores = [(0, 19, 0, 37), (5, 32, 3, 64), (7, 7, 0, 64)]
    dests = [(0, 0), (13, 40), (0, 0)]
    tab = _table([(0, 0)] * N, cores, dests)
    mosaic = torch.full((40, 101), 255, dtype=torch.uint8, device=DEV)
    check(hip.sc_head_conv_fwd_k_mosaic(C.byref(src), ptr(wd), ptr(bd), ptr(mosaic), 40, 101, 101, ptr(dev(torch.from_numpy(tab))),
                                        tab.ctypes.data, N, Cin, K, H, W, stream()))
    torch.cuda.synchronize()
    want = torch.full((40, 101), 255, dtype=torch.uint8)
    cl = classes.cpu()
    want[0:19, 0:37] = cl[0, 0:19, 0:37]
    want[13:40, 40:101] = cl[1, 5:32, 3:64]
    assert int(cl.max()) < K and len(torch.unique(cl)) > 1
    assert torch.equal(mosaic.cpu(), want)
    # a core that leaves the plane / a destination that leaves the mosaic: refused before anything is launched
    for bad_core, bad_dest in (((0, 33, 0, 37), (0, 0)), ((0, 19, 0, 37), (22, 0)), ((0, 19, 0, 37), (0, 65))):
        t2 = _table([(0, 0)], [bad_core], [bad_dest])
        with pytest.raises(ValueError, match="sc_head_conv_fwd_k_mosaic"):
            check(hip.sc_head_conv_fwd_k_mosaic(C.byref(src), ptr(wd), ptr(bd), ptr(mosaic), 40, 101, 101, ptr(dev(torch.from_numpy(t2))),
                                                t2.ctypes.data, 1, Cin, K, H, W, stream()))
    assert torch.equal(mosaic.cpu(), want)


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _model():
    sd = _oracle_case()[0]
    model = sentinel2.CDModel(device=DEV)
    model.load_state_dict({"model." + k: v for k, v in sd.items()}, strict=True)
    return model


def _restated_logits(model, bands, tile, halo, scale=1.0):
    """the same windows, cut in numpy, through the network's eval forward one at a time; cores pasted -> (K, H, W) fp32 logits"""
    _, H, W = bands.shape
    plan = sentinel2.scene_windows(H, W, tile, halo)
    wins = gather_ref(bands, plan.pad_rows, plan.pad_cols, plan.offsets.tolist(), plan.window, scale)
    with torch.no_grad():
        lg = np.stack([model.model(torch.from_numpy(w)[None].to(DEV))[0].cpu().numpy() for w in wins])
        cl = np.stack([model(torch.from_numpy(w)[None].to(DEV))[0].cpu().numpy() for w in wins])
    return plan, paste_cores(lg, plan, H, W), paste_cores(cl, plan, H, W)


def test_predict_scene_small_halo(hip):
    """(13, 150, 217), tile 64, halo 32, batch 4: 3 x 4 windows of 128 x 128 in three batches against the restatement that runs the
    same windows one by one and pastes the cores; the excluded near ties are those of the restatement's fp32 logits"""
    model = _model()
    bands = np.random.default_rng(21).standard_normal((13, 150, 217)).astype(np.float32)
    got = model.predict_scene(bands, tile=64, halo=32, batch=4)
    assert isinstance(got, np.ndarray) and got.shape == (150, 217) and got.dtype == np.uint8
    plan, logits, classes = _restated_logits(model, bands, 64, 32)
    assert plan.window == (128, 128) and plan.offsets.shape[0] == 12
    _check_classes(torch.from_numpy(got), torch.from_numpy(logits).double(), "predict_scene (tile 64, halo 32)")
    # the batch size changes nothing (every window is an item of its own to every layer in eval mode)
    assert np.array_equal(model.predict_scene(bands, tile=64, halo=32, batch=5), got)
    with pytest.raises(AssertionError, match="Expected 13 channels found 12"):
        model.predict_scene(bands[:12])
    with pytest.raises(TypeError):
        model.predict_scene(bands.astype(np.float64))
    with pytest.raises(RuntimeError, match="eval mode"):
        model.model.train().predict_classes_into(torch.zeros(1, 13, 32, 32, device=DEV), torch.zeros(32, 32, dtype=torch.uint8, device=DEV),
                                                 (torch.zeros(1, 8, dtype=torch.int32, device=DEV), np.zeros((1, 8), np.int32), 0))
    model.model.eval()


def test_predict_scene_equals_the_whole_scene_forward(hip):
    """the exactness claim: (13, 790, 500), tile 96, halo 320 -> nine shifted 736 x 512 windows over the 800 x 512 padded scene.
    With halo >= RECEPTIVE_HALO a core's logits are the whole-scene forward's, so the classes agree with the float64 oracle's logits of
    the whole reflect-padded scene, and with CDModel.predict, wherever the oracle's top-two gap is not a near tie.
    Measured on the CPU for this scene (seed 22): 0.002 % of the pixels are near ties; the classes hold 2.6 / 96.1 / 0.96 / 0.40 % of
    the pixels (10 125 / 379 498 / 3 800 / 1 577) -- the minority classes of this weight recipe come from the reflected border, so
    their share falls with the scene size (8.9 / 76.8 / 10.5 / 3.8 % at 150 x 217, 4.6 / 88.3 / 5.1 / 2.0 % at 300 x 420).  Both
    figures are printed; every class must keep at least 0.1 % (395 pixels) so that none goes untested."""
    model = _model()
    ref64 = _oracle_case()[1]
    bands = np.random.default_rng(22).standard_normal((13, 790, 500)).astype(np.float32)
    plan = sentinel2.scene_windows(790, 500, 96, 320)
    assert plan.padded == (800, 512) and plan.window == (736, 512) and plan.offsets.shape[0] == 9
    with torch.no_grad():
        logits64 = ref64(torch.from_numpy(padded_scene(bands, plan)).double()[None])[0]
    logits64 = logits64[:, plan.pad_rows[0]:plan.pad_rows[0] + 790, plan.pad_cols[0]:plan.pad_cols[0] + 500]
    counts = torch.bincount(logits64.argmax(0).flatten(), minlength=4).double()
    print("class shares of the oracle:", (counts / counts.sum()).tolist())
    assert bool((counts / counts.sum() >= 0.001).all())
    got = model.predict_scene(bands, tile=96, halo=320)
    _check_classes(torch.from_numpy(got), logits64, "predict_scene (tile 96, halo 320) vs the float64 oracle")
    whole = model.predict(bands)
    top = logits64.topk(2, dim=0).values
    sure = (top[0] - top[1]) >= 1e-4 * float(logits64.abs().max())
    differ = torch.from_numpy(got != whole)
    print(f"predict_scene vs predict: {int(differ.sum())} pixels differ, {int((differ & sure).sum())} of them outside the near ties")
    assert float(sure.double().mean()) >= 0.99
    assert int((differ & sure).sum()) == 0


def test_predict_scene_uint16(hip):
    """uint16 (13, 70, 100) with scale 1e-4, tile 32, halo 32, device tensor in -> device tensor out, bit-equal to the float32 scene
    dn.astype(float32) * float32(1e-4): the conversion and the one multiply happen in the gather"""
    model = _model()
    dn = np.random.default_rng(23).integers(0, 20000, size=(13, 70, 100)).astype(np.uint16)
    src = torch.from_numpy(dn.view(np.int16)).to(DEV).view(torch.uint16)
    got = model.predict_scene(src, tile=32, halo=32, scale=1e-4)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and got.shape == (70, 100)
    as_f32 = torch.from_numpy(dn.astype(np.float32) * np.float32(1e-4)).to(DEV)
    assert torch.equal(got, model.predict_scene(as_f32, tile=32, halo=32))
    assert len(torch.unique(got)) > 1
    assert np.array_equal(model.predict_scene(dn, tile=32, halo=32, scale=1e-4), got.cpu().numpy())


def test_cloud_mask_file(hip, tmp_path):
    model = _model()
    dn = np.random.default_rng(24).integers(0, 20000, size=(13, 70, 100)).astype(np.uint16)
    geo = {33550: (12, (10.0, 10.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 600000.0, 4500000.0, 0.0)),
           34735: (3, (1, 1, 0, 1, 3072, 0, 1, 32633))}
    src_tif, dst_tif = str(tmp_path / "s2.tif"), str(tmp_path / "mask.tif")
    io_formats.write_tiff(src_tif, dn, extra_tags=geo)
    mask = sentinel2.cloud_mask_file(src_tif, dst_tif, model, tile=32, halo=32, scale=1e-4)
    info = io_formats.tiff_info(dst_tif)
    back = io_formats.read_tiff(dst_tif, info=info)
    assert back.shape == (1, 70, 100) and back.dtype == np.uint8 and info.tiled and info.block == (128, 128)
    assert np.array_equal(back[0], mask) and np.array_equal(mask, model.predict_scene(dn, tile=32, halo=32, scale=1e-4))
    for t, v in geo.items():
        assert info.tags[t][1] == v[1], t
    meta = info.tags[42112][1][0]
    assert 'role="description">cloudmask<' in meta
    for i, name in enumerate(sentinel2.INTERPRETATION_CLOUDSEN12):
        assert f'<Item name="class_{i}">{name}</Item>' in meta
