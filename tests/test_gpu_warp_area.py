"""Footprint resampling of the warp on the GPU (sc_warp_area through the C ABI, warp.reproject with average / max / min / mode,
warp.source_boxes, products.regrid, aviris_scene_predict(resolution=)) against the numpy float64 restatement of
tests/warp_area_util.py.  Gates: boxes within 1e-6 source pixels (the coordinate gate of the warp); outside the tie set -- asserted on
the restatement alone to hold at most 0.1 % of a case's pixels -- the data pixels are the restatement's, ``average`` lies within
2 * 2^-24 * max|x| of float32(restatement) (one float32 rounding, doubled for a flip of the fp64 quotient), the coverage plane within
2 * 2^-24, and max / min / mode are bit-equal.  Every case runs once per forced mapping of the kernel."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import plume_scene_util as PS  # noqa: E402
import warp_area_util as A  # noqa: E402
from hip_ops import DEV  # noqa: E402
from starcop_amd import _lib, io_formats as io, pipeline, products, warp  # noqa: E402
from warp_util import mismatching_bytes  # noqa: E402

COORD_GATE_PX = 1e-6
VARIANTS = ("thread", "lanes")
COVERAGES = (0.0, 0.5, 1.0)
NOD = -9999.0
GRIDS = dict(A.GRIDS)
# boxes of 40 x 40 source pixels off the lattice: the lanes of a group go round their column loop three times
GRIDS["down40"] = ((3, 5), (600123.37, 200.0, 0.0, 3590456.71, 0.0, -200.0), 32613) + A.GRIDS["down12_aligned"][3:]
CASES = ("down12_aligned", "down_geo", "rotated17", "near_one", "up3", "half_outside", "all_outside", "down40")


@functools.lru_cache(maxsize=None)
def footprints(name):
    ds, dgt, dcrs, ss, sgt, scrs = GRIDS[name]
    return A.Footprints(A.boxes_ref(ds, dgt, dcrs, sgt, scrs), ss)


@functools.lru_cache(maxsize=None)
def float_plane(name, kind="holes", seed=11):
    a = A.seeded_plane(GRIDS[name][3], seed, kind)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def mask_plane(name, classes):
    a = A.class_map(GRIDS[name][3], classes)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(name, what, nodata, mode, mc):
    plane = float_plane(name, *what[1:]) if what[0] == "float" else mask_plane(name, what[1])
    val, cov, valid, tie = A.reduce_ref(plane, nodata, footprints(name), mode, mc)
    # at most 0.1 % of a case's pixels may be left out; asserted before the device is touched (these grids and seeds leave out none
    # at min_coverage 0 and 0.5).  At min_coverage 1 every entirely covered pixel has a coverage within rounding of the threshold --
    # that is what the threshold means there -- so those are left out without counting against the bound, and the comparison still
    # establishes that every pixel with a hole or a part outside the raster is no-data
    bound = footprints(name).geom_tie if mc == 1.0 else tie
    assert bound.mean() <= 1e-3, (name, what, mode, mc, int(bound.sum()))
    for a in (val, cov, valid, tie):
        a.setflags(write=False)
    return val, cov, valid, ~tie


def dev(a):
    """host array (the cached ones are read-only) -> device tensor"""
    return torch.from_numpy(np.array(a)).to(DEV)


def run(name, data, mode, **kw):
    ds, dgt, dcrs, ss, sgt, scrs = GRIDS[name]
    return warp.reproject(data, sgt, scrs, dgt, dcrs, ds, resampling=mode, **kw)


def is_data(got, nodata):
    got = np.asarray(got)
    if got.dtype == np.float32:
        return got.view(np.uint32) != np.array(nodata, dtype=np.float32).view(np.uint32)
    return got != nodata


# ------------------------------------------------------------------------------------------------ boxes
@pytest.mark.parametrize("name", CASES + ("one_pixel",))
def test_source_boxes(hip, name):
    ds, dgt, dcrs, ss, sgt, scrs = GRIDS[name]
    want = footprints(name).boxes
    both = []
    for variant in VARIANTS:
        got = warp.source_boxes(ds, dgt, dcrs, sgt, scrs, variant=variant)
        assert got.dtype == torch.float64 and tuple(got.shape) == (4,) + ds and got.is_cuda
        got = got.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(want).any()
        err = float(np.abs(got - want).max())
        size = (want[1] - want[0]).mean(), (want[3] - want[2]).mean()
        print(f"{name} {variant}: mean box {size[0]:.2f} x {size[1]:.2f} px, max |box - restatement| = {err:.3g} px")
        assert err <= COORD_GATE_PX
        both.append(got)
    assert mismatching_bytes(both[0], both[1]) == 0
    assert mismatching_bytes(warp.source_boxes(ds, dgt, dcrs, sgt, scrs).cpu().numpy(), both[0]) == 0


def test_boxes_outside_the_zone(hip):
    """more than 30 degrees from the central meridian a corner has no coordinates: the box is NaN and the pixel no-data"""
    dgt = (-140.0 + 0.123, 1.0, 0.0, 40.0, 0.0, -1.0)                     # 1 degree pixels from 140 W to 70 W; zone 13 is centred on 105 W
    sgt = (500000.0 - 3.0e6, 1000.0, 0.0, 5000000.0, 0.0, -1000.0)
    want = A.boxes_ref((2, 70), dgt, 4326, sgt, 32613)
    assert 0.1 < np.isnan(want[0]).mean() < 0.25
    src = torch.ones((1200, 6000), dtype=torch.float32, device=DEV)
    for variant in VARIANTS:
        got = warp.source_boxes((2, 70), dgt, 4326, sgt, 32613, variant=variant).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and float(np.nanmax(np.abs(got - want))) <= COORD_GATE_PX
        out = warp.reproject(src, sgt, 32613, dgt, 4326, (2, 70), "average", NOD, min_coverage=0.0, variant=variant).cpu().numpy()
        assert (out[np.isnan(want[0])] == np.float32(NOD)).all() and (out == 1.0).any()


# ------------------------------------------------------------------------------------------------ average
@pytest.mark.parametrize("name", CASES)
def test_average(hip, name):
    plane = float_plane(name)
    src = dev(plane)
    finite = plane[np.isfinite(plane) & (plane != NOD)]
    gate = 2 * 2.0 ** -24 * float(np.abs(finite).max())
    for mc in COVERAGES:
        want, wcov, valid, keep = _ref(name, ("float", "holes"), NOD, "average", mc)
        for variant in VARIANTS:
            got, cov = run(name, src, "average", nodata=NOD, min_coverage=mc, return_coverage=True, variant=variant)
            assert got.is_contiguous() and got.dtype == torch.float32 and cov.dtype == torch.float32 and got.shape == cov.shape
            got, cov = got.cpu().numpy(), cov.cpu().numpy()
            assert not np.isnan(got).any()
            assert np.array_equal(is_data(got, NOD)[keep], valid[keep]), f"footprint {name} {variant} min_coverage {mc}"
            m = keep & valid
            err = float(np.abs(got[m].astype(np.float64) - want[m].astype(np.float32).astype(np.float64)).max()) if m.any() else 0.0
            cerr = float(np.abs(cov[m].astype(np.float64) - wcov[m]).max()) if m.any() else 0.0
            print(f"{name} {variant} min_coverage {mc}: {valid.mean():.1%} data, {int((~keep).sum())} left out, max |got - float32(restatement)| = "
                  f"{err:.3g} (gate {gate:.3g}), coverage {cerr:.3g} (gate {2 * 2.0 ** -24:.3g})")
            assert err <= gate and cerr <= 2 * 2.0 ** -24
            assert (cov[keep & ~valid] == 0).all()                          # the coverage plane is 0 where the pixel is no-data
            assert np.array_equal(run(name, src, "average", nodata=NOD, min_coverage=mc, variant=variant).cpu().numpy().view(np.uint32),
                                  got.view(np.uint32))                        # with and without the coverage output
    assert _ref(name, ("float", "holes"), NOD, "average", 0.0)[2].any() == (name != "all_outside")
    if name == "half_outside":
        assert 0.2 < _ref(name, ("float", "holes"), NOD, "average", 0.0)[2].mean() < 0.8
    if name == "down_geo":                                                  # holes and the raster's edge leave pixels below half coverage
        assert _ref(name, ("float", "holes"), NOD, "average", 0.0)[2].sum() > _ref(name, ("float", "holes"), NOD, "average", 0.5)[2].sum()


@pytest.mark.parametrize("name", ["down12_aligned", "down_geo", "near_one", "up3", "half_outside"])
def test_average_of_a_constant_is_the_constant(hip, name):
    src = dev(float_plane(name, "constant"))
    _, _, valid, keep = _ref(name, ("float", "constant"), NOD, "average", 0.5)
    for variant in VARIANTS:
        got = run(name, src, "average", nodata=NOD, variant=variant).cpu().numpy()
        data = is_data(got, NOD)
        assert np.array_equal(data[keep], valid[keep]) and data.any()
        assert (got[data] == np.float32(1234.5678)).all()                    # exactly, wherever valid: keep or no keep


# ------------------------------------------------------------------------------------------------ max, min, mode
@pytest.mark.parametrize("mode", ["max", "min"])
@pytest.mark.parametrize("name", CASES)
def test_extremes_float32_bit_equal(hip, name, mode):
    src = dev(float_plane(name))
    for mc in COVERAGES:
        want, _, valid, keep = _ref(name, ("float", "holes"), NOD, mode, mc)
        want = np.where(valid, want, np.float32(NOD))
        outs = [run(name, src, mode, nodata=NOD, min_coverage=mc, variant=v).cpu().numpy() for v in VARIANTS]
        for got in outs:
            assert np.array_equal(is_data(got, NOD)[keep], valid[keep]), f"footprint {name} {mode} min_coverage {mc}"
            assert mismatching_bytes(got[keep], want[keep]) == 0
        # the two mappings agree everywhere, ties included -- but for min_coverage 1, where an entirely covered pixel is data or not by
        # the last place of a sum that the mappings take in different orders
        same = keep if mc == 1.0 else np.ones_like(keep)
        assert mismatching_bytes(outs[0][same], outs[1][same]) == 0


@pytest.mark.parametrize("classes", [4, 256])
@pytest.mark.parametrize("mode", ["max", "min", "mode"])
@pytest.mark.parametrize("name", CASES)
def test_uint8_bit_equal(hip, name, mode, classes):
    plane = mask_plane(name, classes)
    assert len(np.unique(plane)) == classes
    src = dev(plane)
    for nod, coverages in ((0, COVERAGES), (255, (0.5,))):
        for mc in coverages:
            want, _, valid, keep = _ref(name, ("mask", classes), nod, mode, mc)
            want = np.where(valid, want, np.uint8(nod))
            outs = [run(name, src, mode, nodata=nod, min_coverage=mc, variant=v).cpu().numpy() for v in VARIANTS]
            for got in outs:
                assert got.dtype == np.uint8
                if nod == 255 and classes == 4:
                    assert np.array_equal((got != nod)[keep], valid[keep])   # 255 is no class here: no-data means outside
                assert mismatching_bytes(got[keep], want[keep]) == 0, f"{name} {mode} {classes} classes, no-data {nod}, min_coverage {mc}"
            same = keep if mc == 1.0 else np.ones_like(keep)                  # as for float32
            assert mismatching_bytes(outs[0][same], outs[1][same]) == 0


def test_mode_ties_go_to_the_smallest_value(hip):
    t = np.zeros((24, 24), dtype=np.uint8)
    t[:, 0::2], t[:, 1::2] = 9, 3                                           # every 12 x 12 block: 72 against 72
    t[12:, 12:] = 200
    t[12:18, 12:] = 7
    gt = (0.0, 1.0, 0.0, 0.0, 0.0, -1.0)
    for variant in VARIANTS:
        got = warp.reproject(dev(t), gt, None, (0.0, 12.0, 0.0, 0.0, 0.0, -12.0), None, (2, 2), "mode", 255, variant=variant)
        assert got.cpu().tolist() == [[3, 3], [3, 7]]


def test_auto_variant(hip):
    """the library picks the lane-group mapping for boxes of 12 columns and the thread mapping below one column"""
    for name, want in (("down12_aligned", "lanes"), ("up3", "thread"), ("down40", "lanes"), ("near_one", "thread")):
        ds, dgt, dcrs, ss, sgt, scrs = GRIDS[name]
        assert warp.area_variant(ds, dgt, dcrs, sgt, scrs) == want
        src = dev(float_plane(name))
        auto, forced = run(name, src, "average", nodata=NOD), run(name, src, "average", nodata=NOD, variant=want)
        assert mismatching_bytes(auto.cpu().numpy(), forced.cpu().numpy()) == 0


# ------------------------------------------------------------------------------------------------ planes, layouts
@pytest.mark.parametrize("P", [1, 5, 32, 33])
def test_plane_counts(hip, P):
    name = "half_outside"
    planes = np.stack([float_plane(name, "holes", 100 + p) for p in range(P)])
    nod = [(NOD, float("nan"), 0.0)[p % 3] for p in range(P)]
    src = dev(planes)
    fp = footprints(name)
    for variant in VARIANTS:
        got, cov = run(name, [src[p] for p in range(P)], "average", nodata=nod, return_coverage=True, variant=variant)
        assert tuple(got.shape) == (P,) + GRIDS[name][0]
        got, cov = got.cpu().numpy(), cov.cpu().numpy()
        for p in sorted({0, P // 2, P - 1}):
            want, wcov, valid, tie = A.reduce_ref(planes[p], nod[p], fp, "average")
            assert not tie.any()
            data = ~np.isnan(got[p]) if np.isnan(nod[p]) else is_data(got[p], nod[p])
            assert np.array_equal(data, valid), (P, p, variant)
            gate = 2 * 2.0 ** -24 * float(np.abs(planes[p][A.counting(planes[p], nod[p])]).max())
            assert float(np.abs(got[p][valid].astype(np.float64) - want[valid].astype(np.float32)).max()) <= gate
            assert float(np.abs(cov[p][valid] - wcov[valid]).max()) <= 2 * 2.0 ** -24


@pytest.mark.parametrize("dt", ["float32", "uint8"])
def test_interleaved_cube_in_place(hip, dt):
    name = "down_geo"
    if dt == "float32":
        planes, mode, nod = np.stack([float_plane(name, "holes", 30 + p) for p in range(5)]), "max", NOD
    else:
        planes, mode, nod = np.stack([A.class_map(GRIDS[name][3], 4, seed=30 + p) for p in range(5)]), "mode", 0
    cube = dev(np.ascontiguousarray(planes.transpose(1, 2, 0)))         # (Hs, Ws, 5), pixel-interleaved
    view = cube.permute(2, 0, 1)
    assert not view.is_contiguous() and view.stride(2) == 5
    dense = dev(planes)
    fp = footprints(name)
    for variant in VARIANTS:
        got = run(name, view, mode, nodata=nod, variant=variant).cpu().numpy()
        assert mismatching_bytes(got, run(name, dense, mode, nodata=nod, variant=variant).cpu().numpy()) == 0
        for p in (0, 4):
            want, _, valid, tie = A.reduce_ref(planes[p], nod, fp, mode)
            assert not tie.any() and mismatching_bytes(got[p], np.where(valid, want, np.array(nod, dtype=planes.dtype))) == 0
        part = run(name, view[1:4], mode, nodata=nod, variant=variant).cpu().numpy()     # a slice of the planes
        assert mismatching_bytes(part, got[1:4]) == 0


def call_abi(hip, name, stack, dst, mode, P=None, elem=None, cov=None, boxes=None, **over):
    """one raw sc_warp_area call on a stacked (P, Hs, Ws) device tensor; returns the status code"""
    ds, dgt, dcrs, ss, sgt, scrs = GRIDS[name]
    a = _lib.sc_warp_area_args()
    inv = warp.invert_geotransform(sgt)
    for i in range(6):
        a.dst_gt[i], a.src_inv[i] = dgt[i], inv[i]
    a.dst_crs, a.src_crs = dcrs, scrs
    a.out_h, a.out_w = ds
    a.src_h, a.src_w = ss
    a.P = stack.shape[0] if P is None else P
    a.elem_bytes = stack.element_size() if elem is None else elem
    a.mode, a.variant, a.min_coverage = mode, 0, 0.5
    for p in range(min(max(a.P, 0), _lib.WARP_MAX_PLANES)):
        q = min(p, stack.shape[0] - 1)
        a.src[p] = stack[q].data_ptr()
        a.row_stride[p], a.col_stride[p] = stack.stride(1), stack.stride(2)
        a.nodata_bits[p] = 0
    a.out = dst.data_ptr() if dst is not None else None
    a.coverage, a.boxes = (t.data_ptr() if isinstance(t, torch.Tensor) else t for t in (cov, boxes))      # a tensor, an address or None
    for k, v in over.items():                                              # any field of the struct, by name
        setattr(a, k, v)
    rc = hip.sc_warp_area(a, _lib.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dt, mode", [("float32", _lib.WARP_AREA_AVERAGE), ("float32", _lib.WARP_AREA_MIN), ("uint8", _lib.WARP_AREA_MODE)])
def test_misaligned_output_takes_the_one_pixel_path(hip, dt, mode):
    """up3 has a width of 72 (16-byte stores); written into views aligned to their elements only the bytes are the same"""
    name = "up3"
    planes = np.stack([float_plane(name, "holes", s) for s in (1, 2)]) if dt == "float32" else np.stack([mask_plane(name, 4), mask_plane(name, 256)])
    src = dev(planes)
    H, W = GRIDS[name][0]
    for variant in (_lib.WARP_AREA_THREAD, _lib.WARP_AREA_LANES):
        aligned, acov = torch.zeros((2, H, W), dtype=src.dtype, device=DEV), torch.zeros((2, H, W), dtype=torch.float32, device=DEV)
        assert aligned.data_ptr() % 16 == 0 and acov.data_ptr() % 16 == 0
        assert call_abi(hip, name, src, aligned, mode, cov=acov, variant=variant) == 0
        out = torch.zeros(2 * H * W + 1, dtype=src.dtype, device=DEV)[1:].view(2, H, W)
        cov = torch.zeros(2 * H * W + 1, dtype=torch.float32, device=DEV)[1:].view(2, H, W)
        assert out.data_ptr() % (4 * src.element_size()) != 0 and cov.data_ptr() % 16 != 0
        assert call_abi(hip, name, src, out, mode, cov=cov, variant=variant) == 0
        assert mismatching_bytes(out.cpu().numpy(), aligned.cpu().numpy()) == 0 and mismatching_bytes(cov.cpu().numpy(), acov.cpu().numpy()) == 0
        assert call_abi(hip, name, src, aligned.clone(), mode, cov=cov, variant=variant) == 0      # aligned values, misaligned coverage
        assert mismatching_bytes(cov.cpu().numpy(), acov.cpu().numpy()) == 0
        assert float(acov.max()) > 0.5 and bool((aligned != 0).any())


def test_one_pixel(hip):
    ds, dgt, dcrs, ss, sgt, scrs = GRIDS["one_pixel"]
    plane = np.array([[1.0, 2.0], [4.0, NOD]], dtype=np.float32)
    fp = footprints("one_pixel")
    for mode in ("average", "max", "min"):
        want, wcov, valid, tie = A.reduce_ref(plane, NOD, fp, mode, 0.0)
        assert valid.all() and not tie.any()
        for variant in VARIANTS:
            got, cov = warp.reproject(plane, sgt, scrs, dgt, dcrs, ds, mode, NOD, min_coverage=0.0, return_coverage=True, variant=variant)
            assert isinstance(got, np.ndarray) and got.shape == (1, 1) and cov.shape == (1, 1)        # numpy in, numpy out
            assert abs(float(got[0, 0]) - float(want[0, 0])) <= 2 * 2.0 ** -24 * 4.0 and abs(float(cov[0, 0]) - wcov[0, 0]) <= 2 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ conservation, determinism
def test_average_times_coverage_conserves_the_integral(hip):
    """independent of the restatement: on the shared 12x lattice, sum_dst average * coverage * 3600 m2 == sum_src x * 25 m2 over the
    counting source pixels, within 2^-23 * sum_dst |average| * coverage * 3600 (one float32 rounding of each average, one of each
    coverage)"""
    name = "down12_aligned"
    plane = np.abs(float_plane(name))                                        # non-negative, with NaN and no-data holes (|-9999| = 9999)
    plane = np.where(float_plane(name) == np.float32(NOD), np.float32(NOD), plane).astype(np.float32)
    Hd, Wd = GRIDS[name][0]
    inside = plane[:12 * Hd, :12 * Wd].astype(np.float64)
    want = float(inside[A.counting(plane[:12 * Hd, :12 * Wd], NOD)].sum()) * 25.0
    for variant in VARIANTS:
        avg, cov = run(name, dev(plane), "average", nodata=NOD, min_coverage=0.0, return_coverage=True, variant=variant)
        avg, cov = avg.cpu().numpy().astype(np.float64), cov.cpu().numpy().astype(np.float64)
        assert (cov[avg != NOD] > 0).all() and (cov[avg == NOD] == 0).all() and (cov < 1).any() and (avg != NOD).mean() > 0.9
        got, gate = float((avg * cov).sum()) * 3600.0, 2.0 ** -23 * float((np.abs(avg) * cov).sum()) * 3600.0
        print(f"{variant}: integral {got:.6f} against {want:.6f}, difference {abs(got - want):.3g} (gate {gate:.3g})")
        assert abs(got - want) <= gate


@pytest.mark.parametrize("mode", ["average", "max", "min", "mode"])
def test_two_calls_give_identical_bytes(hip, mode):
    name = "down_geo"
    if mode == "mode":
        planes, nod = np.stack([A.class_map(GRIDS[name][3], c, seed=s) for c, s in ((4, 1), (256, 2), (4, 3))]), 0
    else:
        planes, nod = np.stack([float_plane(name, "holes", s) for s in (1, 2, 3)]), NOD
    src = dev(planes)
    for variant in VARIANTS:
        a = run(name, src, mode, nodata=nod, return_coverage=True, variant=variant)
        b = run(name, src, mode, nodata=nod, return_coverage=True, variant=variant)
        assert mismatching_bytes(a[0].cpu().numpy(), b[0].cpu().numpy()) == 0 and mismatching_bytes(a[1].cpu().numpy(), b[1].cpu().numpy()) == 0


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_errors(hip):
    name = "down_geo"
    Hs, Ws = GRIDS[name][3]
    H, W = GRIDS[name][0]
    AVG, MAX, MIN, MODE = _lib.WARP_AREA_AVERAGE, _lib.WARP_AREA_MAX, _lib.WARP_AREA_MIN, _lib.WARP_AREA_MODE
    s = torch.zeros((2, Hs, Ws), dtype=torch.float32, device=DEV)
    m = torch.zeros((2, Hs, Ws), dtype=torch.uint8, device=DEV)
    out = torch.empty((_lib.WARP_MAX_PLANES, H, W), dtype=torch.float32, device=DEV)
    cov = torch.empty((_lib.WARP_MAX_PLANES, H, W), dtype=torch.float32, device=DEV)
    boxes = torch.empty((4, H, W), dtype=torch.float64, device=DEV)

    def good():
        assert call_abi(hip, name, s, out, AVG) == 0
        assert call_abi(hip, name, s, out, AVG, P=_lib.WARP_MAX_PLANES, cov=cov, boxes=boxes) == 0
        assert call_abi(hip, name, s, None, AVG, P=0, boxes=boxes) == 0
        for mode in (MAX, MIN, MODE):
            assert call_abi(hip, name, m, out, mode) == 0
        for mode in (MAX, MIN):
            assert call_abi(hip, name, s, out, mode, min_coverage=1.0, variant=2) == 0
    good()
    bad = ({"P": -1}, {"P": _lib.WARP_MAX_PLANES + 1}, {"P": 0},                              # P = 0 without boxes: nothing to write
           {"P": 0, "boxes": boxes, "cov": cov},                                         # a coverage without planes
           {"elem": 3}, {"elem": 0}, {"elem": 2}, {"elem": 8}, {"mode": 0}, {"mode": 1}, {"mode": 6}, {"mode": -1},
           {"mode": AVG, "elem": 1}, {"mode": MODE, "elem": 4},
           {"min_coverage": -0.01}, {"min_coverage": 1.01}, {"min_coverage": float("nan")}, {"variant": 3}, {"variant": -1},
           {"dst_crs": 3857}, {"src_crs": 32661}, {"src_crs": 32700}, {"dst_crs": 0}, {"src_crs": 0}, {"dst_crs": -5, "src_crs": -5},
           {"out_h": 0}, {"out_w": -3}, {"src_h": 0}, {"src_w": -1}, {"out_h": 65536, "out_w": 32768},
           {"out": None}, {"out": out.data_ptr() + 2}, {"coverage": cov.data_ptr() + 2}, {"boxes": boxes.data_ptr() + 4})
    for kw in bad:
        rc = call_abi(hip, name, s, out, kw.pop("mode", AVG), **kw)
        assert rc == -1, kw
        with pytest.raises(ValueError, match="sc_warp_area:"):
            _lib.check(rc)
    assert hip.sc_warp_area(None, _lib.stream()) == -1
    assert hip.sc_warp_area(_lib.sc_warp_area_args(), _lib.stream()) == -1         # everything zero
    assert hip.sc_warp_area_variant(_lib.sc_warp_area_args()) == -1
    for over in ({"src": (_lib.C.c_void_p * 32)()}, {"row_stride": (_lib.C.c_int64 * 32)(*([-Ws] * 32))},
                 {"col_stride": (_lib.C.c_int64 * 32)(*([-1] * 32))}, {"src": (_lib.C.c_void_p * 32)(*([s.data_ptr() + 2] * 32))},
                 {"dst_gt": (_lib.C.c_double * 6)(0.0, float("nan"), 0.0, 0.0, 0.0, -1.0)},
                 {"dst_gt": (_lib.C.c_double * 6)(0.0, float("inf"), 0.0, 0.0, 0.0, -1.0)},
                 {"src_inv": (_lib.C.c_double * 6)(0.0, 0.0, 0.0, 0.0, 1.0, 1.0)}, {"dst_gt": (_lib.C.c_double * 6)(0.0, 1.0, 2.0, 0.0, 2.0, 4.0)}):
        assert call_abi(hip, name, s, out, AVG, **over) == -1, list(over)      # null / misaligned source, negative strides, geotransforms
    good()


# ------------------------------------------------------------------------------------------------ the layers above
def test_reproject_like_passes_the_footprint_arguments(hip, tmp_path):
    name = "down_geo"
    ds, dgt, dcrs, ss, sgt, scrs = GRIDS[name]
    path = str(tmp_path / "like.tif")
    io.write_tiff(path, np.zeros(ds, dtype=np.uint8), extra_tags=warp.geo_tags(dgt, dcrs))
    src = dev(float_plane(name))
    got, cov = warp.reproject_like(src, sgt, scrs, path, "average", NOD, min_coverage=0.0, return_coverage=True)
    want, wcov = run(name, src, "average", nodata=NOD, min_coverage=0.0, return_coverage=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(cov, wcov)
    assert not torch.equal(got.view(torch.int32), run(name, src, "average", nodata=NOD).view(torch.int32))      # min_coverage arrived


def test_regrid_equals_per_key_reproject(hip):
    ss, sgt, scrs = GRIDS["down_geo"][3:]
    rng = np.random.default_rng(3)
    pred = dev(rng.random(ss).astype(np.float32))
    mf = dev(float_plane("down_geo"))
    rgb = dev(rng.random((3,) + ss).astype(np.float32))
    binary = (pred > 0.7).to(torch.uint8)
    out = {"prediction": pred, "mf": mf, "rgb": rgb, "pred_binary": binary}
    gt, crs, area = products.regrid(dict_copy := dict(out), sgt, scrs, 32613, 60.0, resampling={"prediction": "average", "mf": "average"},
                                    nodata={"prediction": NOD, "mf": NOD}, mask_resampling="max", min_coverage=0.25)
    shape, want_gt = warp.suggest_grid(ss, sgt, scrs, 32613, 60.0)
    assert gt == want_gt and crs == 32613 and area == 3600.0
    for key, mode, nod in (("prediction", "average", NOD), ("mf", "average", NOD), ("rgb", "nearest", 0), ("pred_binary", "max", 0)):
        want = warp.reproject(out[key], sgt, scrs, gt, 32613, shape, mode, nod, min_coverage=0.25)
        assert dict_copy[key].dtype == want.dtype and torch.equal(dict_copy[key].view(torch.uint8), want.contiguous().view(torch.uint8)), key
    assert int(dict_copy["pred_binary"].sum()) > 0 and tuple(dict_copy["rgb"].shape) == (3,) + shape
    # a plume pixel survives `max` wherever nearest may lose it
    near = warp.reproject(binary, sgt, scrs, gt, 32613, shape)
    assert int(dict_copy["pred_binary"].sum()) > int(near.sum())


def read_all(folder):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder))}


def test_aviris_scene_predict_at_a_resolution(hip, tmp_path):
    """a 70 x 100 flight line of 5 m pixels, file to file onto the north-up 20 m grid"""
    from test_gpu_plume_scene import _model
    H, W, RES = 70, 100, 20.0
    model = _model(bias=-0.93)
    wl = np.array([440.0, 461.0, 500.0, 549.0, 600.0, 641.0, 700.0])
    rng = np.random.default_rng(61)
    cube = rng.uniform(0.5, 12.0, size=(H, W, wl.size)).astype(np.float32)
    mf = (600.0 * rng.standard_normal((H, W)) + 200.0).astype(np.float32)
    mf[:6, :9] = PS.FILL
    kw = dict(toa_correction_factor=1.037, tile=32, halo=32, plumes=True)
    for tag, map_info in (("plain", PS.MAP_INFO), ("rotated", PS.MAP_INFO[:-1] + ", rotation=-12.0}")):
        folder = PS.write_flight_line(str(tmp_path / tag / "ang20190101t180000_rdn"), cube, wl, map_info=map_info)
        io.write_tiff(os.path.join(folder, "mag1c.tif"), mf, blocksize=128, extra_tags={42113: (2, ("-9999",))})
        # resolution=None with the default modes is the call without the new arguments, byte for byte
        old = pipeline.aviris_scene_predict(model, folder, str(tmp_path / tag / "old"), north_up=True, **kw)
        same = pipeline.aviris_scene_predict(model, folder, str(tmp_path / tag / "same"), north_up=True, resolution=None, resampling="nearest",
                                             mask_resampling="nearest", **kw)
        assert read_all(str(tmp_path / tag / "old")) == read_all(str(tmp_path / tag / "same"))
        line = pipeline.aviris_scene_predict(model, folder, **kw)            # the products on the line's own grid
        assert ("geotransform" in old) == (tag == "rotated")
        if tag == "rotated":
            header = io.read_envi_header(os.path.join(folder, os.path.basename(folder) + "_img.hdr"))
            src_gt, epsg, _ = io.envi_geotransform(header)
            shape5, gt5 = warp.suggest_grid((H, W), src_gt, epsg, epsg, 5.0)
            for key, nod in (("prediction", PS.FILL), ("pred_binary", 0), ("mf", PS.FILL)):
                want = warp.reproject(line[key], src_gt, epsg, gt5, epsg, shape5, nodata=nod)
                assert torch.equal(old[key].view(torch.uint8), want.contiguous().view(torch.uint8)), key
        out = pipeline.aviris_scene_predict(model, folder, str(tmp_path / tag / "coarse"), north_up=True, resolution=RES,
                                            resampling={"prediction": "average", "mf": "average"}, mask_resampling="max", **kw)
        header = io.read_envi_header(os.path.join(folder, os.path.basename(folder) + "_img.hdr"))
        src_gt, epsg, _ = io.envi_geotransform(header)
        shape, gt = warp.suggest_grid((H, W), src_gt, epsg, epsg, RES)
        assert tuple(out["geotransform"]) == gt and out["crs"] == epsg and gt[1] == RES and gt[5] == -RES and gt[2] == gt[4] == 0.0
        for key, mode, nod in (("prediction", "average", PS.FILL), ("pred_binary", "max", 0), ("mf", "average", PS.FILL)):
            want = warp.reproject(line[key], src_gt, epsg, gt, epsg, shape, mode, nod)
            assert torch.equal(out[key].view(torch.uint8), want.contiguous().view(torch.uint8)), (tag, key)
        for fname in ("pred.tif", "predbinary.tif"):
            info = io.tiff_info(str(tmp_path / tag / "coarse" / fname))
            assert io.geo_from_tags(info) == (gt, epsg) and (info.height, info.width) == shape and info.tags[33550][1][:2] == (RES, RES)
        table = out["plumes"]
        assert len(table) >= 1 and int(table["area_px"].sum()) == int(out["pred_binary"].sum())
        assert np.array_equal(table["ime_ppmm_m2"].to_numpy(), table["mag1c_sum"].to_numpy() * RES * RES)      # the new pixel area
        assert "ime_ppmm_m2" in open(str(tmp_path / tag / "coarse" / "plumes.csv")).readline()
    with pytest.raises(ValueError, match="north_up"):
        pipeline.aviris_scene_predict(model, folder, resolution=RES, **kw)
