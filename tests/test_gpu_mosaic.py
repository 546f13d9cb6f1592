"""The mosaic on the GPU (sc_mosaic through the C ABI, starcop_amd.mosaic, products.mosaic, pipeline.mosaic_products) against the
numpy restatement of tests/mosaic_util.py: winners, index and count exact, nearest planes bit-equal outside the pixels whose
restated (u, v) lies within 1e-6 px of a cell boundary of any source (none in this scene), bilinear and mean within one float32
rounding doubled (2 * 2^-24 * max|x|) of the float64 restatement rounded once."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mosaic_util as MU  # noqa: E402
import warp_util as U  # noqa: E402
from hip_ops import DEV  # noqa: E402
from starcop_amd import _lib, warp  # noqa: E402
from starcop_amd import mosaic as M  # noqa: E402

RULES = ("first", "last", "max", "min")


def device_sources(planes, which=None):
    which = range(MU.N) if which is None else which
    return [(torch.from_numpy(planes[s]).to(DEV), MU.SOURCES[s][2], MU.SOURCES[s][3]) for s in which]


def run(shape, planes, rule, which=None, **kw):
    return M.mosaic(device_sources(planes, which), MU.DST_GT, MU.DST_CRS, shape, rule, **kw)


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}")


def is_nodata(a, nodata):
    return bits_of(a) == bits_of(np.array(nodata, dtype=a.dtype))


def check_float(got, ref, keep, gate, what):
    """got float32 (P, H, W) against the float64 restatement rounded once: the same no-data pixels, finite values within the gate,
    infinities equal"""
    assert got.dtype == np.float32 and not np.isnan(got).any(), what
    nod = is_nodata(got, MU.NODATA)
    assert np.array_equal(nod[:, keep], ref["nodata"][:, keep]), f"{what}: no-data pixels"
    m = keep[None] & ~ref["nodata"]
    want = ref["out"][m].astype(np.float32)
    g = got[m]
    fin = np.isfinite(want)
    assert np.array_equal(g[~fin], want[~fin]), f"{what}: infinities"
    err = float(np.abs(g[fin].astype(np.float64) - want[fin].astype(np.float64)).max()) if fin.any() else 0.0
    print(f"{what}: {m.mean():.1%} valid, max |got - float32(restatement)| = {err:.3g} (gate {gate:.3g})")
    assert m.any() and err <= gate, what


# ------------------------------------------------------------------------------------------------ winner rules
@pytest.mark.parametrize("shape", MU.SHAPES)
@pytest.mark.parametrize("resampling", ["nearest", "bilinear"])
@pytest.mark.parametrize("rule", RULES)
def test_winner_rules(hip, rule, resampling, shape):
    planes = MU.float_planes(3)
    out, index, count = run(shape, planes, rule, resampling=resampling, nodata=MU.NODATA, return_index=True, return_count=True)
    assert out.is_contiguous() and tuple(out.shape) == (3,) + shape and index.dtype == torch.int32 and count.dtype == torch.int32
    out, index, count = out.cpu().numpy(), index.cpu().numpy(), count.cpu().numpy()
    ref = MU.mosaic_ref(planes, shape, rule, 0, resampling)
    keep = MU.compared(shape)
    assert np.array_equal(index[keep], ref["index"][keep]) and np.array_equal(count[keep], ref["count"][keep])
    assert len(np.unique(ref["index"])) == 6 and ref["count"].max() == 4          # no winner and every source but `far`; up to 4 valid
    if resampling == "nearest":
        bad = U.mismatching_bytes(out[:, keep], ref["out"][:, keep])
        print(f"{rule} {shape}: mismatching bytes {bad}")
        assert bad == 0
    else:
        check_float(out, ref, keep, MU.gate(planes), f"{rule} bilinear {shape}")
        near = run(shape, planes, rule, resampling="nearest", nodata=MU.NODATA).cpu().numpy()
        near_valid = ~is_nodata(near, MU.NODATA) & ~np.isnan(near)
        assert np.array_equal(~is_nodata(out, MU.NODATA), near_valid)                # the footprint of nearest, plane by plane


@pytest.mark.parametrize("dt", MU.NP_DTYPES)
@pytest.mark.parametrize("rule", ["first", "last"])
def test_dtypes_bit_equal(hip, rule, dt):
    shape = (45, 88)                                                              # float64: the 2-pixel vector
    planes, nod = MU.typed_planes(dt, 2, seed=5), MU.nodata_for(dt)
    out, index, count = run(shape, planes, rule, nodata=nod, return_index=True, return_count=True)
    ref = MU.mosaic_ref(planes, shape, rule, 0, nodata=nod)
    keep = MU.compared(shape)
    assert str(out.dtype).endswith(dt)
    assert np.array_equal(index.cpu().numpy()[keep], ref["index"][keep]) and np.array_equal(count.cpu().numpy()[keep], ref["count"][keep])
    assert U.mismatching_bytes(out.cpu().numpy()[:, keep], ref["out"][:, keep]) == 0
    # numpy in, numpy out; 2-D sources give a 2-D result; key = -1: the footprint alone
    one = M.mosaic([(planes[s][1], MU.SOURCES[s][2], MU.SOURCES[s][3]) for s in range(MU.N)], MU.DST_GT, MU.DST_CRS, shape, rule,
                   key=-1, nodata=nod)
    assert isinstance(one, np.ndarray) and one.shape == shape
    ref1 = MU.mosaic_ref([p[1:2] for p in planes], shape, rule, -1, nodata=nod)
    assert U.mismatching_bytes(one[keep], ref1["out"][0][keep]) == 0


# ------------------------------------------------------------------------------------------------ mean
@pytest.mark.parametrize("P", [1, 6])
@pytest.mark.parametrize("resampling", ["nearest", "bilinear"])
def test_mean(hip, resampling, P):
    """P = 6 goes through the chunking of the Python side (4 planes per launch; the key plane rides along)"""
    shape = (45, 88)
    planes = MU.float_planes(P, seed=3)
    key = 0 if P == 1 else 2
    out, count = run(shape, planes, "mean", key=key, resampling=resampling, nodata=MU.NODATA, return_count=True)
    ref = MU.mosaic_ref(planes, shape, "mean", key, resampling)
    keep = MU.compared(shape)
    assert np.array_equal(count.cpu().numpy()[keep], ref["count"][keep])
    check_float(out.cpu().numpy(), ref, keep, MU.gate(planes), f"mean {resampling} P={P}")
    free = run(shape, planes, "mean", key=-1, resampling=resampling, nodata=MU.NODATA)
    check_float(free.cpu().numpy(), MU.mosaic_ref(planes, shape, "mean", -1, resampling), keep, MU.gate(planes), f"mean {resampling} P={P} key=-1")


def test_more_planes_than_one_launch_holds(hip):
    """34 planes with the key in the last one: the launch that holds the key decides, the other follows by its index"""
    shape = (45, 88)
    planes = MU.float_planes(M.MAX_PLANES + 2, seed=11)
    key = M.MAX_PLANES + 1
    out, index, count = run(shape, planes, "min", key=key, nodata=MU.NODATA, return_index=True, return_count=True)
    ref = MU.mosaic_ref(planes, shape, "min", key)
    keep = MU.compared(shape)
    assert np.array_equal(index.cpu().numpy()[keep], ref["index"][keep]) and np.array_equal(count.cpu().numpy()[keep], ref["count"][keep])
    assert U.mismatching_bytes(out.cpu().numpy()[:, keep], ref["out"][:, keep]) == 0


# ------------------------------------------------------------------------------------------------ one source is the warp
@pytest.mark.parametrize("dt", MU.NP_DTYPES)
def test_one_source_equals_the_warp(hip, dt):
    planes, nod = MU.typed_planes(dt, 2, seed=7), MU.nodata_for(dt)
    for shape in ((45, 88), (45, 85)):
        for s in (0, 2, 3, 4):                                                    # 4326, the same zone, rotated, another zone
            _, _, sgt, scrs = MU.SOURCES[s]
            src = torch.from_numpy(planes[s]).to(DEV)
            got = M.mosaic([(src, sgt, scrs)], MU.DST_GT, MU.DST_CRS, shape, "first", key=-1, nodata=nod)
            want = warp.reproject(src, sgt, scrs, MU.DST_GT, MU.DST_CRS, shape, nodata=nod)
            assert U.mismatching_bytes(got.cpu().numpy(), want.cpu().numpy()) == 0, (dt, shape, s)
            if dt == "float32":
                got = M.mosaic([(src, sgt, scrs)], MU.DST_GT, MU.DST_CRS, shape, "first", key=-1, resampling="bilinear", nodata=nod)
                want = warp.reproject(src, sgt, scrs, MU.DST_GT, MU.DST_CRS, shape, "bilinear", nod)
                got, want = got.cpu().numpy(), want.cpu().numpy()
                valid = ~is_nodata(want, nod)
                assert np.array_equal(~is_nodata(got, nod), valid) and valid.any()
                fin = valid & np.isfinite(want)
                assert np.array_equal(got[valid & ~fin], want[valid & ~fin])
                assert float(np.abs(got[fin].astype(np.float64) - want[fin]).max()) <= MU.gate(planes)


# ------------------------------------------------------------------------------------------------ by index
def test_by_index(hip):
    shape = (45, 88)
    planes = MU.float_planes(3, seed=2)
    for resampling in ("nearest", "bilinear"):
        out, index = run(shape, planes, "max", resampling=resampling, nodata=MU.NODATA, return_index=True)
        again = run(shape, planes, "index", resampling=resampling, nodata=MU.NODATA, select=index)
        assert U.mismatching_bytes(out.cpu().numpy(), again.cpu().numpy()) == 0
    masks = MU.typed_planes("uint8", 2, seed=4)
    rng = np.random.default_rng(8)
    sel = rng.integers(-1, MU.N + 1, size=shape).astype(np.int32)                 # -1 and N: none
    sel[rng.random(shape) < 0.05] = 1000
    got = run(shape, masks, "index", nodata=7, select=torch.from_numpy(sel).to(DEV)).cpu().numpy()
    ref = MU.mosaic_ref(masks, shape, "index", -1, nodata=7, select=sel)
    keep = MU.compared(shape)
    assert U.mismatching_bytes(got[:, keep], ref["out"][:, keep]) == 0
    none = (sel < 0) | (sel >= MU.N)
    assert none.sum() > 100 and (got[:, none] == 7).all()
    assert (ref["index"] >= 0).sum() > 500                                        # validity is not consulted; the footprint applies


# ------------------------------------------------------------------------------------------------ the raw ABI
class Call:
    """one raw sc_mosaic call on per-source (P, Hs, Ws) device tensors; every field of the structs can be overridden"""

    def __init__(self, shape, srcs, which=None, boxes="computed"):
        self.which = list(range(MU.N)) if which is None else list(which)
        self.shape, self.srcs = shape, srcs
        n, P = len(self.which), srcs[0].shape[0]
        self.table = (_lib.sc_mosaic_source * max(n, 1))()
        for k, s in enumerate(self.which):
            _, ss, sgt, scrs = MU.SOURCES[s]
            q, inv = self.table[k], warp.invert_geotransform(sgt)
            for i in range(6):
                q.src_inv[i] = inv[i]
            q.src_crs, (q.src_h, q.src_w) = scrs, ss
            box = M.footprint_box(ss, sgt, scrs, MU.DST_GT, MU.DST_CRS, shape) if boxes == "computed" else (0, shape[0], 0, shape[1])
            for i in range(4):
                q.box[i] = box[i]
            for p in range(P):
                q.src[p] = srcs[k][p].data_ptr()
                q.row_stride[p], q.col_stride[p] = srcs[k].stride(1), srcs[k].stride(2)
        a = self.a = _lib.sc_mosaic_args()
        for i in range(6):
            a.dst_gt[i] = MU.DST_GT[i]
        a.dst_crs, (a.out_h, a.out_w) = MU.DST_CRS, shape
        a.N, a.P, a.elem_bytes, a.rule, a.key_plane, a.resampling = n, P, srcs[0].element_size(), 0, 0, 0
        nd = np.dtype(str(srcs[0].dtype).replace("torch.", ""))
        a.flags = _lib.MOSAIC_KEY_FLOAT if nd.kind == "f" else 0
        for p in range(P):
            a.nodata_bits[p] = int(bits_of(np.array([MU.nodata_for(nd)], dtype=nd))[0])
        a.sources = ctypes.cast(self.table, ctypes.POINTER(_lib.sc_mosaic_source))
        self.dev_table = torch.empty(ctypes.sizeof(_lib.sc_mosaic_source) * _lib.MOSAIC_MAX_SOURCES, dtype=torch.uint8, device=DEV)
        a.table = self.dev_table.data_ptr()

    def __call__(self, hip, o, ix=None, ct=None, **over):
        a = self.a
        a.out = o.data_ptr() if o is not None else None
        a.index = ix.data_ptr() if ix is not None else None
        a.count = ct.data_ptr() if ct is not None else None
        a.select = None
        saved = {k: getattr(a, k) for k in over if k != "sources"}                # (a pointer field read back is a view of the struct)
        for k, v in over.items():
            setattr(a, k, v)
        rc = hip.sc_mosaic(a, _lib.stream())
        torch.cuda.synchronize()
        for k, v in saved.items():
            setattr(a, k, v)
        a.sources = ctypes.cast(self.table, ctypes.POINTER(_lib.sc_mosaic_source))
        return rc


def float_call(shape, P=3, boxes="computed", seed=0, which=None):
    planes = MU.float_planes(P, seed)
    which = list(range(MU.N)) if which is None else which
    return Call(shape, [torch.from_numpy(planes[s]).to(DEV) for s in which], which, boxes)


@pytest.mark.parametrize("shape", MU.SHAPES)
def test_cull_changes_nothing(hip, shape):
    for rule, mode in ((_lib.MOSAIC_MAX, 0), (_lib.MOSAIC_LAST, 1), (_lib.MOSAIC_MEAN, 1)):
        res = []
        for boxes in ("computed", "whole"):
            call = float_call(shape, boxes=boxes)
            out = torch.zeros((3,) + shape, dtype=torch.float32, device=DEV)
            index = torch.zeros(shape, dtype=torch.int32, device=DEV) if rule != _lib.MOSAIC_MEAN else None
            count = torch.zeros(shape, dtype=torch.int32, device=DEV)
            assert call(hip, out, index, count, rule=rule, resampling=mode) == 0
            res.append([t.cpu().numpy() for t in (out, index, count) if t is not None])
        for x, y in zip(*res):
            assert U.mismatching_bytes(x, y) == 0, (rule, mode)


def test_tile_that_meets_no_box(hip):
    shape = (45, 152)
    planes = MU.float_planes(2)
    out, index, count = run(shape, planes, "first", nodata=[MU.NODATA, 5.0], return_index=True, return_count=True)
    out, index, count = out.cpu().numpy(), index.cpu().numpy(), count.cpu().numpy()
    assert (out[0, :, 128:] == np.float32(MU.NODATA)).all() and (out[1, :, 128:] == 5.0).all()
    assert (index[:, 128:] == -1).all() and (count[:, 128:] == 0).all() and (index[:, :128] >= 0).any()
    mean, count = run(shape, planes, "mean", nodata=[MU.NODATA, MU.NODATA], return_count=True)
    assert (mean.cpu().numpy()[:, :, 128:] == np.float32(MU.NODATA)).all() and (count.cpu().numpy()[:, 128:] == 0).all()


def test_ties_go_to_the_lower_number(hip):
    shape = (45, 88)
    planes = MU.float_planes(2, seed=6)
    same = [planes[0], planes[0].copy()]
    _, _, sgt, scrs = MU.SOURCES[0]
    srcs = [(torch.from_numpy(p).to(DEV), sgt, scrs) for p in same]
    for rule in ("max", "min"):
        out, index, count = M.mosaic(srcs, MU.DST_GT, MU.DST_CRS, shape, rule, nodata=MU.NODATA, return_index=True, return_count=True)
        index, count = index.cpu().numpy(), count.cpu().numpy()
        assert (count == 2).sum() > 1000 and not (index == 1).any() and (index[count == 2] == 0).all()
    # -0.0 and 0.0 are equal
    z = [np.zeros((1, 60, 56), dtype=np.float32), np.full((1, 60, 56), -0.0, dtype=np.float32)]
    index = M.mosaic([(torch.from_numpy(p).to(DEV), sgt, scrs) for p in z], MU.DST_GT, MU.DST_CRS, shape, "min", nodata=MU.NODATA,
                     return_index=True)[1].cpu().numpy()
    assert not (index == 1).any() and (index == 0).any()


def test_a_source_in_place(hip):
    """pixel-interleaved cubes, permuted: read in place through their strides"""
    shape = (45, 88)
    planes = MU.float_planes(5, seed=9)
    srcs = []
    for s in range(MU.N):
        cube = torch.from_numpy(np.ascontiguousarray(planes[s].transpose(1, 2, 0))).to(DEV)      # (Hs, Ws, 5)
        view = cube.permute(2, 0, 1)
        assert not view.is_contiguous() and view.stride(2) == 5
        srcs.append((view, MU.SOURCES[s][2], MU.SOURCES[s][3]))
    got = M.mosaic(srcs, MU.DST_GT, MU.DST_CRS, shape, "max", key=1, nodata=MU.NODATA).cpu().numpy()
    want = run(shape, planes, "max", key=1, nodata=MU.NODATA).cpu().numpy()
    assert U.mismatching_bytes(got, want) == 0
    keep = MU.compared(shape)
    assert U.mismatching_bytes(got[:, keep], MU.mosaic_ref(planes, shape, "max", 1)["out"][:, keep]) == 0
    part = M.mosaic([(v[1:4], g, c) for v, g, c in srcs], MU.DST_GT, MU.DST_CRS, shape, "max", key=0, nodata=MU.NODATA).cpu().numpy()
    assert U.mismatching_bytes(part, want[1:4]) == 0


@pytest.mark.parametrize("dt", ["uint8", "float32", "float64"])
def test_misaligned_output_takes_the_scalar_variant(hip, dt):
    shape = (45, 88)
    H, W = shape
    planes = MU.typed_planes(dt, 2, seed=4)
    srcs = [torch.from_numpy(p).to(DEV) for p in planes]
    call = Call(shape, srcs)
    res = []
    for off in (0, 1):
        base = torch.zeros(2 * H * W + 1, dtype=srcs[0].dtype, device=DEV)
        ibase = torch.zeros(2 * H * W + 2, dtype=torch.int32, device=DEV)
        out, index, count = base[off:off + 2 * H * W].view(2, H, W), ibase[off:off + H * W].view(H, W), ibase[H * W + 1:2 * H * W + 1].view(H, W)
        assert (out.data_ptr() % 16 != 0) == bool(off) and out.data_ptr() % srcs[0].element_size() == 0
        assert call(hip, out, index, count if off else None, rule=_lib.MOSAIC_LAST) == 0
        res.append((out.cpu().numpy(), index.cpu().numpy()))
    assert U.mismatching_bytes(res[0][0], res[1][0]) == 0 and U.mismatching_bytes(res[0][1], res[1][1]) == 0
    ref = MU.mosaic_ref(planes, shape, "last", 0, nodata=MU.nodata_for(dt))
    assert np.array_equal(res[1][1], ref["index"]) and U.mismatching_bytes(res[1][0], ref["out"]) == 0


def test_abi_refusals(hip):
    shape = (45, 88)
    call = float_call(shape)
    out = torch.empty((4,) + shape, dtype=torch.float32, device=DEV)
    index = torch.empty(shape, dtype=torch.int32, device=DEV)
    count = torch.empty(shape, dtype=torch.int32, device=DEV)
    assert call(hip, out, index, count) == 0
    assert call(hip, out, None, None, rule=_lib.MOSAIC_BY_INDEX, select=index.data_ptr()) == 0
    bad = ({"N": 0}, {"N": 65}, {"P": 0}, {"P": 33}, {"key_plane": 3}, {"key_plane": -2},
           {"rule": 6}, {"rule": -1}, {"resampling": 2}, {"flags": 2}, {"elem_bytes": 3},
           {"rule": _lib.MOSAIC_MAX, "elem_bytes": 1}, {"rule": _lib.MOSAIC_MEAN, "elem_bytes": 8}, {"rule": _lib.MOSAIC_MIN, "key_plane": -1},
           {"resampling": 1, "elem_bytes": 8}, {"flags": 1, "elem_bytes": 2},
           {"dst_crs": 3857}, {"dst_crs": 0}, {"dst_crs": -1},
           {"out_h": 0}, {"out_w": -3}, {"out_h": 65536, "out_w": 32768},
           {"out": None}, {"table": None}, {"sources": None}, {"out": out.data_ptr() + 2}, {"index": index.data_ptr() + 2},
           {"count": count.data_ptr() + 1}, {"table": call.dev_table.data_ptr() + 4},
           {"rule": _lib.MOSAIC_BY_INDEX})                                        # by index without `select`
    for kw in bad:
        if "sources" in kw:
            kw = {"sources": ctypes.POINTER(_lib.sc_mosaic_source)()}
        rc = call(hip, out, index, None if kw.get("rule") == _lib.MOSAIC_BY_INDEX else count, **kw)
        assert rc == -1, kw
        with pytest.raises(ValueError, match="sc_mosaic"):
            _lib.check(rc)
    assert call(hip, out, index, count, rule=_lib.MOSAIC_MEAN) == -1               # mean with an index
    assert call(hip, out, None, count, rule=_lib.MOSAIC_BY_INDEX, select=index.data_ptr()) == -1      # by index with a count
    assert hip.sc_mosaic(None, _lib.stream()) == -1
    five = float_call(shape, P=5)
    assert five(hip, out, None, count, rule=_lib.MOSAIC_MEAN) == -1               # mean with P = 5
    assert float_call(shape, P=4)(hip, out, None, count, rule=_lib.MOSAIC_MEAN) == 0
    q = call.table[1]
    for field, value in (("src_crs", 32661), ("src_crs", 0), ("src_h", 0), ("src_w", -1)):
        keep = getattr(q, field)
        setattr(q, field, value)
        assert call(hip, out, index, count) == -1, (field, value)
        setattr(q, field, keep)
    for arr, i, value in ((q.src, 1, None), (q.src, 0, q.src[0] + 2), (q.row_stride, 2, -56), (q.col_stride, 0, -1),
                          (q.src_inv, 1, float("nan")), (q.box, 1, shape[0] + 1), (q.box, 2, -1)):
        keep = arr[i]
        arr[i] = value
        assert call(hip, out, index, count) == -1, (i, value)
        arr[i] = keep
    keep = (q.src_inv[1], q.src_inv[2])
    q.src_inv[1] = q.src_inv[2] = 0.0
    assert call(hip, out, index, count) == -1                                     # a singular transform
    q.src_inv[1], q.src_inv[2] = keep
    _lib.check(call(hip, out, index, count))                                      # everything is back in place: the call goes through


@pytest.mark.parametrize("rule", RULES + ("mean", "index"))
def test_two_calls_give_identical_bytes(hip, rule):
    shape = (45, 88)
    planes = MU.float_planes(3, seed=1)
    kw = {"select": run(shape, planes, "max", return_index=True)[1]} if rule == "index" else {}
    if rule not in ("mean", "index"):
        kw.update(return_index=True, return_count=True)
    for resampling in ("nearest", "bilinear"):
        a = run(shape, planes, rule, resampling=resampling, nodata=MU.NODATA, **kw)
        b = run(shape, planes, rule, resampling=resampling, nodata=MU.NODATA, **kw)
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert U.mismatching_bytes(x.cpu().numpy(), y.cpu().numpy()) == 0


# ------------------------------------------------------------------------------------------------ products.mosaic, mosaic_products
def scene_dicts():
    """three prediction dicts of 64 x 80 pixels on the grids of geo_a, geo_b and utm_same; a blob of high probability is planted at
    one place of the ground that geo_a and geo_b both see (longitude -103.9106, latitude 32.4330)"""
    outs = []
    for i, s in enumerate((0, 1, 2)):
        _, _, gt, crs = MU.SOURCES[s]
        rng = np.random.default_rng(40 + i)
        prob = (rng.random((64, 80)) * 0.4).astype(np.float32)
        mf = (rng.standard_normal((64, 80)) * 300 + 200).astype(np.float32)
        if crs == 4326:
            c, r = int((-103.9106 - gt[0]) / gt[1]), int((32.4330 - gt[3]) / gt[5])
            prob[r - 3:r + 4, c - 3:c + 4] = 0.9 + 0.01 * i
        prob[:2, :] = MU.NODATA                                                   # a no-data rim
        mask = (prob > 0.5).astype(np.uint8)
        outs.append({"prediction": torch.from_numpy(prob).to(DEV), "mf": torch.from_numpy(mf).to(DEV),
                     "pred_binary": torch.from_numpy(mask).to(DEV), "geotransform": gt, "crs": crs})
    return outs


def test_products_mosaic_groups_and_counts_each_plume_once(hip, monkeypatch):
    from starcop_amd import plumes, products
    outs = scene_dicts()
    before = [{k: v.clone() for k, v in o.items() if isinstance(v, torch.Tensor)} for o in outs]
    calls = []
    real = M.mosaic

    def counting(sources, *a, **kw):
        planes = sources[0][0]
        calls.append((str(planes[0].dtype), len(planes)))
        return real(sources, *a, **kw)
    monkeypatch.setattr(M, "mosaic", counting)
    new = products.mosaic(outs, 32613, 60.0, nodata=MU.NODATA)
    monkeypatch.undo()
    assert sorted(calls) == [("torch.float32", 2), ("torch.uint8", 1)], calls       # the float keys in ONE launch, the mask by index
    for o, b in zip(outs, before):
        assert all(torch.equal(o[k], b[k]) for k in b)                            # the inputs are unchanged
    shape, gt = tuple(new["prediction"].shape), new["geotransform"]
    assert (shape, gt) == M.union_grid([((64, 80), o["geotransform"], o["crs"]) for o in outs], 32613, 60.0) and new["crs"] == 32613
    index, count = new["source_index"].cpu().numpy(), new["source_count"].cpu().numpy()
    assert index.dtype == np.int32 and set(np.unique(index)) == {-1, 0, 1, 2} and count.max() == 3
    keep = np.ones(shape, dtype=bool)
    mask, prob = np.zeros(shape, dtype=np.uint8), np.full(shape, MU.NODATA, dtype=np.float32)
    for k, o in enumerate(outs):
        uv = U.source_coords_ref(shape, gt, 32613, o["geotransform"], o["crs"], (64, 80))
        keep &= ~U.near_boundary(uv)
        m = index == k
        mask[m] = U.nearest_ref(o["pred_binary"].cpu().numpy()[None], uv, [0])[0][m]
        prob[m] = U.nearest_ref(o["prediction"].cpu().numpy()[None], uv, [MU.NODATA])[0][m]
    assert keep.mean() >= 0.999
    assert np.array_equal(new["pred_binary"].cpu().numpy()[keep], mask[keep])      # the restated gather by source_index
    assert U.mismatching_bytes(new["prediction"].cpu().numpy()[keep], prob[keep]) == 0
    assert new["pred_binary"].dtype == torch.uint8 and tuple(new["mf"].shape) == shape
    # one plume on the mosaic, two in the concatenated per-scene tables
    each = sum(len(plumes.plume_table(o["pred_binary"], mag1c=o["mf"], prob=o["prediction"])) for o in outs)
    products.annotate(new, new["pred_binary"], new["mf"], new["prediction"], gt, abs(gt[1] * gt[5]), plumes=True)
    assert each == 2 and len(new["plumes"]) == 1


def test_mosaic_products_file_to_file(hip, tmp_path):
    from starcop_amd import io_formats as io
    from starcop_amd import pipeline, products
    outs = scene_dicts()
    folders = []
    for i, o in enumerate(outs):
        folders.append(str(tmp_path / f"scene{i}"))
        products.write_rasters(o, (products.MAG1C, products.PRED, products.PREDBINARY), folders[-1], True,
                               warp.geo_tags(o["geotransform"], o["crs"]), MU.NODATA, {})
    want = products.mosaic(outs, 32613, 60.0, nodata=MU.NODATA)
    for cog in (False, True):
        dest = str(tmp_path / f"mosaic{int(cog)}")
        res = pipeline.mosaic_products(folders, dest, crs=32613, resolution=60.0, cog=cog)
        names = ("mag1c.tif", "pred.tif", "predbinary.tif", "source.tif")
        assert sorted(os.path.basename(f) for f in res["files"]) == sorted(names)
        for name, key in zip(names, ("mf", "prediction", "pred_binary", None)):
            path = os.path.join(dest, name)
            info = io.tiff_info(path)
            gt, epsg = io.geo_from_tags(info)
            assert epsg == 32613 and np.allclose(gt, want["geotransform"], rtol=0, atol=1e-6)
            a = io.read_tiff(path, info=info)
            a = a[0] if a.ndim == 3 else a
            if key is not None:
                assert U.mismatching_bytes(a, want[key].cpu().numpy()) == 0, name
            else:
                count = want["source_count"].cpu().numpy()
                assert a.dtype == np.uint8 and np.array_equal(a == 255, count == 0) and (count == 0).any()
                assert np.array_equal(a[a != 255], want["source_index"].cpu().numpy()[a != 255])
                assert "scene1" in str(info.tags[42112][1])
            if cog:
                assert io.cog_layout_problems(path) == [], name
    with pytest.raises(ValueError, match="georeferencing"):
        io.write_tiff(os.path.join(folders[0], "pred.tif"), outs[0]["prediction"].cpu().numpy())
        pipeline.mosaic_products(folders, str(tmp_path / "none"))
    with pytest.raises(NotImplementedError, match="Cloud Storage"):
        pipeline.mosaic_products(["gs://bucket/scene"], str(tmp_path / "none"))
