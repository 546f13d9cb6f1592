"""sc_component_stats / starcop_amd.plumes against the numpy + scipy oracle of tests/plumes_util.py.

Integer columns are equal; max / min are bit-equal apart from the sign of a zero (numeric equality of float32 values, NaN where
the oracle has NaN); every fp64 sum lies within area * 2^-50 * sum|x| of math.fsum -- 8 x the first-order bound
(area - 1) * 2^-53 * sum|x| of a float64 summation in ANY order, a property of float64, not of the kernel."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import plumes_util as pu  # noqa: E402
from starcop_amd import _lib, mask_creation as mc, plumes, stacks  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = os.path.join(ROOT, "tests", "golden", "io", "emit_l1b_like_sb0.nc")


def _host(st):
    return {k: v.cpu().numpy() for k, v in st.items()}


def _check_rows(got, n, want, count, what=""):
    """rows [0, count) of image n of a host stats dict == the oracle's; rows at or above count are zero"""
    for f in pu.COMPONENT_FIELDS:
        assert np.array_equal(got[f][n, :count], want[f]), (what, f, got[f][n, :count], want[f])
        assert not got[f][n, count:].any(), (what, f, "rows above the count are not zero")
    for f in ("n_finite", "argmax"):
        assert np.array_equal(got[f][n, :count], want[f]), (what, f)
    for f in ("max", "min"):
        assert got[f].dtype == np.float32
        assert np.array_equal(got[f][n, :count], want[f], equal_nan=True), (what, f)
    tol = want["area"][:, None] * 2.0 ** -50 * want["sum_abs"]
    err = np.abs(got["sum"][n, :count] - want["sum"])
    assert (err <= tol).all(), (what, "sum", float(err.max()), float(tol[err > tol].min()))
    for f in pu.PLANE_FIELDS:
        assert not got[f][n, count:].view(np.uint8).any(), (what, f, "rows above the count are not zero")


def _run(lab, count, planes=(), other=None, M=None):
    """one image through component_stats and the oracle; returns the host stats"""
    st = plumes.component_stats(torch.from_numpy(lab.astype(np.int32)).to(DEV), int(count),
                                [torch.from_numpy(p).to(DEV) for p in planes],
                                None if other is None else torch.from_numpy(other).to(DEV), M=M)
    got = _host(st)
    _check_rows(got, 0, pu.oracle_stats(lab, count, planes, other), count, (lab.shape, count))
    return got


def _labelled(mask, conn):
    lab, cnt = mc.connected_components(torch.from_numpy(mask).to(DEV), connectivity=conn)
    want, n = pu.scipy_label(mask, conn)
    assert cnt == n and np.array_equal(lab.cpu().numpy(), want)
    return want, n


#          shape, density, seed, connectivity, components, largest (or None), single pixels (or None): counted with scipy
RANDOM = [((1, 1), 1.0, 4, 1, 1, 1, 1), ((1, 1), 1.0, 4, 2, 1, 1, 1),
          ((1, 7), 0.6, 5, 1, 1, 5, 0), ((1, 7), 0.6, 5, 2, 1, 5, 0),
          ((5, 1), 0.6, 6, 1, 1, 4, 0), ((5, 1), 0.6, 6, 2, 1, 4, 0),
          ((33, 65), 0.35, 1, 1, 270, 35, 151), ((33, 65), 0.35, 1, 2, 93, 76, 33),
          ((64, 64), 0.35, 7, 1, 506, 48, 271), ((64, 64), 0.35, 7, 2, 138, 169, 49),
          ((130, 257), 0.35, 2, 1, 3983, 44, 2039), ((130, 257), 0.35, 2, 2, 1055, 353, 356),
          ((130, 257), 0.55, 3, 2, 67, 18227, 46)]          # one large component whose box spans the image, next to specks


@pytest.mark.parametrize("shape,dens,seed,conn,count,largest,singles", RANDOM,
                         ids=[f"{c[0][0]}x{c[0][1]}-p{c[1]}-conn{c[3]}" for c in RANDOM])
def test_random_masks(hip, shape, dens, seed, conn, count, largest, singles):
    rng = np.random.default_rng(seed)
    mask = rng.random(shape) < dens
    planes = [(rng.standard_normal(shape) * 800).astype(np.float32) for _ in range(2)]
    other = (rng.random(shape) < 0.3).astype(np.uint8)
    lab, n = _labelled(mask, conn)
    areas = np.bincount(lab.ravel(), minlength=2)[1:]
    assert (n, int(areas.max()), int((areas == 1).sum())) == (count, largest, singles)
    got = _run(lab, n, planes, other)
    assert got["area"].shape == (1, n) and got["sum"].shape == (1, n, 2)


def test_all_foreground_and_all_background(hip):
    rng = np.random.default_rng(11)
    shape = (130, 257)
    planes = [(rng.standard_normal(shape) * 800).astype(np.float32)]
    lab, n = _labelled(np.ones(shape, bool), 2)
    assert n == 1
    got = _run(lab, 1, planes)
    assert got["area"][0, 0] == 130 * 257 and got["first_pixel"][0, 0] == 0
    assert (got["row_max"][0, 0], got["col_max"][0, 0]) == (129, 256)
    lab, n = _labelled(np.zeros(shape, bool), 2)
    assert n == 0
    got = _run(lab, 0, planes)
    assert got["area"].shape == (1, 0) and got["sum"].shape == (1, 0, 1)
    got = _run(lab, 0, planes, M=4)                 # capacity above the count: every output is zero-filled
    assert got["area"].shape == (1, 4) and got["max"].shape == (1, 4, 1)


@pytest.mark.parametrize("conn", (1, 2))
def test_structured_masks(hip, conn):
    rng = np.random.default_rng(12 + conn)
    cb = (np.add.outer(np.arange(16), np.arange(16)) % 2) == 0
    masks = {"checkerboard": (cb, {1: 128, 2: 1}), "spiral": (pu.spiral(65), {1: 1, 2: 1}),
             "stripes": (pu.diagonal_stripes(70, 90), {1: int(pu.diagonal_stripes(70, 90).sum()), 2: 40})}
    for name, (mask, counts) in masks.items():
        lab, n = _labelled(mask, conn)
        assert n == counts[conn], name
        planes = [(rng.standard_normal(mask.shape) * 800).astype(np.float32)]
        got = _run(lab, n, planes, (rng.random(mask.shape) < 0.5).astype(np.uint8))
        if name == "spiral":
            box = (got["row_max"][0, 0] - got["row_min"][0, 0] + 1) * (got["col_max"][0, 0] - got["col_min"][0, 0] + 1)
            assert box == 65 * 65 and got["area"][0, 0] * 3 < box * 2


def test_arbitrary_labels(hip):
    """values that are not components of anything: every label is scattered over the whole image"""
    rng = np.random.default_rng(21)
    lab = rng.integers(0, 40, (70, 90)).astype(np.int32)
    planes = [(rng.standard_normal(lab.shape) * 800).astype(np.float32) for _ in range(2)]
    other = (rng.random(lab.shape) < 0.5).astype(np.uint8)
    assert len(np.unique(lab)) == 40
    clean = _run(lab, 39, planes, other)
    assert (clean["area"][0] > 100).all()
    stray = lab.copy()
    where = rng.choice(lab.size, 12, replace=False)
    stray.ravel()[where[:6]], stray.ravel()[where[6:]] = 1000, -3
    got = _run(stray, 39, planes, other)
    assert got["area"].sum() == clean["area"].sum() - int((lab.ravel()[where] > 0).sum())
    # a count below the values present: the values above it are ignored too
    _run(lab, 17, planes, other)
    # a count above them: values no pixel carries give empty rows
    got = _run(lab, 45, planes, other)
    assert not got["area"][0, 39:].any() and (got["first_pixel"][0, 39:] == -1).all() and (got["argmax"][0, 39:] == -1).all()


def test_non_finite_values(hip):
    rng = np.random.default_rng(31)
    mask = np.zeros((40, 70), bool)
    mask[2:12, 3:30] = True          # 1: NaN / inf sprinkled in
    mask[20:24, 5:9] = True          # 2: all NaN
    mask[20:30, 40:66] = True        # 3: a plateau of equal maxima
    mask[34:38, 10:50] = True        # 4: all negative
    lab, n = _labelled(mask, 2)
    assert n == 4
    v = (rng.standard_normal(mask.shape) * 800).astype(np.float32)
    spr = rng.choice(10 * 27, 30, replace=False)
    blk = v[2:12, 3:30].copy().ravel()
    blk[spr[:10]], blk[spr[10:20]], blk[spr[20:]] = np.nan, np.inf, -np.inf
    v[2:12, 3:30] = blk.reshape(10, 27)
    v[20:24, 5:9] = np.nan
    v[20:30, 40:66] = np.minimum(v[20:30, 40:66], 100.0)
    v[22, 50:60] = 2500.0
    v[27, 41:45] = 2500.0
    v[34:38, 10:50] = -np.abs(v[34:38, 10:50]) - 1.0
    got = _run(lab, 4, [v, -v])
    assert got["n_finite"][0, 0, 0] == 270 - 30 and got["n_finite"][0, 1, 0] == 0
    assert np.isnan(got["max"][0, 1, 0]) and np.isnan(got["min"][0, 1, 0]) and got["argmax"][0, 1, 0] == -1 and got["sum"][0, 1, 0] == 0
    assert got["max"][0, 2, 0] == 2500.0 and got["argmax"][0, 2, 0] == 22 * 70 + 50
    assert got["min"][0, 2, 1] == -2500.0
    assert got["max"][0, 3, 0] < 0


def test_batch_bits(hip):
    rng = np.random.default_rng(41)
    N, H, W = 3, 64, 96
    masks = np.zeros((N, H, W), bool)
    masks[1, 10:50, 20:90] = True
    masks[2] = rng.random((H, W)) < 0.4
    labs = np.zeros((N, H, W), np.int32)
    counts = []
    for n in range(N):
        labs[n], c = pu.scipy_label(masks[n], 2)
        counts.append(c)
    assert counts[0] == 0 and counts[1] == 1 and counts[2] > 50
    M = max(counts) + 5
    planes = [(rng.standard_normal((N, H, W)) * 800).astype(np.float32) for _ in range(2)]
    other = (rng.random((N, H, W)) < 0.3).astype(np.uint8)
    d_lab, d_cnt = torch.from_numpy(labs).to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)
    d_pl, d_ot = [torch.from_numpy(p).to(DEV) for p in planes], torch.from_numpy(other).to(DEV)
    a = _host(plumes.component_stats(d_lab, d_cnt, d_pl, d_ot, M=M))
    b = _host(plumes.component_stats(d_lab, d_cnt, d_pl, d_ot, M=M))
    for f in a:
        assert a[f].shape[:2] == (N, M)
        assert a[f].tobytes() == b[f].tobytes(), f                        # two calls: identical bits
    for n in range(N):
        _check_rows(a, n, pu.oracle_stats(labs[n], counts[n], [p[n] for p in planes], other[n]), counts[n], ("batch", n))
        alone = _host(plumes.component_stats(d_lab[n], counts[n], [p[n] for p in d_pl], d_ot[n]))
        for f in a:
            assert alone[f][0].tobytes() == a[f][n, :counts[n]].tobytes(), (f, n)      # alone == inside the batch
    # the default capacity is the largest count
    assert plumes.component_stats(d_lab, d_cnt)["area"].shape == (N, max(counts))
    # a device count above the capacity: the first M components, and nothing written outside the M rows.  Through the C ABI,
    # with three guard rows behind every column
    M, G, P = 7, 3, 2
    assert counts[2] > M
    cols = {f: torch.full((M + G,), 0x7b7b7b7b7b7b7b7b, dtype=torch.int64, device=DEV) for f in pu.COMPONENT_FIELDS}
    cols.update({f: torch.full(((M + G) * P,), 0x7b7b7b7b7b7b7b7b, dtype=torch.int64, device=DEV) for f in pu.PLANE_FIELDS})
    args = _lib.sc_cstats_args()
    args.labels, args.counts, args.N, args.H, args.W, args.M, args.P = d_lab[2].data_ptr(), d_cnt[2:].data_ptr(), 1, H, W, M, P
    for q in range(P):
        args.plane[q], args.plane_stride[q] = d_pl[q][2].data_ptr(), H * W
    args.other, args.other_stride = d_ot[2].data_ptr(), H * W
    for f, t in cols.items():
        setattr(args, f, t.data_ptr())
    wb = hip.sc_component_stats_workspace_bytes(1, H, W, M, P)
    work = torch.empty(wb, dtype=torch.uint8, device=DEV)
    assert hip.sc_component_stats(C.byref(args), _lib.ptr(work), wb, _lib.stream()) == 0
    width = {"row_min": 4, "row_max": 4, "col_min": 4, "col_max": 4, "max": 4, "min": 4}
    small = {}
    for f, t in cols.items():
        raw = t.cpu().numpy().view(np.uint8)
        used = M * (P if f in pu.PLANE_FIELDS else 1) * width.get(f, 8)
        assert (raw[used:] == 0x7b).all(), (f, "written outside the M rows")
        dt = {"sum": np.float64, "max": np.float32, "min": np.float32}.get(f, np.int32 if width.get(f) == 4 else np.int64)
        small[f] = raw[:used].view(dt).reshape((1, M, P) if f in pu.PLANE_FIELDS else (1, M))
    _check_rows(small, 0, pu.oracle_stats(labs[2], M, [p[2] for p in planes], other[2]), M, "capacity below the count")


def test_strided_planes_are_read_in_place(hip):
    rng = np.random.default_rng(51)
    N, H, W = 2, 33, 65
    masks = rng.random((N, H, W)) < 0.35
    d_lab, d_cnt = mc.connected_components(torch.from_numpy(masks).to(DEV))
    x = torch.from_numpy((rng.standard_normal((N, 3, H, W)) * 800).astype(np.float32)).to(DEV)
    rgba = torch.from_numpy((rng.random((N, 4, H, W)) < 0.3).astype(np.uint8) * 255).to(DEV)
    ops = [stacks.plane_operand(p, torch.float32) for p in (x[:, 0], x[:, 2])]
    oth = stacks.plane_operand(rgba[:, 3], torch.uint8)
    assert [t.data_ptr() for t, _ in ops] == [x[:, 0].data_ptr(), x[:, 2].data_ptr()] and [s for _, s in ops] == [3 * H * W] * 2
    assert oth[0].data_ptr() == rgba[:, 3].data_ptr() and oth[1] == 4 * H * W
    got = _host(plumes.component_stats(d_lab, d_cnt, [x[:, 0], x[:, 2]], rgba[:, 3]))
    copy = _host(plumes.component_stats(d_lab, d_cnt, [x[:, 0].contiguous(), x[:, 2].contiguous()], rgba[:, 3].contiguous()))
    for f in got:
        assert got[f].tobytes() == copy[f].tobytes(), f
    labs, counts, xs, oth_h = d_lab.cpu().numpy(), d_cnt.cpu().numpy(), x.cpu().numpy(), rgba.cpu().numpy()
    for n in range(N):
        assert counts[n] > 50
        _check_rows(got, n, pu.oracle_stats(labs[n], counts[n], [xs[n, 0], xs[n, 2]], oth_h[n, 3]), counts[n], ("strided", n))


def test_read_back_of_the_stats_columns(hip):
    """``stacks.read_back`` of a ``component_stats`` dict (int32, int64, float32 and float64 columns) is every column's own copy,
    byte for byte, with rows and with M = 0"""
    rng = np.random.default_rng(52)
    N, H, W = 2, 33, 65
    d_lab, d_cnt = mc.connected_components(torch.from_numpy(rng.random((N, H, W)) < 0.35).to(DEV))
    x = torch.from_numpy((rng.standard_normal((N, H, W)) * 800).astype(np.float32)).to(DEV)
    for M in (None, 0):
        st = plumes.component_stats(d_lab, d_cnt, [x], M=M)
        got, want = stacks.read_back(st), _host(st)
        assert list(got) == list(want) and got["area"].shape[1] == (0 if M == 0 else int(d_cnt.max()))
        for f in want:
            assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, f
            assert got[f].tobytes() == want[f].tobytes() and got[f].flags.c_contiguous and got[f].flags.aligned, f


@pytest.mark.parametrize("with_other", (False, True))
@pytest.mark.parametrize("P", (0, 1, 8))
def test_plane_counts(hip, P, with_other):
    rng = np.random.default_rng(60 + P)
    mask = rng.random((33, 65)) < 0.35
    lab, n = pu.scipy_label(mask, 2)
    assert n > 50
    planes = [(rng.standard_normal(mask.shape) * 800).astype(np.float32) for _ in range(P)]
    other = (rng.random(mask.shape) < 0.3).astype(np.uint8) if with_other else None
    got = _run(lab, n, planes, other)
    assert got["sum"].shape == (1, n, P)
    assert with_other or not got["n_other"].any()


def test_error_codes_through_the_c_abi(hip):
    lab = torch.zeros((1, 4, 4), dtype=torch.int32, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(N=1, H=4, W=4, M=1, P=0, labels=lab, work_bytes=1 << 20):
        a = _lib.sc_cstats_args()
        a.labels, a.counts = (labels.data_ptr() if labels is not None else None), cnt.data_ptr()
        a.N, a.H, a.W, a.M, a.P = N, H, W, M, P
        return hip.sc_component_stats(C.byref(a), None, work_bytes, None)
    SC_ERR_ARG = -1
    assert call(P=9) == SC_ERR_ARG
    assert call(H=1 << 16, W=1 << 15) == SC_ERR_ARG            # H*W = 2^31: dims only, nothing is allocated or dereferenced
    assert call(N=0) == SC_ERR_ARG
    assert call(N=65536) == SC_ERR_ARG
    assert call(labels=None) == SC_ERR_ARG
    assert call() == SC_ERR_ARG                                # null output columns / workspace
    assert b"sc_component_stats" in hip.sc_last_error()
    assert hip.sc_component_stats_workspace_bytes(1, 1 << 16, 1 << 15, 1, 0) == 0
    assert hip.sc_component_stats_workspace_bytes(1, 64, 64, 10, 2) >= (10 + 1) * (40 + 2 * 32)
    torch.cuda.synchronize()


GT = (-103.75, 0.0005, 0.0, 32.5, 0.0, -0.0005)


def _planted_scene():
    H, W = 96, 160
    mask = np.zeros((H, W), bool)
    mag = np.full((H, W), 10.0, np.float32)
    prob = np.full((H, W), 0.25, np.float32)
    mask[10:20, 30:50] = True                # 200 px, mag 500 with a 900 peak at (12, 41)
    mag[10:20, 30:50] = 500.0
    mag[12, 41] = 900.0
    prob[10:20, 30:50] = 0.75
    mask[40:43, 100:104] = True              # 12 px, an L: drop one corner -> 11 px
    mask[40, 103] = False
    mag[40:43, 100:104] = 250.0
    prob[40:43, 100:104] = 0.5
    mask[70:90, 5] = True                    # 20 px column, mag = row index
    mag[70:90, 5] = np.arange(70, 90, dtype=np.float32)
    mask[60, 150] = True                     # the single pixel min_area drops
    mag[60, 150] = 333.0
    label = np.zeros((H, W), bool)
    label[15:25, 30:40] = True               # covers 5 x 10 of the first blob
    return mask, mag, prob, label


def test_plume_table_end_to_end(hip):
    mask, mag, prob, label = _planted_scene()
    want = pd.DataFrame({
        "item": [0, 0, 0], "plume_id": [1, 2, 4], "area_px": [200, 11, 20],
        "row_min": [10, 40, 70], "row_max": [19, 42, 89], "col_min": [30, 100, 5], "col_max": [49, 103, 5],
        "centroid_row": [14.5, (40 * 3 + 41 * 4 + 42 * 4) / 11, 79.5], "centroid_col": [39.5, (12 * 101.5 - 103) / 11, 5.0],
        "mag1c_sum": [199 * 500.0 + 900.0, 11 * 250.0, float(sum(range(70, 90)))],
        "mag1c_mean": [(199 * 500.0 + 900.0) / 200, 250.0, 79.5], "mag1c_max": [900.0, 250.0, 89.0],
        "mag1c_max_row": [12, 40, 89], "mag1c_max_col": [41, 100, 5],
        "ime_ppmm_m2": [(199 * 500.0 + 900.0) * 3600.0, 11 * 250.0 * 3600.0, sum(range(70, 90)) * 3600.0],
        "prob_mean": [0.75, 0.5, 0.25], "prob_max": [0.75, 0.5, 0.25], "overlap_px": [50, 0, 0]})
    want["x"] = GT[0] + (want["centroid_col"] + 0.5) * GT[1]
    want["y"] = GT[3] + (want["centroid_row"] + 0.5) * GT[5]
    kw = dict(min_area=2, geotransform=GT, pixel_area_m2=3600.0)
    dev = plumes.plume_table(torch.from_numpy(mask).to(DEV), mag1c=torch.from_numpy(mag).to(DEV), prob=torch.from_numpy(prob).to(DEV),
                             label_mask=torch.from_numpy(label).to(DEV), **kw)
    host = plumes.plume_table(mask, mag1c=mag, prob=prob, label_mask=label, **kw)
    for t in (dev, host):
        pd.testing.assert_frame_equal(t, want, check_exact=True)        # every sum here is exact in float64
    pu.assert_table(dev, pu.oracle_table(mask, 2, mag, prob, label, **kw))
    full = plumes.plume_table(mask, mag1c=mag)
    assert full["area_px"].tolist() == [200, 11, 1, 20] and full["mag1c_max"].tolist() == [900.0, 250.0, 333.0, 89.0]
    assert "x" not in full.columns and "prob_mean" not in full.columns and "overlap_px" not in full.columns
    # a batch: item numbers the images
    both = plumes.plume_table(np.stack([mask, label]), mag1c=np.stack([mag, mag]))
    assert both["item"].tolist() == [0, 0, 0, 0, 1] and both["area_px"].tolist() == [200, 11, 1, 20, 100]


def test_match_plumes(hip):
    pred = np.zeros((32, 32), bool)
    lab = np.zeros((32, 32), bool)
    pred[2:6, 2:6] = True
    lab[4:9, 4:9] = True                     # pair A: 4 shared pixels
    pred[12:16, 20:28] = True
    lab[10:20, 18:30] = True                 # pair B: the detection lies inside the label, 32 shared pixels
    pred[25:28, 2:5] = True                  # spurious
    lab[28:31, 24:27] = True                 # missed
    pred[20:23, 15:18] = True                # touches label B at its corner (19, 18) only: no shared pixel
    m = plumes.match_plumes(pred, lab)
    assert (m["tp"], m["fp"], m["fn"]) == (2, 2, 1)
    assert m["pred"]["overlap_px"].tolist() == [4, 32, 0, 0] and m["label"]["overlap_px"].tolist() == [4, 32, 0]
    assert m["pred"]["area_px"].tolist() == [16, 32, 9, 9] and m["label"]["area_px"].tolist() == [25, 120, 9]
    assert m["precision"] == 0.5 and m["recall"] == 2 / 3
    m5 = plumes.match_plumes(torch.from_numpy(pred).to(DEV), torch.from_numpy(lab).to(DEV), min_overlap_px=5)
    assert (m5["tp"], m5["fp"], m5["fn"]) == (1, 3, 2) and m5["precision"] == 0.25 and m5["recall"] == 1 / 3
    assert plumes.match_plumes(pred, lab, min_area=10)["pred"]["area_px"].tolist() == [16, 32]


GT_EMIT = (-110.25, 0.000542232520256367, 0.0, 35.5, 0.0, -0.000542232520256367)


def _emit_oracle(out, geotransform):
    fill = out["fill_value"]
    prob = out["prediction"].cpu().numpy()
    mf = out["mf"].cpu().numpy()[:prob.shape[0], :prob.shape[1]]        # sensor geometry: the network crops to multiples of 32
    return pu.oracle_table(out["pred_binary"].cpu().numpy() != 0, 2, np.where(mf == fill, np.nan, mf),
                           np.where(prob == fill, np.nan, prob), geotransform=geotransform)


def test_emit_granule_predict_plumes(hip, tmp_path):
    from starcop_amd import model_module as mm, pipeline
    torch.manual_seed(0)
    model = mm.ModelModule(mm.default_settings(pos_weight=1)).to(DEV).eval()
    tifs = ["albedo.tif", "mag1c.tif", "pred.tif", "predbinary.tif", "rgb.tif"]
    base = pipeline.emit_granule_predict(model, NC, column_step=4, georeferenced=True, out_folder=str(tmp_path / "base"), geotransform=GT_EMIT)
    out = pipeline.emit_granule_predict(model, NC, column_step=4, georeferenced=True, out_folder=str(tmp_path / "with"), geotransform=GT_EMIT,
                                        plumes=True)
    # plumes=False: the keys and files of before
    assert "plumes" not in base and set(out) == set(base) | {"plumes"}
    assert sorted(os.listdir(tmp_path / "base")) == tifs and sorted(os.path.basename(p) for p in base["files"]) == tifs
    assert sorted(os.listdir(tmp_path / "with")) == tifs[:2] + ["plumes.csv"] + tifs[2:]
    assert [os.path.basename(p) for p in out["files"]] == [os.path.basename(p) for p in base["files"]] + ["plumes.csv"]
    for k in ("mf", "prediction", "pred_binary"):
        assert torch.equal(out[k], base[k]), k
    table = out["plumes"]
    want = _emit_oracle(out, GT_EMIT)
    print(f"georeferenced: {len(want['item'])} plumes, areas {want['area_px'].tolist()[:8]}")
    pu.assert_table(table, want)
    assert len(table) >= 1                          # the seeded model predicts plumes on the fixture: the comparison is not empty
    back = pd.read_csv(tmp_path / "with" / "plumes.csv", float_precision="round_trip")
    assert list(back.columns) == list(table.columns) and len(back) == len(table)
    for c in table.columns:
        assert np.array_equal(back[c].to_numpy(dtype=np.float64), table[c].to_numpy(dtype=np.float64), equal_nan=True), c
    # sensor geometry: no x / y
    raw = pipeline.emit_granule_predict(model, NC, column_step=4, plumes=True)
    want = _emit_oracle(raw, None)
    print(f"sensor geometry: {len(want['item'])} plumes, areas {want['area_px'].tolist()[:8]}")
    assert "x" not in raw["plumes"].columns and "files" not in raw
    assert len(raw["plumes"]) >= 1
    pu.assert_table(raw["plumes"], want)
