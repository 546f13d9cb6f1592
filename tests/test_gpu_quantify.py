"""sc_component_radial / plumes.component_radial and plume_table(quantify=...) against the numpy restatement of
tests/quantify_util.py.

Plane values are dyadic (integers / 256, |v| <= 1024) wherever equality is asked for: every float64 sum of them is exact in any
order, so all outputs are compared bit for bit.  On arbitrary float32 data a bin's sum may differ from the restatement's by the
rounding of two different summation orders of its n values: at most 2 * (n - 1) * 2^-53 * sum|v|, a property of float64."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import quantify_util as qu  # noqa: E402
from starcop_amd import _lib, mask_creation as mc, plumes, quantify as qf  # noqa: E402

DEV = "cuda"
R7 = [1.0, 1.5, 2.0, 3.0, 4.99, 5.0, 9.0]
RADII = {1: [5.0], 7: R7, 64: list(1.0 + 2.5 * np.arange(64))}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dyadic(rng, shape, top=1024):
    return (rng.integers(-top * 256, top * 256 + 1, size=shape) / 256.0).astype(np.float32)


def radial(lab, count, origins, radii, plane, M=None):
    """one (H, W) or (N, H, W) label image through component_stats and component_radial -> (host radial dict, device stats)"""
    lab_d = dev(lab.astype(np.int32))
    counts = int(count) if np.ndim(count) == 0 else dev(np.asarray(count, dtype=np.int32))
    plane_d = plane if isinstance(plane, torch.Tensor) else dev(plane)
    st = plumes.component_stats(lab_d, counts, [plane_d], M=M)
    if origins is None:
        org = plumes.origins_from_argmax(st, lab.shape[-1])
    else:
        org = dev(np.asarray(origins, dtype=np.int32).reshape(st["area"].shape + (2,)))
    got = plumes.component_radial(lab_d, counts, st, org, radii, plane_d, M=M)
    assert [got[f].dtype for f in qu.RADIAL_FIELDS] == [torch.int64, torch.float64] + [torch.int64] * 4
    host = {f: v.cpu().numpy() for f, v in got.items()}
    host["origin"] = org.cpu().numpy()
    return host, st


def same(got, n, want, what=""):
    """image n of a host radial dict == the restatement, bit for bit"""
    for f in qu.RADIAL_FIELDS:
        g, w = got[f][n], want[f]
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, f, g, w)
        if f == "bin_sum":
            assert not np.signbit(g[g == 0]).any(), (what, f, "an empty bin is +0.0")


@functools.lru_cache(maxsize=None)
def random_case(density, conn):
    rng = np.random.default_rng(int(density * 100) + conn)
    mask = rng.random((96, 150)) < density
    lab, cnt = mc.connected_components(dev(mask), connectivity=conn)
    return lab.cpu().numpy(), int(cnt), dyadic(rng, (96, 150))


# --------------------------------------------------------------------------------------------------------- exact equality
@pytest.mark.parametrize("K", [1, 7, 64])
@pytest.mark.parametrize("conn", [1, 2])
@pytest.mark.parametrize("density", [0.3, 0.55, 0.7])
def test_random_masks_equal_the_restatement(hip, density, conn, K):
    lab, cnt, plane = random_case(density, conn)
    got, _ = radial(lab, cnt, None, RADII[K], plane)
    origins = qu.argmax_origins(lab, cnt, cnt, plane)
    assert np.array_equal(got["origin"][0], origins)
    assert got["bin_count"].shape == (1, cnt, K + 1)
    same(got, 0, qu.radial_ref(lab, cnt, cnt, origins, qu.edges_of(RADII[K]), plane), (density, conn, K))


# -------------------------------------------------------------------------------------------------------- launch geometry
H, W = 128, 160


def block_image():
    lab = np.zeros((H, W), np.int32)
    lab[10:110, 20:150] = 1                         # 100 x 130: many row bands (four of the 32-row kind), wider than a wave
    return lab


def narrow_boxes():
    lab = np.zeros((H, W), np.int32)
    for k, (c0, w) in enumerate([(2, 1), (6, 2), (12, 3), (20, 5), (30, 64)]):       # several rows per wave step; the exact wave
        lab[5:75, c0:c0 + w] = k + 1
    return lab


GEOMETRY = {
    "block": (block_image, 1, [(60, 80)]),
    "block, origin outside the box": (block_image, 1, [(3, 155)]),
    "corner 00": (block_image, 1, [(0, 0)]), "corner 0W": (block_image, 1, [(0, W - 1)]),
    "corner H0": (block_image, 1, [(H - 1, 0)]), "corner HW": (block_image, 1, [(H - 1, W - 1)]),
    "narrow boxes": (narrow_boxes, 5, [(5, 2), (40, 7), (74, 13), (0, 0), (40, 60)]),
    "whole image": (lambda: np.ones((H, W), np.int32), 1, [(64, 80)]),
    "skipped": (narrow_boxes, 5, [(5, 2), (-1, -1), (74, 13), (-1, 7), (40, 60)]),
}


@pytest.mark.parametrize("case", list(GEOMETRY))
def test_launch_geometry(hip, case):
    make, cnt, origins = GEOMETRY[case]
    lab = make()
    plane = dyadic(np.random.default_rng(len(case)), (H, W))
    got, _ = radial(lab, cnt, origins, R7, plane)
    want = qu.radial_ref(lab, cnt, cnt, np.asarray(origins), qu.edges_of(R7), plane)
    same(got, 0, want, case)
    if case == "skipped":
        for k in (1, 3):
            assert got["d2_max"][0, k] == -1 and not got["bin_count"][0, k].any() and not got["sum_rr"][0, k]
    if case == "block":
        assert got["bin_count"][0, 0].sum() == 100 * 130


def test_rows_without_pixels_values_above_the_count_and_spare_rows(hip):
    lab = np.zeros((H, W), np.int32)
    lab[3:40, 5:9] = 1
    lab[50:90, 30:100] = 3                          # no pixel carries 2
    lab[100:120, 10:20] = 7                         # above the count: ignored
    plane = dyadic(np.random.default_rng(9), (H, W))
    M = 6
    origins = np.array([(3, 5), (10, 10), (60, 40), (0, 0), (0, 0), (0, 0)])
    got, st = radial(lab, 3, origins, R7, plane, M=M)
    same(got, 0, qu.radial_ref(lab, 3, M, origins, qu.edges_of(R7), plane))
    for k in (1, 3, 4, 5):
        assert got["d2_max"][0, k] == -1 and not got["bin_count"][0, k].any() and not got["bin_sum"][0, k].view(np.int64).any()
    assert got["bin_count"][0, 2].sum() == 40 * 70


# ------------------------------------------------------------------------------------------------------------ the edge rule
def test_edge_rule_and_overflow_bin(hip):
    lab = np.zeros((16, 16), np.int32)
    lab[5, 5] = lab[8, 9] = lab[15, 15] = 1         # offsets (0, 0), (3, 4): d2 = 25, and (10, 10): d2 = 200
    plane = np.zeros((16, 16), np.float32)
    plane[5, 5], plane[8, 9], plane[15, 15] = 1.0, 2.0, 4.0
    got, _ = radial(lab, 1, [(5, 5)], [4.99, 5.0], plane)
    assert got["bin_count"][0, 0].tolist() == [1, 1, 1] and got["bin_sum"][0, 0].tolist() == [1.0, 2.0, 4.0]
    got, _ = radial(lab, 1, [(5, 5)], [5.0], plane)                  # inside radius 5.0
    assert got["bin_count"][0, 0].tolist() == [2, 1] and got["bin_sum"][0, 0].tolist() == [3.0, 4.0]
    got, _ = radial(lab, 1, [(5, 5)], [4.99], plane)                 # outside 4.99: the overflow bin
    assert got["bin_count"][0, 0].tolist() == [1, 2] and got["bin_sum"][0, 0].tolist() == [1.0, 6.0]
    assert got["d2_max"][0, 0] == 200
    got, _ = radial(lab, 1, [(5, 5)], [0.5, 14.2], plane)            # floor(0.25) = 0: the origin pixel alone
    assert got["bin_count"][0, 0].tolist() == [1, 2, 0]


# -------------------------------------------------------------------------------------------------------- non-finite values
def test_non_finite_values(hip):
    lab = np.zeros((40, 70), np.int32)
    lab[4:30, 3:68] = 1
    plane = dyadic(np.random.default_rng(3), (40, 70))
    plane[29, 67] = np.nan                          # the farthest pixel from the origin
    plane[4, 3], plane[10, 20], plane[11, 21] = np.nan, np.inf, -np.inf
    got, st = radial(lab, 1, [(4, 3)], R7, plane)
    same(got, 0, qu.radial_ref(lab, 1, 1, np.array([(4, 3)]), qu.edges_of(R7), plane))
    assert got["bin_count"][0, 0].sum() == 26 * 65 - 4 and np.isfinite(got["bin_sum"]).all()
    assert got["d2_max"][0, 0] == 25 ** 2 + 64 ** 2
    rr, cc = np.nonzero(lab == 1)
    assert got["sum_rr"][0, 0] == (rr.astype(np.int64) ** 2).sum() and got["sum_rc"][0, 0] == (rr.astype(np.int64) * cc).sum()
    assert got["bin_count"][0, 0, 0] == 2           # d2 <= 1: the two neighbours; the origin pixel itself is NaN


# --------------------------------------------------------------------------------------- consistency with component_stats
def test_consistent_with_component_stats(hip):
    import plumes_util as pu
    lab, cnt, plane = random_case(0.55, 2)
    plane = plane.copy()
    plane[::7, ::5] = np.nan
    speck = np.flatnonzero(np.bincount(lab.ravel(), minlength=cnt + 1)[1:] == 1)[0] + 1
    plane[lab == speck] = np.nan                    # a single pixel without a finite value: no maximum, no origin
    got, st = radial(lab, cnt, None, R7, plane)
    host = {f: v.cpu().numpy() for f, v in st.items()}
    assert np.array_equal(got["bin_count"].sum(-1), host["n_finite"][..., 0])
    assert np.array_equal(got["bin_sum"].sum(-1), host["sum"][..., 0])
    rows, cols = np.indices(lab.shape)
    skipped_none = True
    for k in range(1, cnt + 1):
        sel = lab == k
        r, c = rows[sel].astype(np.int64), cols[sel].astype(np.int64)
        r0, c0 = got["origin"][0, k - 1]
        if r0 < 0:                                  # every value of the component is NaN: no maximum, skipped
            assert host["n_finite"][0, k - 1, 0] == 0 and got["d2_max"][0, k - 1] == -1 and got["sum_rr"][0, k - 1] == 0
            skipped_none = False
            continue
        assert got["d2_max"][0, k - 1] == ((r - r0) ** 2 + (c - c0) ** 2).max()
        assert got["sum_rr"][0, k - 1] == (r * r).sum() and got["sum_cc"][0, k - 1] == (c * c).sum()
        assert got["sum_rc"][0, k - 1] == (r * c).sum()
    assert not skipped_none                         # the case has specks on NaN pixels
    want = pu.oracle_stats(lab, cnt, [plane])       # the statistics call itself is what it was
    for f in pu.COMPONENT_FIELDS + ("n_finite", "argmax"):
        assert np.array_equal(host[f][0], want[f]), f
    assert np.array_equal(host["sum"][0], want["sum"]) and np.array_equal(host["max"][0], want["max"], equal_nan=True)
    assert np.array_equal(host["min"][0], want["min"], equal_nan=True)


# --------------------------------------------------------------------------------------------------------------------- bits
def batch_case():
    rng = np.random.default_rng(77)
    labs, cnts = [], []
    for d in (0.3, 0.55, 0.7):
        lab, cnt = mc.connected_components(dev(rng.random((96, 150)) < d), connectivity=2)
        labs.append(lab.cpu().numpy())
        cnts.append(int(cnt))
    M = max(cnts)
    return np.stack(labs), cnts, M, rng.random((3, 96, 150)).astype(np.float32) * 2000.0 - 500.0


def test_repeated_calls_and_batches_give_identical_bytes(hip):
    labs, cnts, M, plane = batch_case()
    a, _ = radial(labs, cnts, None, R7, plane, M=M)
    b, _ = radial(labs, cnts, None, R7, plane, M=M)
    for f in qu.RADIAL_FIELDS:
        assert a[f].tobytes() == b[f].tobytes(), f
    for n in range(3):
        one, _ = radial(labs[n], cnts[n], None, R7, plane[n], M=M)
        for f in qu.RADIAL_FIELDS:
            assert one[f][0].tobytes() == a[f][n].tobytes(), (n, f)


def test_float32_data_within_the_bound_of_two_summation_orders(hip):
    labs, cnts, M, plane = batch_case()
    got, _ = radial(labs, cnts, None, R7, plane, M=M)
    for n in range(3):
        want = qu.radial_ref(labs[n], cnts[n], M, got["origin"][n], qu.edges_of(R7), plane[n])
        for f in ("bin_count", "d2_max", "sum_rr", "sum_cc", "sum_rc"):
            assert np.array_equal(got[f][n], want[f]), (n, f)
        tol = 2.0 * np.maximum(want["bin_count"] - 1, 0) * 2.0 ** -53 * want["bin_abs"]
        err = np.abs(got["bin_sum"][n] - want["bin_sum"])
        assert (err <= tol).all(), (n, float(err.max()), float(tol[err > tol].min()))


# -------------------------------------------------------------------------------------------------------- a plane in place
def test_plane_read_in_place_as_a_channel(hip):
    labs, cnts, M, _ = batch_case()
    rng = np.random.default_rng(5)
    cube = dyadic(rng, (3, 4, 96, 150))
    cube_d = dev(cube)
    view = cube_d[:, 2]
    assert not view.is_contiguous()
    got, _ = radial(labs, cnts, None, R7, view, M=M)
    for n in range(3):
        same(got, n, qu.radial_ref(labs[n], cnts[n], M, got["origin"][n], qu.edges_of(R7), cube[n, 2]), n)
    assert np.array_equal(cube_d.cpu().numpy(), cube)


# -------------------------------------------------------------------------------------------------------------- error codes
def test_error_codes_of_the_c_abi(hip):
    N, h, w, M, K = 1, 32, 48, 3, 4
    lab = dev(np.zeros((N, h, w), np.int32))
    counts = dev(np.array([0], np.int32))
    box = [torch.zeros((N, M), dtype=torch.int32, device=DEV) for _ in range(4)]
    org = torch.zeros((N, M, 2), dtype=torch.int32, device=DEV)
    plane = torch.zeros((N, h, w), dtype=torch.float32, device=DEV)
    outs = [torch.ones((N, M, K + 1), dtype=torch.int64, device=DEV), torch.ones((N, M, K + 1), dtype=torch.float64, device=DEV)] + \
           [torch.ones((N, M), dtype=torch.int64, device=DEV) for _ in range(4)]
    wb = hip.sc_component_radial_workspace_bytes(N, h, w, M, K)
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device=DEV)

    def args(**kw):
        a = _lib.sc_cradial_args()
        a.labels, a.counts, a.N, a.H, a.W, a.M, a.K = lab.data_ptr(), counts.data_ptr(), N, h, w, M, K
        a.row_min, a.row_max, a.col_min, a.col_max = (t.data_ptr() for t in box)
        a.origin, a.plane, a.plane_stride = org.data_ptr(), plane.data_ptr(), h * w
        for j, e in enumerate(kw.pop("edges", [1, 4, 9, 16])):
            a.edge2[j] = e
        for f, t in zip(qu.RADIAL_FIELDS, outs):
            setattr(a, f, t.data_ptr())
        for f, v in kw.items():
            setattr(a, f, v)
        return a

    def call(a, nbytes=wb):
        return hip.sc_component_radial(a, _lib.ptr(work), nbytes, _lib.stream())
    assert call(args()) == 0
    for bad in (args(K=0), args(K=65), args(edges=[1, 4, 4, 16]), args(edges=[9, 4, 16, 25]), args(edges=[-1, 4, 9, 16]),
                args(labels=None), args(counts=None), args(plane=None), args(origin=None), args(row_max=None), args(bin_sum=None),
                args(d2_max=None), args(N=0), args(H=0), args(W=40000), args(M=-1)):
        assert call(bad) == -1 and b"sc_component_radial" in hip.sc_last_error()
    assert call(args(), wb - 1) == -1 and b"workspace" in hip.sc_last_error()
    assert hip.sc_component_radial(None, _lib.ptr(work), wb, _lib.stream()) == -1
    assert hip.sc_component_radial_workspace_bytes(N, h, w, M, 0) == 0 and hip.sc_component_radial_workspace_bytes(N, h, w, M, 65) == 0
    assert call(args(M=0, row_min=None, bin_count=None), 0) == 0                    # nothing to write: SC_OK
    torch.cuda.synchronize()
    assert (outs[2] == -1).all() and all(not t.view(torch.uint8).any() for i, t in enumerate(outs) if i != 2)     # count 0: zero rows, d2_max -1


def test_component_radial_refuses_bad_arguments(hip):
    lab = dev(np.ones((8, 9), np.int32))
    plane = dev(np.ones((8, 9), np.float32))
    st = plumes.component_stats(lab, 1, [plane])
    org = plumes.origins_from_argmax(st, 9)
    assert org.dtype == torch.int32 and org.cpu().tolist() == [[[0, 0]]]
    plumes.component_radial(lab, 1, st, org, [1.0], plane)
    for radii in ([], list(np.arange(1, 66.0)), [1.0, 1.2], [2.0, 1.0], [0.0, 1.0], [-1.0], [float("nan")], [1.0, 2.0 ** 15.5]):
        with pytest.raises(ValueError):
            plumes.component_radial(lab, 1, st, org, radii, plane)
    with pytest.raises(ValueError):
        plumes.component_radial(lab, 1, st, org, [1.0], plane[:, :8])                # shape mismatch
    with pytest.raises(ValueError):
        plumes.component_radial(lab, 1, st, org[:, :, :1], [1.0], plane)
    with pytest.raises(ValueError):
        plumes.component_radial(lab, 1, st, org, [1.0], plane.cpu())                 # a CPU tensor
    with pytest.raises(ValueError):
        plumes.component_radial(lab.cpu(), 1, st, org, [1.0], plane)
    with pytest.raises(ValueError):
        plumes.component_radial(lab, 1, st, org.cpu(), [1.0], plane)
    no = plumes.origins_from_argmax(plumes.component_stats(lab, 1, [plane * float("nan")]), 9)
    assert no.cpu().tolist() == [[[-1, -1]]]


# ----------------------------------------------------------------------------------------- plume_table(quantify=...) end to end
PX = 4.0                                            # pixel size in m: the area and the radii in m are exact
GT = (500000.0, PX, 0.0, 4100000.0, 0.0, -PX)
LINE_E = 3.5


def planted():
    """a 64 x 96 scene: a one-pixel-wide horizontal line of constant enhancement from (6, 10), 30 long; a filled disc of radius
    9 around its maximum at (40, 30); a slanted blob; dyadic noise elsewhere"""
    rng = np.random.default_rng(11)
    mask = np.zeros((64, 96), bool)
    mag = dyadic(rng, (64, 96), top=64)
    mask[6, 10:40] = True
    mag[6, 10:40] = LINE_E
    rr, cc = np.indices(mask.shape)
    disc = (rr - 40) ** 2 + (cc - 30) ** 2 <= 81
    mask |= disc
    mag[disc] = np.abs(mag[disc]) + 1.0
    mag[40, 30] = 1024.0
    blob = (np.abs((rr - 30) - 0.5 * (cc - 75)) <= 2) & (np.abs(cc - 75) <= 14)
    mask |= blob
    mag[blob] = np.abs(mag[blob]) + 0.25
    return mask, mag


def assert_quantify_columns(table, want, rows=None):
    for c in qf.QUANTIFY_COLUMNS:
        got, w = table[c].to_numpy(), want[c] if rows is None else want[c][rows]
        assert np.array_equal(got, w, equal_nan=got.dtype.kind == "f"), (c, got, w)


def test_plume_table_quantify_on_planted_plumes(hip, tmp_path):
    mask, mag = planted()
    lab, cnt = mc.connected_components(dev(mask), connectivity=2)
    lab, cnt = lab.cpu().numpy(), int(cnt)
    assert cnt == 3
    kg = qf.kg_per_ppmm_m2()
    radii_px = np.array([1.5, 2.0, 3.7, 5.0, 12.0, 40.0])
    q = {"wind_speed_m_s": 2.5, "radii_m": list(radii_px * PX)}
    kw = dict(mag1c=dev(mag), geotransform=GT, pixel_area_m2=PX * PX)
    plain = plumes.plume_table(dev(mask), **kw)
    table = plumes.plume_table(dev(mask), quantify=q, **kw)
    assert [c for c in table.columns if c not in plain.columns] == list(qf.QUANTIFY_COLUMNS)
    assert table.drop(columns=list(qf.QUANTIFY_COLUMNS)).equals(plain)
    want, rad = qu.quantify_ref(lab, cnt, mag, radii_px, radii_px * PX, PX, 2.5, kg)
    assert_quantify_columns(table, want)
    # the line: IME_j = e * (floor(r_j) + 1) * a * kg while the circle ends inside it, and everything from the first that holds it
    line = int(lab[6, 10]) - 1
    assert (table["origin_row"][line], table["origin_col"][line]) == (6, 10) and table["fetch_max_m"][line] == 29 * PX
    _, curves = plumes.fetch_profiles(dev(mask), dev(mag), q, geotransform=GT, pixel_area_m2=PX * PX)
    ime = (LINE_E * (np.minimum(np.floor(radii_px), 29) + 1)) * (PX * PX) * kg
    assert np.array_equal(curves["ime_kg"][line], ime) and np.array_equal(curves["ime_kg"], want["_ime_profile_kg"])
    assert np.array_equal(curves["n_px"][line], np.minimum(np.floor(radii_px), 29) + 1)
    assert curves["used"][line].tolist() == [True] * 6 and table["q_fetch_n"][line] == 6       # 12 px < 29 px: 40 px is the first to hold it
    assert table["ime_kg"][line] == LINE_E * 30 * (PX * PX) * kg
    assert table["minor_axis_m"][line] == 0.0 and table["orientation_rad"][line] == np.pi / 2
    assert table["major_axis_m"][line] == 4.0 * np.sqrt((30 * 30 - 1) / 12.0) * PX
    # the disc: isotropic, held by the 12 px circle
    disc = int(lab[40, 30]) - 1
    assert table["orientation_rad"][disc] == 0.0 and table["major_axis_m"][disc] == table["minor_axis_m"][disc]
    assert table["fetch_max_m"][disc] == 9 * PX and table["q_fetch_n"][disc] == 5
    q_j = 3600.0 * 2.5 * want["_ime_profile_kg"][disc][:5] / (radii_px[:5] * PX)
    assert table["q_fetch_kg_h"][disc] == q_j.sum() / 5.0 and table["q_fetch_kg_h"][disc] > 0
    # defaults: r_j = j * pixel size up to 150 m; per-plume winds and origins; min_area keeps their alignment
    dflt = plumes.plume_table(dev(mask), quantify={"wind_speed_m_s": [1.0, 2.0, 3.0], "min_fetch_m": 10.0}, min_area=100, **kw)
    jj = np.arange(1.0, 38.0)
    want_d, _ = qu.quantify_ref(lab, cnt, mag, jj, jj * PX, PX, np.array([1.0, 2.0, 3.0]), kg, min_fetch_m=10.0)
    keep = np.flatnonzero(np.bincount(lab.ravel(), minlength=cnt + 1)[1:] >= 100)
    assert len(dflt) == len(keep) < cnt
    assert_quantify_columns(dflt, want_d, keep)
    org = np.array([[6.0, 39.9], [np.nan, 0.0], [40.2, 30.0]])[np.argsort([line, 3 - line - disc, disc])]
    given = plumes.plume_table(dev(mask), quantify={**q, "origin": org}, **kw)
    want_g, _ = qu.quantify_ref(lab, cnt, mag, radii_px, radii_px * PX, PX, 2.5, kg, origins=np.where(np.isnan(org), -1, np.floor(org)).astype(np.int64))
    assert_quantify_columns(given, want_g)
    assert given["origin_col"][line] == 39 and np.isnan(given["q_fetch_kg_h"][3 - line - disc]) and given["q_fetch_n"][3 - line - disc] == 0
    xy = np.stack([GT[0] + (np.floor(org[:, 1]) + 0.25) * GT[1], GT[3] + (np.floor(org[:, 0]) + 0.25) * GT[5]], 1)
    by_xy = plumes.plume_table(dev(mask), quantify={**q, "origin": xy, "origin_xy": True}, **kw)
    assert by_xy.equals(given)
    # no plume at all: the columns are there, no row is
    empty = plumes.plume_table(dev(np.zeros_like(mask)), quantify=q, **kw)
    assert len(empty) == 0 and [c for c in empty.columns if c not in plain.columns] == list(qf.QUANTIFY_COLUMNS)
    # quantify=None: the table and the file it becomes are what they were
    none = plumes.plume_table(dev(mask), quantify=None, **kw)
    assert none.equals(plain)
    plumes.write_plumes(none, str(tmp_path / "none.csv"))
    plumes.write_plumes(plain, str(tmp_path / "plain.csv"))
    assert open(str(tmp_path / "none.csv"), "rb").read() == open(str(tmp_path / "plain.csv"), "rb").read()
    for bad, extra in (({"wind": 1.0}, {}), ({"wind_speed_m_s": 1.0, "fetch": 3}, {}), ({"wind_speed_m_s": 1.0, "max_fetch_m": 3.0}, {}),
                       ({"wind_speed_m_s": 1.0}, {"pixel_area_m2": None}), ({"wind_speed_m_s": 1.0}, {"mag1c": None}),
                       ({"wind_speed_m_s": 1.0}, {"geotransform": (0.0, 4.0, 0.0, 0.0, 0.0, -5.0)}),
                       ({"wind_speed_m_s": [1.0, 2.0]}, {}), ({"wind_speed_m_s": 1.0, "origin": org[:2]}, {})):
        with pytest.raises(ValueError):
            plumes.plume_table(dev(mask), quantify=bad, **{**kw, **extra})


def test_plume_table_quantify_above_the_background_ring(hip):
    mask, mag = planted()
    lab, cnt = mc.connected_components(dev(mask), connectivity=2)
    lab, cnt = lab.cpu().numpy(), int(cnt)
    q = {"wind_speed_m_s": 2.5, "max_fetch_m": 60.0, "kg_per_ppmm_m2": 2.0 ** -20}
    kw = dict(mag1c=dev(mag), pixel_area_m2=PX * PX, quantify=q)
    plain = plumes.plume_table(dev(mask), **kw)
    mag2 = mag.copy()
    ring_of_blob = plumes.background_rings(lab, 3.0, 1.0) == lab[30, 75]
    mag2[ring_of_blob] = np.nan                     # the blob has no background: NaN rates
    ringed = plumes.plume_table(dev(mask), background_ring_px=3.0, background_gap_px=1.0, **{**kw, "mag1c": dev(mag2)})
    jj = np.arange(1.0, 16.0)
    bg = ringed["mag1c_bg_mean"].to_numpy()
    want, _ = qu.quantify_ref(lab, cnt, mag2, jj, jj * PX, PX, 2.5, 2.0 ** -20, bg_mean=bg)
    assert_quantify_columns(ringed, want)
    blob = int(lab[30, 75]) - 1
    assert ringed["bg_px"][blob] == 0 and np.isnan(ringed["ime_kg"][blob]) and np.isnan(ringed["q_fetch_kg_h"][blob])
    assert np.isnan(ringed["q_sqrt_area_kg_h"][blob]) and np.isfinite(ringed["fetch_max_m"][blob])
    disc = int(lab[40, 30]) - 1
    assert ringed["bg_px"][disc] > 0 and ringed["ime_kg"][disc] != plain["ime_kg"][disc]
    assert ringed["ime_kg"][disc] == ringed["mag1c_sum_bgsub"][disc] * (PX * PX) * 2.0 ** -20


# ------------------------------------------------------------------------------------------------------------ one scene call
def test_scene_call_writes_the_quantification_columns(hip, tmp_path):
    """the 70 x 100 ENVI flight line of the background-ring scene test: plumes.csv and the GeoJSON properties gain the columns,
    and without the keyword no byte of any file changes"""
    import pandas as pd
    import plume_scene_util as SU
    from starcop_amd import io_formats, pipeline, products
    from test_gpu_plume_scene import _model
    h, w = 70, 100
    model = _model(bias=-0.93)
    valid = SU.strip_mask(h, w, centre=30.0, slope=0.3, half_width=25.0)
    planes = SU.flight_line(h, w, 61, valid=valid)[0]
    cube = np.stack([planes[3], planes[2], planes[1]], axis=-1)
    folder = SU.write_flight_line(str(tmp_path / "ang20190101t180000_rdn"), cube, np.array([460.0, 550.0, 640.0]))
    io_formats.write_tiff(os.path.join(folder, "mag1c.tif"), planes[0], blocksize=128, extra_tags={42113: (2, ("-9999",))})
    kw = dict(toa_correction_factor=1.037, tile=32, halo=32, plumes=True, plume_outlines=True)
    names = ("plumes.csv", "plumes.geojson", "pred.tif", "predbinary.tif")

    def read(sub):
        return [open(str(tmp_path / sub / n), "rb").read() for n in names]
    before = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "before"), **kw)
    q = {"wind_speed_m_s": 3.0}
    out = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "quant"), plume_quantify=q, **kw)
    pipeline.aviris_scene_predict(model, folder, str(tmp_path / "after"), plume_quantify=None, **kw)
    assert read("after") == read("before")
    assert read("quant")[2:] == read("before")[2:]
    csv = pd.read_csv(str(tmp_path / "quant" / "plumes.csv"))
    old = pd.read_csv(str(tmp_path / "before" / "plumes.csv"))
    new = list(qf.QUANTIFY_COLUMNS)
    assert len(csv) >= 1 and [c for c in csv.columns if c not in old.columns] == new
    assert csv.drop(columns=new).equals(old) and before["plumes"].equals(out["plumes"].drop(columns=new))
    gt = (500000.0, 5.0, 0.0, 4100000.0, 0.0, -5.0)
    table = plumes.plume_table(out["pred_binary"], mag1c=out["mf"], prob=out["prediction"], geotransform=gt, pixel_area_m2=25.0, quantify=q)
    assert table.equals(out["plumes"]) and np.isfinite(table["q_sqrt_area_kg_h"]).any()
    feats = json.load(open(str(tmp_path / "quant" / "plumes.geojson")))["features"]
    assert len(feats) == len(table)
    for feat, row in zip(feats, table.to_dict("records")):
        for c in new:
            v = feat["properties"][c]
            assert (v is None and not np.isfinite(row[c])) or v == row[c], (c, v, row[c])
    with pytest.raises(ValueError):
        pipeline.aviris_scene_predict(model, folder, str(tmp_path / "bad"), plume_quantify={"wind_speed_m_s": 3.0, "u10": 2}, **kw)
    assert not os.path.exists(str(tmp_path / "bad"))
    # a longitude / latitude grid has no pixel area
    with pytest.raises(ValueError, match="utm"):
        products.annotate({}, out["pred_binary"], out["mf"], out["prediction"], (-103.0, 5e-4, 0.0, 32.0, 0.0, -5e-4), None, plumes=True,
                          plume_quantify=q)
