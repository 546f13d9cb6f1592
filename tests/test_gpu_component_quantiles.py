"""sc_component_quantiles / plumes.component_quantiles, component_median_mad and the ``background_stat="median"`` / ``percentiles=``
columns of plume_table against the numpy restatement of tests/component_quantiles_util.py.

Every comparison is ``np.array_equal(got, want, equal_nan=True)`` on float32 (a zero may have either sign, everything else is bit
equality) or exact integer equality: there is no tolerance in this file."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import component_quantiles_util as cq  # noqa: E402
import quantify_util as qu  # noqa: E402
from starcop_amd import _lib, mask_creation as mc, plumes, products, quantify as qf  # noqa: E402

DEV = "cuda"
T = _lib.CQUANT_SMALL_MAX
Q8 = (5, 25, "median", 75, 95, 2.5, 99.9, 33.3)
QSETS = {"median": ("median",), "minmax": (0, 100), "eight": Q8}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(lab, counts, plane, q=("median",), center=None, M=None):
    """labels (H, W) or (N, H, W), counts an int or (N,), plane numpy or a device tensor -> host (n_finite, quantile)"""
    counts = int(counts) if np.ndim(counts) == 0 else dev(np.asarray(counts, dtype=np.int32))
    plane_d = plane if isinstance(plane, torch.Tensor) else dev(plane)
    got = plumes.component_quantiles(dev(np.asarray(lab, dtype=np.int32)), counts, plane_d, q,
                                     center=None if center is None else dev(np.asarray(center, dtype=np.float32)), M=M)
    assert got["n_finite"].dtype == torch.int64 and got["quantile"].dtype == torch.float32
    assert got["quantile"].shape == got["n_finite"].shape + (len(q),)
    return got["n_finite"].cpu().numpy(), got["quantile"].cpu().numpy()


def check(lab, counts, plane, q=("median",), center=None, M=None, what=""):
    nf, qs = run(lab, counts, plane, q, center, M)
    wnf, wqs = cq.oracle(lab, np.atleast_1d(counts), plane, q, center, M)
    assert np.array_equal(nf, wnf), (what, nf, wnf)
    assert cq.same(qs, wqs), (what, np.argwhere(~((qs == wqs) | (np.isnan(qs) & np.isnan(wqs)))), qs, wqs)
    return nf, qs


def noisy_plane(rng, shape):
    p = (rng.standard_normal(shape) * 300).astype(np.float32)
    p[rng.random(shape) < 0.02] = np.nan
    flat = p.reshape(-1)
    flat[rng.choice(flat.size, 6, replace=False)] = [np.inf, -np.inf] * 3
    return p


@functools.lru_cache(maxsize=None)
def random_case(density, conn):
    rng = np.random.default_rng(int(density * 100) + conn)
    mask = rng.random((96, 150)) < density
    lab, cnt = mc.connected_components(dev(mask), connectivity=conn)
    return lab.cpu().numpy(), int(cnt), noisy_plane(rng, (96, 150))


@functools.lru_cache(maxsize=None)
def random_oracle(density, conn, qname):
    lab, cnt, plane = random_case(density, conn)
    return cq.oracle(lab, [cnt], plane, QSETS[qname])


# ------------------------------------------------------------------------------------------------------------- 1. random masks
@pytest.mark.parametrize("qname", list(QSETS))
@pytest.mark.parametrize("conn", [1, 2])
@pytest.mark.parametrize("density", [0.3, 0.55, 0.7])
def test_random_masks_equal_the_restatement(hip, density, conn, qname):
    lab, cnt, plane = random_case(density, conn)
    nf, qs = run(lab, cnt, plane, QSETS[qname])
    wnf, wqs = random_oracle(density, conn, qname)
    assert nf.shape == (1, cnt) and np.array_equal(nf, wnf)
    assert cq.same(qs, wqs), (density, conn, qname)
    if qname == "minmax":
        st = plumes.component_stats(dev(lab), cnt, [dev(plane)], M=cnt)
        assert np.array_equal(st["n_finite"][0, :, 0].cpu().numpy(), nf[0])
        assert np.array_equal(st["min"][0, :, 0].cpu().numpy(), qs[0, :, 0], equal_nan=True)
        assert np.array_equal(st["max"][0, :, 0].cpu().numpy(), qs[0, :, 1], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------- 2. small counts
def test_small_counts(hip):
    lab = np.zeros((9, 12), np.int32)
    plane = np.full((9, 12), np.nan, np.float32)
    vals = {1: [3.5], 2: [-2.0, 7.0], 3: [9.0, -4.0, 1.0], 4: [0.5, -0.25, 8.0, -16.0]}
    for k, v in vals.items():
        lab[k, :len(v) + 2] = k                     # two NaN pixels beside the finite ones
        plane[k, :len(v)] = v
    lab[6, 2:9] = 5                                 # all NaN
    lab[7, :6] = 6                                  # finite except for one NaN
    plane[7, :6] = [4.0, 2.0, np.nan, -6.0, 10.0, 0.0]
    nf, qs = check(lab, 6, plane, (0, 25, "median", 100))
    assert nf.tolist() == [[1, 2, 3, 4, 0, 5]]
    assert qs[0, 0].tolist() == [3.5] * 4 and qs[0, 1].tolist() == [-2.0, 0.25, 2.5, 7.0] and qs[0, 2, 2] == 1.0
    assert qs[0, 3].tolist() == [-16.0, -4.1875, 0.125, 8.0] and np.isnan(qs[0, 4]).all() and qs[0, 5, 2] == 2.0


def test_wave_sized_components(hip):
    """a row of at most 64 members is sorted by one wave, a larger one by a work-group: 63, 64, 65 and 66 finite values"""
    rng = np.random.default_rng(64)
    lab = np.zeros((8, 70), np.int32)
    plane = (rng.standard_normal((8, 70)) * 300).astype(np.float32)
    for k, n in enumerate([63, 64, 65, 66, 64]):
        lab[k, :] = k + 1
        plane[k, n:] = np.nan
    plane[4, :64] = np.rint(plane[4, :64] / 100)            # ties inside the wave
    nf, _ = check(lab, 5, plane, Q8)
    assert nf.tolist() == [[63, 64, 65, 66, 64]]
    check(lab, 5, plane, (0, "median", 100))


# ------------------------------------------------------------------------------------------------------- 3. ties and close keys
def _tie_planes():
    rng = np.random.default_rng(3)
    shape = (96, 150)
    tiny = np.array([1e-40, -1e-40, 0.0, -0.0, 1e-3, -1e-3], np.float32)
    return {
        "integers": np.rint(rng.standard_normal(shape) * 3).astype(np.float32),
        "last digit": (1.0 + rng.integers(0, 64, shape) * 2.0 ** -23).astype(np.float32),
        "denormals, zeros and the sign boundary": tiny[rng.integers(0, tiny.size, shape)],
        "constant": np.full(shape, -7.25, np.float32),
    }


@pytest.mark.parametrize("name", list(_tie_planes()))
def test_ties_and_close_keys(hip, name):
    lab, cnt, _ = random_case(0.55, 2)
    plane = _tie_planes()[name]
    check(lab, cnt, plane, Q8, what=name)
    check(np.ones_like(lab), 1, plane, Q8, what=name + ", one large component")


# --------------------------------------------------------------------------------------- 4. both selection paths, their boundary
@pytest.mark.parametrize("equal", [False, True])
def test_both_selection_paths_and_their_boundary(hip, equal):
    sizes = [T - 1, T, T + 1, 2 * T + 3]
    spare = 5                                       # NaN pixels per large label: the counts are set by construction
    side = int(np.ceil(np.sqrt(sum(sizes) + len(sizes) * spare + 150)))
    rng = np.random.default_rng(T + equal)
    order = rng.permutation(side * side)            # the members of every label are scattered over the image
    lab = np.zeros(side * side, np.int32)
    plane = (rng.standard_normal(side * side) * 300).astype(np.float32)
    at, holes = 0, []
    for k, n in enumerate(sizes):
        px = order[at:at + n + spare]
        lab[px] = k + 1
        holes.extend(px[n:])
        at += n + spare
    k = len(sizes)
    while at + 7 <= order.size and k < len(sizes) + 20:     # small components in the same image
        n = 1 + (k % 7)
        k += 1
        lab[order[at:at + n]] = k
        at += n
    if equal:                                       # every histogram pass sees one bin; and a sorted segment of equal keys
        plane[lab == 4] = -123.456
        plane[lab == 2] = 7.0
    plane[holes] = np.nan
    lab, plane = lab.reshape(side, side), plane.reshape(side, side)
    nf, _ = check(lab, k, plane, Q8, what=f"equal={equal}")
    assert nf[0, :4].tolist() == sizes
    check(lab, k, plane, ("median",))
    check(lab, k, plane, (0, 100))


# ----------------------------------------------------------------------------------------------- 5. labels that are not components
def test_ring_labels(hip):
    lab, cnt, plane = random_case(0.3, 2)
    rings = plumes.background_rings(lab, 6, 1)
    assert rings.max() > 0
    check(rings, cnt, plane, (5, "median", 95), what="rings")


def test_values_outside_the_counts_and_row_capacity(hip):
    lab, cnt, plane = random_case(0.55, 1)
    odd = lab.copy()
    odd[0, :5] = [-1, -2 ** 31, 2 ** 31 - 1, cnt + 1, cnt + 1000]
    nf, qs = check(odd, cnt, plane, (10, "median"), what="values outside [1, count]")
    cut, more = cnt // 2, cnt + 9
    nf_c, qs_c = check(odd, cnt, plane, (10, "median"), M=cut, what="M below the count")
    assert nf_c.shape == (1, cut) and np.array_equal(nf_c, nf[:, :cut]) and cq.same(qs_c, qs[:, :cut])
    nf_m, qs_m = check(odd, cnt, plane, (10, "median"), M=more, what="M above the count")
    assert nf_m.shape == (1, more) and not nf_m[0, cnt:].any() and np.isnan(qs_m[0, cnt:]).all()
    assert np.array_equal(nf_m[:, :cnt], nf) and cq.same(qs_m[:, :cnt], qs)
    low = check(odd, 3, plane, (10, "median"), M=cnt, what="a count below the labels")[0]
    assert not low[0, 3:].any()
    empty = plumes.component_quantiles(dev(odd), 0, dev(plane), M=0)
    assert empty["n_finite"].shape == (1, 0) and empty["quantile"].shape == (1, 0, 1)


# ----------------------------------------------------------------------------------------------------------------- 6. center
def test_median_mad_and_centres(hip):
    lab, cnt, plane = random_case(0.55, 2)
    got = plumes.component_median_mad(dev(lab), cnt, dev(plane))
    wnf, wmed, wmad = cq.median_mad(lab, [cnt], plane)
    assert [got[f].dtype for f in ("n_finite", "median", "mad")] == [torch.int64, torch.float32, torch.float32]
    assert np.array_equal(got["n_finite"].cpu().numpy(), wnf)
    assert cq.same(got["median"].cpu().numpy(), wmed) and cq.same(got["mad"].cpu().numpy(), wmad)
    rings = plumes.background_rings(lab, 6, 1)
    got = plumes.component_median_mad(dev(rings), cnt, dev(plane), M=cnt)
    wnf, wmed, wmad = cq.median_mad(rings, [cnt], plane, M=cnt)
    assert np.array_equal(got["n_finite"].cpu().numpy(), wnf)
    assert cq.same(got["median"].cpu().numpy(), wmed) and cq.same(got["mad"].cpu().numpy(), wmad)
    # a centre that is not finite empties its row and no other
    big = int(np.argmax(wnf[0]))
    centre = wmed.copy()
    centre[0, big] = np.nan
    centre[0, (big + 1) % cnt] = np.inf
    nf, qs = check(lab, cnt, plane, ("median", 90), center=centre, what="NaN centre")
    ref_nf, ref_qs = run(lab, cnt, plane, ("median", 90), center=wmed)
    rest = np.ones(cnt, bool)
    rest[[big, (big + 1) % cnt]] = False
    assert nf[0, big] == 0 and np.isnan(qs[0, big]).all() and nf[0, (big + 1) % cnt] == 0
    assert np.array_equal(nf[0, rest], ref_nf[0, rest]) and cq.same(qs[0, rest], ref_qs[0, rest])


# ------------------------------------------------------------------------------------------------------ 7. batch and determinism
def test_batch_rows_equal_single_calls_and_calls_repeat(hip):
    cases = [random_case(0.3, 2), random_case(0.55, 1), random_case(0.7, 2)]
    labs = np.stack([c[0] for c in cases])
    labs[2] = np.where(labs[2] > 0, 1 + np.arange(labs.shape[2])[None, :] % 2, 0)     # image 2: two interleaved labels above the threshold
    counts = np.array([cases[0][1], cases[1][1], 2], np.int32)
    planes = np.stack([c[2] for c in cases])
    M = int(counts.max())
    args = (dev(labs), dev(counts), dev(planes), Q8)
    one = plumes.component_quantiles(*args, M=M)
    two = plumes.component_quantiles(*args, M=M)
    for f in ("n_finite", "quantile"):
        assert one[f].cpu().numpy().tobytes() == two[f].cpu().numpy().tobytes(), f
    nf, qs = one["n_finite"].cpu().numpy(), one["quantile"].cpu().numpy()
    for n in range(3):
        s_nf, s_qs = run(labs[n], int(counts[n]), planes[n], Q8, M=M)
        assert nf[n].tobytes() == s_nf[0].tobytes() and qs[n].tobytes() == s_qs[0].tobytes(), n
    wnf, wqs = cq.oracle(labs[2], [2], planes[2], Q8, M=M)
    assert np.array_equal(nf[2:], wnf) and cq.same(qs[2:], wqs) and (wnf[0, :2] > T).all()


# ---------------------------------------------------------------------------------------------------- 8. a plane read in place
def test_plane_read_in_place_as_a_channel(hip):
    cases = [random_case(0.55, 2), random_case(0.7, 1)]
    labs = np.stack([c[0] for c in cases])
    counts = np.array([c[1] for c in cases], np.int32)
    rng = np.random.default_rng(8)
    cube = (rng.standard_normal((2, 3) + labs.shape[1:]) * 50).astype(np.float32)
    cube[:, 1] = np.stack([c[2] for c in cases])
    cube_d = dev(cube)
    view = cube_d[:, 1]
    assert not view.is_contiguous()
    nf, qs = run(labs, counts, view, (5, "median", 95))
    c_nf, c_qs = run(labs, counts, view.contiguous(), (5, "median", 95))
    assert nf.tobytes() == c_nf.tobytes() and qs.tobytes() == c_qs.tobytes()
    wnf, wqs = cq.oracle(labs, counts, cube[:, 1], (5, "median", 95))
    assert np.array_equal(nf, wnf) and cq.same(qs, wqs)


# ------------------------------------------------------------------------------------------------------------- 9. plume_table
PX = 4.0


def planted():
    """64 x 96, dyadic values (every float64 sum exact): a disc, a line and a blob over a noisy background with NaN"""
    rng = np.random.default_rng(9)
    mag = (rng.integers(-64 * 256, 64 * 256 + 1, size=(64, 96)) / 256.0).astype(np.float32)
    rr, cc = np.indices(mag.shape)
    mask = (rr - 40) ** 2 + (cc - 30) ** 2 <= 81
    mag[mask] = np.abs(mag[mask]) + 100.0
    mag[40, 30] = 1024.0
    mask[6, 10:40] = True
    mag[6, 10:40] = 3.5
    blob = (np.abs((rr - 30) - 0.5 * (cc - 75)) <= 2) & (np.abs(cc - 75) <= 14)
    mask |= blob
    mag[blob] = np.abs(mag[blob]) + 0.25
    mag[rng.random(mag.shape) < 0.03] = np.nan
    mag[40, 30] = 1024.0
    return mask, mag


def test_plume_table_median_background(hip, tmp_path):
    mask, mag = planted()
    lab, cnt = mc.connected_components(dev(mask), connectivity=2)
    lab, cnt = lab.cpu().numpy(), int(cnt)
    assert cnt == 3
    kw = dict(mag1c=dev(mag), pixel_area_m2=PX * PX, background_ring_px=6, background_gap_px=1)
    base = plumes.plume_table(dev(mask), **kw)
    # the default and "mean" leave the table and the file as they are
    mean = plumes.plume_table(dev(mask), background_stat="mean", percentiles=None, **kw)
    assert mean.equals(base)
    plumes.write_plumes(base, str(tmp_path / "base.csv"))
    plumes.write_plumes(mean, str(tmp_path / "mean.csv"))
    assert open(str(tmp_path / "base.csv"), "rb").read() == open(str(tmp_path / "mean.csv"), "rb").read()
    bare = plumes.plume_table(dev(mask), mag1c=dev(mag))
    assert plumes.plume_table(dev(mask), mag1c=dev(mag), background_stat="mean").equals(bare)
    # "median": the restatement from the oracle on background_rings
    table = plumes.plume_table(dev(mask), background_stat="median", **kw)
    new = ["mag1c_bg_median", "mag1c_bg_mad", "mag1c_bg_sigma", "ime_sigma_ppmm_m2", "snr"]
    assert list(table.columns) == list(base.columns) + new
    rings = plumes.background_rings(lab, 6, 1)
    wnf, wmed, wmad = cq.median_mad(rings, [cnt], mag)
    med, mad = wmed[0].astype(np.float64), wmad[0].astype(np.float64)
    n = np.array([np.isfinite(mag[lab == k]).sum() for k in range(1, cnt + 1)], np.float64)
    s = base["mag1c_sum"].to_numpy()
    assert np.array_equal(table["bg_px"], wnf[0]) and np.array_equal(table["bg_px"], base["bg_px"])
    assert np.array_equal(table["mag1c_bg_mean"], base["mag1c_bg_mean"]) and np.array_equal(table["mag1c_sum"], s)
    assert np.array_equal(table["mag1c_bg_median"], med) and np.array_equal(table["mag1c_bg_mad"], mad) and (mad > 0).all()
    assert np.array_equal(table["mag1c_sum_bgsub"], s - med * n) and not np.array_equal(table["mag1c_sum_bgsub"], base["mag1c_sum_bgsub"])
    assert np.array_equal(table["ime_bgsub_ppmm_m2"], (s - med * n) * (PX * PX))
    assert np.array_equal(table["mag1c_bg_sigma"], 1.4826 * mad)
    assert np.array_equal(table["ime_sigma_ppmm_m2"], 1.4826 * mad * np.sqrt(n) * (PX * PX))
    assert np.array_equal(table["snr"], (s - med * n) / (1.4826 * mad * np.sqrt(n)))
    # a plume without ring pixels: NaN median, NaN bgsub and snr, the other rows as before
    mag2 = mag.copy()
    mag2[rings == lab[30, 75]] = np.nan
    t2 = plumes.plume_table(dev(mask), background_stat="median", **{**kw, "mag1c": dev(mag2)})
    blob = int(lab[30, 75]) - 1
    assert t2["bg_px"][blob] == 0 and np.isnan(t2["mag1c_bg_median"][blob]) and np.isnan(t2["mag1c_sum_bgsub"][blob]) and np.isnan(t2["snr"][blob])
    keep = np.arange(cnt) != blob
    assert np.array_equal(t2["snr"][keep], table["snr"][keep])


def test_plume_table_quantify_follows_the_median(hip):
    mask, mag = planted()
    lab, cnt = mc.connected_components(dev(mask), connectivity=2)
    lab, cnt = lab.cpu().numpy(), int(cnt)
    q = {"wind_speed_m_s": 2.5, "max_fetch_m": 60.0, "kg_per_ppmm_m2": 2.0 ** -20}
    kw = dict(mag1c=dev(mag), pixel_area_m2=PX * PX, quantify=q, background_ring_px=6, background_gap_px=1)
    by_mean = plumes.plume_table(dev(mask), **kw)
    table, curves = plumes.fetch_profiles(dev(mask), dev(mag), q, pixel_area_m2=PX * PX, background_ring_px=6, background_gap_px=1,
                                          background_stat="median")
    assert table.equals(plumes.plume_table(dev(mask), background_stat="median", **kw))
    med = cq.median_mad(plumes.background_rings(lab, 6, 1), [cnt], mag)[1][0].astype(np.float64)
    jj = np.arange(1.0, 16.0)
    want, _ = qu.quantify_ref(lab, cnt, mag, jj, jj * PX, PX, 2.5, 2.0 ** -20, bg_mean=med)
    for c in qf.QUANTIFY_COLUMNS:
        got = table[c].to_numpy()
        assert np.array_equal(got, want[c], equal_nan=got.dtype.kind == "f"), c
    assert np.array_equal(curves["ime_kg"], want["_ime_profile_kg"])
    assert np.array_equal(table["ime_kg"], table["mag1c_sum_bgsub"] * (PX * PX) * 2.0 ** -20)
    assert not np.array_equal(table["ime_kg"], by_mean["ime_kg"])


def test_plume_table_percentiles(hip):
    mask, mag = planted()
    lab, cnt = mc.connected_components(dev(mask), connectivity=2)
    lab, cnt = lab.cpu().numpy(), int(cnt)
    base = plumes.plume_table(dev(mask), mag1c=dev(mag), prob=dev(np.abs(mag) / 2048))
    table = plumes.plume_table(dev(mask), mag1c=dev(mag), prob=dev(np.abs(mag) / 2048), percentiles=(5, "median", 95))
    assert [c for c in table.columns if c not in base.columns] == ["mag1c_p5", "mag1c_median", "mag1c_p95"]
    assert table.drop(columns=["mag1c_p5", "mag1c_median", "mag1c_p95"]).equals(base)
    _, wqs = cq.oracle(lab, [cnt], mag, (5, "median", 95))
    for j, c in enumerate(["mag1c_p5", "mag1c_median", "mag1c_p95"]):
        assert table[c].dtype == np.float64 and np.array_equal(table[c], wqs[0, :, j].astype(np.float64)), c
    small = plumes.plume_table(dev(mask), mag1c=dev(mag), percentiles=(2.5,), min_area=100)
    assert list(small.columns)[-1] == "mag1c_p2.5" and len(small) < cnt
    empty = plumes.plume_table(dev(np.zeros_like(mask)), mag1c=dev(mag), percentiles=(5, "median"), background_ring_px=4,
                               background_stat="median")
    assert len(empty) == 0 and "mag1c_bg_median" in empty.columns and "mag1c_median" in empty.columns


def test_annotate_passes_the_stat_through(hip):
    mask, mag = planted()
    out, ref = {}, {}
    products.annotate(out, dev(mask.astype(np.uint8)), dev(mag), dev(np.abs(mag) / 2048), None, PX * PX, plumes=True,
                      plume_background={"ring_px": 6, "gap_px": 1, "stat": "median"})
    products.annotate(ref, dev(mask.astype(np.uint8)), dev(mag), dev(np.abs(mag) / 2048), None, PX * PX, plumes=True,
                      plume_background={"ring_px": 6, "gap_px": 1})
    new = ["mag1c_bg_median", "mag1c_bg_mad", "mag1c_bg_sigma", "ime_sigma_ppmm_m2", "snr"]
    assert [c for c in out["plumes"].columns if c not in ref["plumes"].columns] == new
    want = plumes.plume_table(dev(mask), mag1c=dev(mag), prob=dev(np.abs(mag) / 2048), pixel_area_m2=PX * PX, background_ring_px=6,
                              background_gap_px=1, background_stat="median")
    assert out["plumes"].equals(want)


# ------------------------------------------------------------------------------------ 10. refusals through the C entry point
def test_error_codes_of_the_c_abi(hip):
    lib = hip
    H, W, M = 16, 20, 4
    lab = torch.zeros((H, W), dtype=torch.int32, device=DEV)
    counts = torch.tensor([M], dtype=torch.int32, device=DEV)
    plane = torch.zeros((H, W), device=DEV)
    nf = torch.zeros((1, M), dtype=torch.int64, device=DEV)
    qs = torch.zeros((1, M, 8), device=DEV)
    wb = lib.sc_component_quantiles_workspace_bytes(1, H, W, M, 8)
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device=DEV)

    def call(Q=1, q0=0.5, work_bytes=wb, **over):
        a = _lib.sc_cquant_args()
        a.labels, a.counts, a.N, a.H, a.W, a.M, a.Q = lab.data_ptr(), counts.data_ptr(), 1, H, W, M, Q
        a.plane, a.plane_stride, a.n_finite, a.quantile = plane.data_ptr(), H * W, nf.data_ptr(), qs.data_ptr()
        a.q[0] = q0
        for f, v in over.items():
            setattr(a, f, v)
        rc = lib.sc_component_quantiles(a, _lib.ptr(work), work_bytes, _lib.stream())
        return rc, lib.sc_last_error().decode() if rc else ""

    assert call()[0] == 0
    torch.cuda.synchronize()
    assert nf.cpu().tolist() == [[0] * M] and torch.isnan(qs.view(-1)[:M]).all()          # Q = 1: M values, densely
    for kw in (dict(Q=0), dict(Q=9), dict(q0=1.5), dict(q0=float("nan")), dict(work_bytes=wb - 1), dict(labels=None), dict(plane=None),
               dict(quantile=None), dict(N=0), dict(M=-1), dict(H=1 << 16, W=1 << 15)):
        rc, msg = call(**kw)
        assert rc == -1 and "sc_component_quantiles" in msg, (kw, rc, msg)          # SC_ERR_ARG, with a message
    assert lib.sc_component_quantiles_workspace_bytes(1, H, W, M, 0) == 0 and lib.sc_component_quantiles_workspace_bytes(1, H, W, M, 9) == 0
    assert lib.sc_component_quantiles_workspace_bytes(1, 1 << 16, 1 << 15, M, 1) == 0
