"""The launch geometry of the fused training block (csrc/conv_irt.hip) and the case table of tests/test_gpu_irt_variants.py (no GPU).

sc_irt_geometry is the host query the launchers of conv_irt.hip compute their grids through.  Here it is swept over every Cin and
hidden the block accepts and planes from 4 x 8 up to the large cases: its invariants must hold, and the set of geometry classes it
reaches under the size caps of an ordinary case must EQUAL the set of classes of the ordinary rows of the GPU table -- deleting a row, or
a launcher gaining a path without a case, fails this test; so does a row whose shape no longer has the class written next to it, and a
table that loses one of the loops, chunk shapes or ABI modes it is there for."""
import pytest

from test_gpu_irt_variants import CAPS, CASES, LOOPS, flags_of, geo_class, is_ragged, per_channel, source_of
from starcop_amd import _lib

CINS = (8, 16, 24, 32)
HIDDENS = tuple(range(8, 193, 8))
# H x W within the caps of an ordinary case (4096 pixels per image): square, wide, and the narrow planes that maximise the tile counts
PLANES_SMALL = ((4, 8), (4, 16), (8, 32), (12, 24), (16, 64), (20, 40), (28, 56), (36, 72), (40, 72), (64, 64), (4, 1024), (128, 32),
                (256, 16), (344, 8), (348, 8), (508, 8), (512, 8))
PLANES_LARGE = ((64, 64 * 16), (128, 128), (256, 256), (164, 208), (164, 232), (152, 296), (148, 296), (104, 224), (512, 512))
ORDINARY = [c for c in CASES if "big" not in flags_of(c)]
BIG = [c for c in CASES if "big" in flags_of(c)]


def _sweep(planes, batches):
    for Cin in CINS:
        for hidden in HIDDENS:
            for H, W in planes:
                for N in batches:
                    yield N, Cin, hidden, H, W


def test_geometry_invariants():
    lib = _lib.load()
    n = 0
    for N, Cin, hidden, H, W in list(_sweep(PLANES_SMALL, (1, 2, 3))) + list(_sweep(PLANES_LARGE, (1, 3, 16))):
        if N * H * W * hidden >= 2 ** 31:
            assert _lib.irt_geometry(N, Cin, hidden, H, W) is None
            continue
        g = _lib.irt_geometry(N, Cin, hidden, H, W)
        key = (N, Cin, hidden, H, W, g)
        assert g is not None and lib.sc_irt_supported(Cin, hidden, H, W, 2) == 1, key
        NP = N * H * W
        assert (g["nks"], g["nch"], g["ngroups"]) == (-(-Cin // 16), -(-hidden // 32), -(-hidden // 96)), key
        # rows agree with the row queries the callers size their buffers by
        assert g["stats_grid"] == lib.sc_irt_rows(0, N, H, W, 2) and g["fwd_tiles"] == lib.sc_irt_rows(1, N, H, W, 2), key
        assert g["bwd_rows"] == lib.sc_irt_bwd_rows(N, hidden, H, W), key
        # H % 4 == 0 and W % 8 == 0: the flat 32-pixel blocks of k_irt_stats / k_irt_fix are never ragged against the batch
        assert g["pixel_blocks"] * 32 == NP, key
        assert g["fwd_tiles"] == N * -(-(H // 2) // 4) * -(-(W // 2) // 16) and g["bwd_tiles"] == N * (H // 4) * -(-W // 32), key
        # every grid at least 1 and at most its cap, and every loop covers its range
        assert 1 <= g["stats_grid"] <= 512 and g["stats_grid"] == min(512, -(-g["pixel_blocks"] // 4)), key
        assert 1 <= g["fwd_per_cu"] <= 4 and 1 <= g["fwd_grid"] == min(g["fwd_tiles"], 256 * g["fwd_per_cu"]), key
        assert 1 <= g["bwd_rows"] and g["bwd_rows"] * g["ngroups"] <= 512 and g["tiles_per_wg"] >= 1, key
        assert g["bwd_rows"] * g["tiles_per_wg"] >= g["bwd_tiles"] > (g["bwd_rows"] - 1) * g["tiles_per_wg"], key
        # (the last k_irt_xmom work-groups may be left without a step: 34,112 steps in 256 shares of 134; they write zero rows)
        assert 1 <= g["mom_grid"] <= 256 and g["mom_grid"] == min(256, -(-NP // 256)) and g["mom_ksteps"] == -(-(NP // 16) // g["mom_grid"]), key
        assert 1 <= g["fix_grid"] <= 1024 and g["fix_grid"] == min(1024, -(-g["pixel_blocks"] // 4)), key
        # the workspace holds the sections the kernels index with these rows (conv_irt.hip irt_work), + the ABI's 16 floats of slack
        sections = (g["bwd_rows"] * g["nch"] * 32 * 32, g["mom_grid"] * 33 * 32, 2 * 33 * 32, 33 * 32, g["nch"] * 4 * 3 * 64 * 4,
                    g["ngroups"] * N * Cin * H * W)
        assert sum(sections) + 16 <= lib.sc_irt_bwd_workspace_floats(N, Cin, hidden, H, W) <= sum(sections) + 16 + 4, key
        n += 1
    assert n > 5000


def test_rejected_blocks():
    ok = (2, 16, 96, 32, 64, 2)
    assert _lib.irt_geometry(*ok) is not None
    for i, bad in ((0, 0), (0, -1), (1, 20), (1, 40), (1, 4), (2, 200), (2, 0), (3, 6), (3, 0), (4, 60), (5, 1), (0, 2 ** 31 // (96 * 32 * 64) + 1)):
        a = list(ok)
        a[i] = bad
        assert _lib.irt_geometry(*a) is None, a
    assert _lib.load().sc_irt_geometry(*ok, None) != 0


def test_case_table_reaches_every_class_under_the_caps():
    assert CAPS == dict(N=3, pixels=4096)
    for case in CASES:
        cls, N, Cin, Hd, H, W, _ = case
        assert geo_class(_lib.irt_geometry(N, Cin, Hd, H, W), Hd) == cls, case
    got = {geo_class(_lib.irt_geometry(N, Cin, hd, H, W), hd) for N, Cin, hd, H, W in _sweep(PLANES_SMALL, (1, 2, 3))}
    want = {(nks, nch, full, "", False) for nks in (1, 2) for nch in range(1, 7) for full in (True, False)}
    want |= {(nks, nch, full, "b", short) for nks in (1, 2) for nch in (4, 5, 6) for full in (True, False) for short in (True, False)}
    assert got == {c[0] for c in ORDINARY} == want and len(want) == 48
    assert len(ORDINARY) == len(want), "one ordinary case per class"


def test_cases_stay_within_the_size_caps():
    for case in ORDINARY:
        _, N, Cin, Hd, H, W, _ = case
        assert N <= CAPS["N"] and H * W <= CAPS["pixels"], case
        assert (H <= 40 and W <= 72) or W == 8, case
    assert len(BIG) == 2 and all(c[1] <= CAPS["N"] and c[1] * c[4] * c[5] <= 135000 for c in BIG)


def test_large_cases_make_every_loop_iterate():
    loops = set("".join(c[0][3] for c in BIG))
    assert loops == set(LOOPS)
    g = {c[0][:2]: _lib.irt_geometry(*c[1:6]) for c in BIG}
    a, b = g[(2, 6)], g[(1, 1)]
    assert (a["fwd_tiles"], a["fwd_per_cu"], a["fwd_grid"]) == (294, 1, 256) and (a["bwd_tiles"], a["ngroups"], a["tiles_per_wg"], a["bwd_rows"]) == (574, 2, 3, 192)
    assert a["stats_grid"] == 512 and a["mom_grid"] == 256 and a["mom_ksteps"] == 17
    assert (b["pixel_blocks"], b["fix_grid"], b["bwd_tiles"], b["ngroups"], b["tiles_per_wg"]) == (4218, 1024, 1140, 1, 3)
    # tiles_per_wg > 1 with the last work-group short, and with one and two chunk groups
    assert any(c[0][4] and "b" in c[0][3] for c in BIG) and {_lib.irt_geometry(*c[1:6])["ngroups"] for c in BIG} == {1, 2}


def test_chunk_shapes_and_modes_are_covered():
    by = lambda pred: [c for c in CASES if pred(c, flags_of(c))]      # noqa: E731
    hiddens = {c[3] for c in ORDINARY}
    assert {8, 32, 104, 128} <= hiddens and {c[0][1] for c in ORDINARY} == set(range(1, 7))
    assert any((c[1], c[4], c[5]) == (1, 4, 8) for c in ORDINARY)                                   # the smallest plane
    for c in CASES:
        assert ("ragged" in flags_of(c)) <= is_ragged(c), c
    for nks in (1, 2):
        mine = by(lambda c, f: c[0][0] == nks)
        assert {source_of(c) for c in mine} == {"raw", "affine", "relu", "relu6"}, nks
        for flag in ("fix4", "nostats", "ragged"):
            assert any(flag in flags_of(c) for c in mine), (nks, flag)
        assert any(flags_of(c) & {"bnb6", "bnbn"} for c in mine), nks
        assert any(c[0][1] == 4 and not c[0][2] and "fix4" in flags_of(c) for c in mine)            # the one-chunk second group, partial
    for flag in ("bnb6", "bnbn"):      # each gradient-source activation on a ragged case and on a large case
        assert by(lambda c, f: flag in f and "ragged" in f and "big" not in f) and by(lambda c, f: flag in f and "big" in f), flag
    for src in ("relu", "relu6"):
        assert by(lambda c, f: source_of(c) == src and "big" not in f)
    assert all(flags_of(c) >= {"fix4", "nostats"} for c in BIG)


def test_per_channel_error_routes_small_channels_to_the_tensor_maximum():
    import torch
    ref = torch.tensor([[1.0, -2.0], [1e-4, 5e-4], [0.5, 0.25]], dtype=torch.float64)
    got = ref + torch.tensor([[1e-6, 0.0], [1e-6, 0.0], [0.0, 1e-6]], dtype=torch.float64)
    worst, low, n = per_channel(got, ref, (0,))
    assert (low, n) == (1, 3) and worst == pytest.approx(1e-6 / 0.5)      # row 1 is measured against 2.0, row 2 against 0.5
    worst, low, n = per_channel(got, ref, (0, 1))
    assert (low, n) == (2, 6) and worst == pytest.approx(1e-6 / 0.25)
