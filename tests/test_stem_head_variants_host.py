"""The GPU case tables of tests/test_gpu_stem_head_variants.py reach EVERY launch form of the stem and head kernels, and every bound
in them is tight enough to see a one-pixel mistake (no GPU).

The stem and head launchers dispatch on the host queries sc_stem_fwd_kernel, sc_stem_wgrad_njb / sc_stem_wgrad_rows, sc_head_fwd_kernel
and sc_head_bwd_bn_rows.  Here each query is swept over the shapes its entry point accepts, and the set of codes it returns must EQUAL
the set of codes of that op's case table.  Every table is also held to the list of what its rows are there for (WANT_*): deleting a
row, a dispatcher gaining a branch without a case, a row whose shape no longer selects the code written next to it, or a row that
loses the edge it is there for fails this file.  The strength test computes, for every GPU case, the float64 reference and a mutated
one (taps shifted by one column, or the last row dropped from a sum) and asserts that the mutation violates the case's bound at least
10-fold somewhere: a bound wide enough to hide that would check nothing."""
import pytest
import torch

from test_gpu_stem_head_variants import (HEAD_BWD_CASES, HEAD_DGRAD_CASES, HEAD_FWD_CASES, HEAD_WGRAD_CASES, HK_FWD16, HK_FWD16V, HK_GENERIC,
                                         K_MFMA4, K_VALU4, K_VALU8, K_VALU16, STEM_FWD_CASES, STEM_WGRAD_CASES, chain_head_bwd,
                                         chain_head_dbias, chain_head_wgrad, chain_stem_stats, chain_stem_wgrad, head_bwd_ref, head_bwd_rows,
                                         head_bwd_tiles, head_dgrad_ref, head_fwd_code, head_fwd_ref, head_wgrad_ref, out_size, reduce_levels,
                                         stem_fwd_code, stem_fwd_ref, stem_wgrad_njb, stem_wgrad_ref, stem_wgrad_rows, stem_wgrad_tiles)
from test_gpu_depthwise_variants import OP_WGRAD, dw_code, dw_tiles, wgrad_tiles_per_group

# what each row is there for: (code, Cin, source modes, flags) -- shapes are the table's business, held to the flags below
WANT_STEM_FWD = {
    (K_MFMA4, 4, "norm", ""), (K_MFMA4, 3, "affine_relu", "ragged"),
    (K_VALU4, 4, "raw", ""), (K_VALU4, 1, "norm", "ragged"), (K_VALU4, 4, "norm", "offset"), (K_VALU4, 2, "affine_relu", "tiny"),
    (K_VALU8, 8, "norm", ""), (K_VALU8, 5, "affine_relu", "ragged"), (K_VALU8, 6, "raw", ""),
    (K_VALU16, 16, "raw", ""), (K_VALU16, 13, "norm", "ragged"), (K_VALU16, 9, "affine_relu", "tiny"),
}
# (NJB, Cin, (dy mode, input mode), flags, k_reduce16 levels)
WANT_STEM_WGRAD = {
    (3, 4, ("raw", "norm"), "", 0), (3, 5, ("bnbwd6", "norm"), "", 0), (3, 1, ("bnbwd6", "raw"), "ragged", 1),
    (3, 5, ("affine", "norm"), "ragged", 0), (3, 4, ("bnbwd6", "norm"), "loop", 2),
    (5, 8, ("raw", "norm"), "", 0), (5, 6, ("bnbwd6", "norm"), "ragged", 1), (5, 8, ("affine", "raw"), "ragged", 1),
    (5, 8, ("bnbwd6", "norm"), "loop", 2),
}
WANT_HEAD_FWD = {
    (HK_GENERIC, 5, "raw", ""), (HK_GENERIC, 32, "affine_relu", "ragged"), (HK_GENERIC, 5, "affine_relu", "tiny"),
    (HK_FWD16, 16, "raw", ""), (HK_FWD16, 16, "affine_relu", "ragged"), (HK_FWD16, 16, "affine_relu", "offset_in"),
    (HK_FWD16, 16, "affine_relu", "offset_out"), (HK_FWD16, 16, "raw", "tiny"),
    (HK_FWD16V, 16, "affine_relu", ""), (HK_FWD16V, 16, "raw", "ragged"),
}
WANT_HEAD_GRAD = {(c, f) for c in (5, 16, 32) for f in ("", "ragged")}
# (BNS, (H, W), mode, flags)
WANT_HEAD_BWD = {
    (0, (32, 64), "raw", ""), (0, (3, 5), "affine_relu", "ragged"), (0, (33, 70), "affine6", "ragged"), (0, (36, 64), "raw", "ragged"),
    (0, (256, 8), "raw", "loop"),
    (1, (32, 64), "affine_relu", ""), (1, (3, 5), "affine6", "ragged"), (1, (33, 70), "affine_relu", "ragged"), (1, (36, 64), "affine6", "ragged"),
    (1, (256, 8), "affine6", "loop"),
}


def _fl(flags):
    return set(flags.split())


def _small(N, H, W):
    return N <= 3 and H <= 40 and W <= 72


def _plain_and_ragged(cases, code_of, flags_of):
    for code in {code_of(c) for c in cases}:
        mine = [c for c in cases if code_of(c) == code]
        assert any(flags_of(c) == "" for c in mine), (code, "no plain case")
        assert any("ragged" in _fl(flags_of(c)) for c in mine), (code, "no ragged case")


def test_stem_fwd_table():
    assert len(STEM_FWD_CASES) == len(WANT_STEM_FWD) and {(c[0], c[2], c[5], c[6]) for c in STEM_FWD_CASES} == WANT_STEM_FWD
    sweep = {stem_fwd_code(ci, W, al) for ci in range(1, 17) for W in range(1, 161) for al in (False, True)}
    assert sweep == {c[0] for c in STEM_FWD_CASES} == {K_MFMA4, K_VALU4, K_VALU8, K_VALU16}
    _plain_and_ragged(STEM_FWD_CASES, lambda c: c[0], lambda c: c[6])
    for code, N, Cin, H, W, mode, flags in STEM_FWD_CASES:
        fl = _fl(flags)
        assert stem_fwd_code(Cin, W, "offset" not in fl) == code and _small(N, H, W)
        if "ragged" in fl:
            assert H % 2 == 1 and out_size(H) % 8 != 0 and out_size(W) % 32 != 0 and out_size(W) > 32
            assert W % 2 == 1 or code == K_MFMA4
        if "offset" in fl:      # the same shape, aligned, takes the 16-byte form and is in the table
            assert code == K_VALU4 and stem_fwd_code(Cin, W, True) == K_MFMA4
            assert any(d[0] == K_MFMA4 and d[1:5] == (N, Cin, H, W) for d in STEM_FWD_CASES)
        if "tiny" in fl:
            assert (H, W) == (1, 3)
    # the MFMA form with a last column tile of 4 columns
    assert any(c[0] == K_MFMA4 and c[4] == 72 and "ragged" in _fl(c[6]) for c in STEM_FWD_CASES)
    # statistics rows run for every Cin <= 8 case: both VALU widths, Cin 5 and 8 among them
    assert {5, 8} <= {c[2] for c in STEM_FWD_CASES if c[0] == K_VALU8}
    assert {"raw", "norm", "affine_relu"} == {c[5] for c in STEM_FWD_CASES}
    assert stem_fwd_code(0, 64, True) < 0 and stem_fwd_code(17, 64, True) < 0


def test_stem_wgrad_table():
    got = {(c[0], c[2], c[5], c[6], reduce_levels(stem_wgrad_rows(c[1], c[3], c[4]))) for c in STEM_WGRAD_CASES}
    assert len(STEM_WGRAD_CASES) == len(WANT_STEM_WGRAD) and got == WANT_STEM_WGRAD
    assert {stem_wgrad_njb(ci) for ci in range(1, 9)} == {c[0] for c in STEM_WGRAD_CASES} == {3, 5}
    assert {c[2] for c in STEM_WGRAD_CASES if c[0] == 3} == {1, 4, 5} and {c[2] for c in STEM_WGRAD_CASES if c[0] == 5} == {6, 8}
    assert stem_wgrad_njb(0) < 0 and stem_wgrad_njb(9) < 0 and stem_wgrad_rows(0, 8, 8) < 0 and stem_wgrad_rows(1, 8, 0) < 0
    sweep = {reduce_levels(stem_wgrad_rows(N, H, W)) for N in (1, 3, 16, 33) for H in range(1, 80, 7) for W in range(1, 300, 13)}
    assert sweep == {0, 1, 2}
    _plain_and_ragged(STEM_WGRAD_CASES, lambda c: c[0], lambda c: c[6])
    for njb, N, Cin, H, W, modes, flags in STEM_WGRAD_CASES:
        fl = _fl(flags)
        rows, tiles = stem_wgrad_rows(N, H, W), stem_wgrad_tiles(N, H, W)
        assert stem_wgrad_njb(Cin) == njb and rows == min(tiles, 1024)
        if "loop" in fl:
            assert (N, H, W) == (33, 64, 256) and tiles == 1056 and rows == 1024 and reduce_levels(rows) == 2
        else:
            assert _small(N, H, W) and tiles == rows
        if "ragged" in fl:
            assert H % 2 == 1 and W % 2 == 1 and out_size(H) % 4 != 0 and out_size(W) % 32 != 0
    for njb in (3, 5):
        mine = [c for c in STEM_WGRAD_CASES if c[0] == njb]
        assert {"raw", "affine", "bnbwd6"} == {c[5][0] for c in mine} and {"raw", "norm"} == {c[5][1] for c in mine}
        assert {0, 1, 2} == {reduce_levels(stem_wgrad_rows(c[1], c[3], c[4])) for c in mine}


def test_head_fwd_table():
    assert len(HEAD_FWD_CASES) == len(WANT_HEAD_FWD) and {(c[0], c[2], c[5], c[6]) for c in HEAD_FWD_CASES} == WANT_HEAD_FWD
    sweep = {head_fwd_code(ci, W, ai, ao) for ci in range(1, 33) for W in range(1, 81) for ai in (False, True) for ao in (False, True)}
    assert sweep == {c[0] for c in HEAD_FWD_CASES} == {HK_GENERIC, HK_FWD16, HK_FWD16V}
    assert head_fwd_code(0, 64) < 0 and head_fwd_code(33, 64) < 0
    _plain_and_ragged(HEAD_FWD_CASES, lambda c: c[0], lambda c: c[6])
    for code, N, Cin, H, W, mode, flags in HEAD_FWD_CASES:
        fl = _fl(flags)
        assert head_fwd_code(Cin, W, "offset_in" not in fl, "offset_out" not in fl) == code and _small(N, H, W)
        th, tw = (8, 32) if code == HK_GENERIC else (16, 64)
        if "ragged" in fl:
            assert H % th != 0 and W % tw != 0 and H > th and W > tw
        if fl & {"offset_in", "offset_out"}:
            assert code == HK_FWD16 and head_fwd_code(Cin, W) == HK_FWD16V
            assert any(d[0] == HK_FWD16V and d[1:5] == (N, Cin, H, W) for d in HEAD_FWD_CASES)
        if "tiny" in fl:
            assert (H, W) == (1, 3)
    assert any(c[0] == HK_FWD16 and c[4] % 4 != 0 and "ragged" in _fl(c[6]) for c in HEAD_FWD_CASES)
    assert {5, 32} <= {c[2] for c in HEAD_FWD_CASES if c[0] == HK_GENERIC}
    assert all({"raw", "affine_relu"} == {c[5] for c in HEAD_FWD_CASES if c[0] == k} for k in (HK_GENERIC, HK_FWD16, HK_FWD16V))


def test_head_grad_tables():
    assert len(HEAD_DGRAD_CASES) == 6 and {(c[1], c[4]) for c in HEAD_DGRAD_CASES} == WANT_HEAD_GRAD
    small = [c for c in HEAD_WGRAD_CASES if "loop" not in _fl(c[5])]
    assert len(small) == 6 and {(c[1], c[5]) for c in small} == WANT_HEAD_GRAD and {"raw", "affine_relu"} == {c[4] for c in small}
    for c in HEAD_DGRAD_CASES + small:
        N, Cin, H, W = c[:4]
        assert _small(N, H, W)
        if "ragged" in _fl(c[-1]):
            assert H % 8 != 0 and W % 32 != 0 and H > 8 and W > 32
    for N, Cin, H, W, mode, flags in small:
        code = dw_code(OP_WGRAD, N, Cin, H, W, 1)
        assert N * dw_tiles(OP_WGRAD, code, H, W, 1) <= 4096 // Cin and wgrad_tiles_per_group(code, N, Cin, H, W, 1) == 1
    # the cap on the filter gradient's grid: more tiles than 4096 / Cin work-groups
    loops = [c for c in HEAD_WGRAD_CASES if "loop" in _fl(c[5])]
    assert len(loops) == 1 and len(HEAD_WGRAD_CASES) == 7
    N, Cin, H, W, mode, flags = loops[0]
    code = dw_code(OP_WGRAD, N, Cin, H, W, 1)
    assert N * dw_tiles(OP_WGRAD, code, H, W, 1) > 4096 // Cin and wgrad_tiles_per_group(code, N, Cin, H, W, 1) == 2


def test_head_bwd_table():
    assert len(HEAD_BWD_CASES) == len(WANT_HEAD_BWD) and {(c[0], (c[2], c[3]), c[4], c[5]) for c in HEAD_BWD_CASES} == WANT_HEAD_BWD
    _plain_and_ragged(HEAD_BWD_CASES, lambda c: c[0], lambda c: c[5])
    for bns, N, H, W, mode, flags in HEAD_BWD_CASES:
        fl = _fl(flags)
        rows, tiles = head_bwd_rows(N, H, W), head_bwd_tiles(N, H, W)
        assert rows == min(tiles, 1024)
        if "loop" in fl:
            assert (N, H, W) == (129, 256, 8) and tiles == 1032 and rows == 1024
        else:
            assert _small(N, H, W) and tiles == rows
        if "ragged" in fl:
            assert H % 32 != 0 or W % 64 != 0
        assert not bns or mode != "raw"
    for bns in (0, 1):
        mine = [c for c in HEAD_BWD_CASES if c[0] == bns]
        assert {(3, 5), (33, 70), (36, 64)} <= {(c[2], c[3]) for c in mine}
        assert {"affine_relu", "affine6"} <= {c[4] for c in mine}
    assert any(c[4] == "raw" for c in HEAD_BWD_CASES)


def test_chain_counts():
    """the fp32 chain lengths the GPU bounds use, written out for the cases that matter"""
    assert chain_stem_wgrad(1, 16, 64) == 32 + 3 + 16 + 3 and chain_stem_wgrad(2, 37, 71) == 32 + 3 + 32 + 3
    assert chain_stem_wgrad(33, 64, 256) == 64 + 3 + 48 + 3
    assert chain_stem_stats(K_MFMA4) == 10 and chain_stem_stats(K_VALU8) == 13
    assert chain_head_bwd(2, 32, 64) == 32 + 6 and chain_head_bwd(1, 3, 5) == 3 + 6 and chain_head_bwd(129, 256, 8) == 64 + 6
    assert chain_head_wgrad(65, 32, 32, 16) == chain_head_wgrad(1, 32, 32, 16) + 1
    assert chain_head_dbias(1, 3, 5) == 1 + 10 and chain_head_dbias(2, 32, 64) == 16 + 10 and chain_head_dbias(129, 256, 8) == 16 + 10


STRENGTH = ([(stem_fwd_ref, c) for c in STEM_FWD_CASES] + [(stem_wgrad_ref, c) for c in STEM_WGRAD_CASES]
            + [(head_fwd_ref, c) for c in HEAD_FWD_CASES] + [(head_dgrad_ref, c) for c in HEAD_DGRAD_CASES]
            + [(head_wgrad_ref, c) for c in HEAD_WGRAD_CASES] + [(head_bwd_ref, c) for c in HEAD_BWD_CASES])


@pytest.mark.parametrize("ref_of,case", STRENGTH, ids=lambda v: v.__name__ if callable(v) else "-".join(map(str, v)).replace(" ", "+"))
def test_bounds_see_a_one_pixel_mistake(ref_of, case):
    """every compared output of every GPU case: the mutated reference lies outside the bound by a factor of 10 somewhere"""
    _, checks = ref_of(case)
    assert checks
    for name, (ref, bound, mutated) in checks.items():
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), name
        if mutated is None:
            assert name == "absmax"          # a relative bound of 2 u: nothing to show
            continue
        err = (mutated - ref).abs()
        pos = bound > 0
        assert bool(pos.any()), name
        ratio = float((err[pos] / bound[pos]).max())
        print(f"STRENGTH {ref_of.__name__} {case} {name} {ratio:.3g}")
        assert ratio >= 10, (name, ratio)
