"""The GPU case tables of tests/test_gpu_sp_variants.py reach EVERY kernel variant the sub-pixel decoder launchers can select (no GPU).

sc_conv3x3_sp, sc_conv3x3_sp_dgrad and sc_conv3x3_sp_wgrad switch on the functions behind the host-only queries sc_sp_variant,
sc_spd_variant and sc_sp_wgrad_variant.  Here each query is swept over the arguments its entry point accepts, and the set of codes it
returns must EQUAL the set of codes of that op's case table and a literal WANT set: deleting a case, or a launcher gaining a branch
without a case, fails this test; so does a table entry whose arguments no longer select the code written next to it, and a table that
loses one of the edges or features it is there for."""
import os

import pytest

from test_gpu_sp_variants import (CAPS, CASES, KNOBS, OP_SP, OP_SPD, OP_SPW, XB_MAX, act_scale, case_args, case_code, channel_tiles,
                                  dgrad_probe_plan, flags_of, fwd_probe_plans, query, sp_args, spd_args, spw_args, spw_plan, tile_of,
                                  wgrad_probe_plans, work_groups2)
from starcop_amd import _lib

OPS = (OP_SP, OP_SPD, OP_SPW)
WANT = {
    OP_SP: {100 * tw + 10 * npp + m for tw in (1, 2) for npp in (1, 2) for m in (1, 4)},
    OP_SPD: {1000 * mode + 100 * tw + 10 * npp + m for mode in (0, 1, 2) for tw in (1, 2) for npp in (1, 2) for m in (1, 4)},
    OP_SPW: {1, 2},
}
NWANT = {OP_SP: 8, OP_SPD: 24, OP_SPW: 2}
PROBES = {OP_SP: ("fprobe", "aprobe"), OP_SPD: ("fprobe", "aprobe"), OP_SPW: ("wprobe", "xprobe")}


@pytest.fixture(scope="module", autouse=True)
def _no_dispatch_knobs():
    """STARCOP_SP_NPP changes what the queries answer (that is its meaning): the tables describe the default dispatch"""
    for k in KNOBS:
        if k in os.environ:
            pytest.fail(f"{k} is set: the case tables cover the default dispatch")


def _sweep_sp():
    got = set()
    for terms in (0, 1, 2, 3, 4):
        for srcs in ("raw", "affine", "affine+raw", "raw+affine", "bnbwd"):
            for N, H, W in ((1, 8, 32), (2, 16, 64), (3, 20, 36), (3, 20, 68), (3, 48, 192), (3, 148, 36), (2, 16, 33), (2, 15, 32)):
                for cout in (1, 32, 40, 136, 160):
                    got.add(query(OP_SP, sp_args(N, (16, 13), cout, H, W, srcs, set(), terms)))
    return got


def _sweep_spd():
    got = set()
    for terms in (0, 1, 2, 3, 4):
        for mode in ("bnbwd", "raw"):
            for N, H, W in ((1, 8, 32), (2, 16, 64), (3, 20, 36), (3, 172, 196), (3, 692, 36), (3, 88, 68), (3, 180, 36), (2, 16, 33), (2, 15, 32)):
                for chans in ((32, 0), (40, 0), (64, 16), (65, 16), (64, 17), (32, 32), (40, 70), (32, 96), (300, 8)):
                    got.add(query(OP_SPD, spd_args(N, chans, 13, H, W, mode, set(), terms)))
    return got


def _sweep_spw():
    got = set()
    for terms in (0, 1, 3, 4):
        for dym in ("raw", "affine", "bnbwd"):
            for xm in ("raw", "affine", "bnbwd"):
                for cup in (1, 40, 64, 65, 128, 136, 300):
                    for H, W in ((16, 64), (30, 100), (15, 64)):
                        got.add(query(OP_SPW, spw_args(2, (cup, 8), 13, H, W, (dym, xm), set(), terms)))
    return got


SWEEP = {OP_SP: _sweep_sp, OP_SPD: _sweep_spd, OP_SPW: _sweep_spw}


@pytest.mark.parametrize("op", OPS)
def test_case_table_reaches_every_variant(op):
    cases = CASES[op]
    for case in cases:
        assert case_code(op, case) == case[0], case
    got = SWEEP[op]()
    assert -1 in got, "the sweep also passes arguments the entry point rejects"
    got.discard(-1)
    assert got == {c[0] for c in cases} == WANT[op]
    assert len(WANT[op]) == NWANT[op]


@pytest.mark.parametrize("op", OPS)
def test_cases_stay_within_the_size_caps(op):
    assert CAPS == dict(N=3, pixels=4096, C=160, wgs_big=160)
    for case in CASES[op]:
        code, N, (ca, cb), Cc, H, W, _, _ = case
        fl = flags_of(case)
        assert N <= CAPS["N"] and ca + cb <= CAPS["C"], case
        if "big" in fl:      # just past the 128 work-groups of the NPP rule, by no more than a quarter
            assert op != OP_SPW and (code // 10) % 10 == 2 and 128 < work_groups2(op, case) <= CAPS["wgs_big"], (case, work_groups2(op, case))
            assert ca + cb <= 136 and (op == OP_SPD or ca + cb <= 32), case
        else:
            assert N * (H // 2) * (W // 2) <= CAPS["pixels"] and Cc <= CAPS["C"], case
            assert op == OP_SPW or ((code // 10) % 10 == 1 and work_groups2(op, case) <= 128), case
    if op != OP_SPW:
        assert all(("big" in flags_of(c)) == ((c[0] // 10) % 10 == 2) for c in CASES[op])


def _is_plain(op, case):
    code, N, (ca, cb), Cc, H, W, _, _ = case
    Hl, Wl = H // 2, W // 2
    if op == OP_SPW:
        K, Kp, cbk, mt, nt, kst, nsl = spw_plan(N, H, W, Cc, ca)
        return K == Kp and (Kp // 32) % kst == 0 and ca % (64 * cbk) == 0 and Cc % 32 == 0
    th, tw = tile_of(code)
    if op == OP_SP:
        return Hl % th == 0 and Wl % tw == 0 and ca % 16 == 0 and cb % 16 == 0 and Cc % 32 == 0
    return Hl % th == 0 and Wl % tw == 0 and Cc % 16 == 0 and (ca % 128 == 0 or ca % 32 == 0) and cb % 16 == 0


def _is_ragged(op, case):
    code, N, (ca, cb), Cc, H, W, _, _ = case
    Hl, Wl = H // 2, W // 2
    if op == OP_SPW:      # a zero tail, a shorter last K slice, rows and columns off the 256 x 64 CB tile, skip columns to leave alone
        K, Kp, cbk, mt, nt, kst, nsl = spw_plan(N, H, W, Cc, ca)
        return K % 32 != 0 and nsl > 1 and (Kp // 32) % kst != 0 and (9 * Cc) % 256 != 0 and (ca % (64 * cbk) != 0 or ca in (64, 65)) and cb > 0
    th, tw = tile_of(code)
    edge = 1 <= Wl % tw <= 2 and Hl % th != 0 and Hl > th and (N * -(-Wl // tw) * -(-Hl // th)) % 8 != 0
    if op == OP_SP:
        return edge and ca % 8 != 0 and cb % 8 != 0 and Cc % 32 != 0
    mode = code // 1000
    return edge and Cc % 8 != 0 and ca % 128 != 0 and (mode == 0 or (cb % 16 != 0 and cb % 32 != 0))


@pytest.mark.parametrize("op", OPS)
def test_every_variant_has_a_plain_a_ragged_case_and_probes(op):
    cases = CASES[op]
    for code in sorted(WANT[op]):
        mine = [c for c in cases if c[0] == code]
        rand = [c for c in mine if not flags_of(c) & set(PROBES[op])]
        assert any(_is_plain(op, c) and "ragged" not in flags_of(c) for c in rand), (op, code, "no plain case")
        assert any("ragged" in flags_of(c) for c in rand), (op, code, "no ragged case")
        for c in mine:
            assert ("ragged" in flags_of(c)) <= _is_ragged(op, c), (c, "flagged ragged, but is not")
        for p in PROBES[op]:      # each kind of probe, at a ragged shape
            assert any(p in flags_of(c) and "ragged" in flags_of(c) for c in mine), (op, code, p)


def _has(cases, code, pred):
    return any(pred(c, flags_of(c)) for c in cases if c[0] == code)


def test_required_features_are_on_every_code_that_accepts_them():
    sp = CASES[OP_SP]
    for code in sorted(WANT[OP_SP]):
        assert _has(sp, code, lambda c, f: "stats" in f), code
        assert _has(sp, code, lambda c, f: c[6].startswith("affine") and c[2][1] > 0), code       # AFFINE + ReLU, with a skip source
        assert _has(sp, code, lambda c, f: c[6].startswith("raw+") and c[2][1] > 0 and not f & {"fprobe", "aprobe", "xbound"}), code
        assert _has(sp, code, lambda c, f: c[2][1] == 0 and c[6] == "affine"), code                # without a skip source: AFFINE + ReLU
        assert _has(sp, code, lambda c, f: c[2][1] == 0 and c[6] == "raw"), code                   # ... and RAW
        assert _has(sp, code, lambda c, f: c[6].endswith("+affine")), code                         # an AFFINE skip source
        assert _has(sp, code, lambda c, f: "batched" in f) and _has(sp, code, lambda c, f: "batched" not in f), code
        assert _has(sp, code, lambda c, f: "xbound" in f and c[6] == "raw+raw"), code
    assert act_scale(XB_MAX) == 1.0 and act_scale(16376.0) == 2.0 and act_scale(16377.0) == 1.0
    spd = CASES[OP_SPD]
    for code in sorted(WANT[OP_SPD]):
        mode, m = code // 1000, code % 10
        assert {c[6] for c in spd if c[0] == code} >= {"bnbwd", "bnbwd6"}, code
        assert _has(spd, code, lambda c, f: "accum" in f), code                                    # accum0, and accum1 with a skip output
        assert all((c[2][1] > 0) == (mode > 0) for c in spd if c[0] == code), code
        assert _has(spd, code, lambda c, f: "batched" in f) and _has(spd, code, lambda c, f: "batched" not in f), code
        if m == 4:
            assert _has(spd, code, lambda c, f: "g3e-8" in f) and _has(spd, code, lambda c, f: "g2e4" in f), code
            assert _has(spd, code, lambda c, f: not f & {"g3e-8", "g2e4", "fprobe", "aprobe"}), code
    spw = CASES[OP_SPW]
    for code in sorted(WANT[OP_SPW]):
        assert {c[6][0] for c in spw if c[0] == code} >= {"bnbwd", "bnbwd6", "raw", "affine"}, code
        assert {c[6][1] for c in spw if c[0] == code} >= {"raw", "affine"}, code
        assert _has(spw, code, lambda c, f: "g3e-8" in f) and _has(spw, code, lambda c, f: "g2e4" in f), code
        assert _has(spw, code, lambda c, f: not f & {"g3e-8", "g2e4", "wprobe", "xprobe"}), code
        assert _has(spw, code, lambda c, f: c[2][1] > 0), code
        assert _has(spw, code, lambda c, f: c[2][0] == (64 if code == 1 else 65)), code            # the CB threshold itself
        assert _has(spw, code, lambda c, f: c[2][0] % 64 != 0) and (code == 1 or _has(spw, code, lambda c, f: c[2][0] > 128 and c[2][0] % 128 != 0)), code


def test_probe_impulses_cover_the_borders_the_seams_and_every_channel():
    def lo_ok(plan, Hl, Wl, th, tw):
        ys, xs = {p[1] for p in plan}, {p[2] for p in plan}
        return {0, Hl - 1, th - 1, th} <= ys and {0, Wl - 1, tw - 1, tw} <= xs

    def hi_ok(plan, Hl, Wl, th, tw):
        ys, xs = {p[1] for p in plan}, {p[2] for p in plan}
        if not ({0, 2 * Hl - 1} <= ys and {0, 2 * Wl - 1} <= xs):
            return False
        for qy in (0, 1):      # every parity on both sides of the doubled seam
            for qx in (0, 1):
                par = [(y // 2, x // 2) for _, y, x in plan if y % 2 == qy and x % 2 == qx]
                rows, cols = {i for i, _ in par}, {j for _, j in par}
                if not ({th - 1, th} <= rows and {tw - 1, tw} <= cols):      # the row seam and the column seam, separately
                    return False
        return True

    for case in CASES[OP_SP]:
        if "fprobe" in flags_of(case):
            code, N, (C0, C1), _, H, W = case[:6]
            lo, hi = fwd_probe_plans(case)
            assert len(lo) == C0 and len(hi) == C1, case                                            # one impulse in every input channel
            assert len({(n, "lo", y, x) for n, y, x in lo} | {(n, "hi", y, x) for n, y, x in hi}) == C0 + C1
            assert lo_ok(lo, H // 2, W // 2, *tile_of(code)) and hi_ok(hi, H // 2, W // 2, *tile_of(code)), case
            assert all(0 <= n < N and 0 <= y < H // 2 and 0 <= x < W // 2 for n, y, x in lo) and all(0 <= n < N and 0 <= y < H and 0 <= x < W for n, y, x in hi)
    for case in CASES[OP_SPD]:
        if "fprobe" in flags_of(case):
            code, N, _, Co, H, W = case[:6]
            hi = dgrad_probe_plan(case)
            assert len(hi) == Co and hi_ok(hi, H // 2, W // 2, *tile_of(code)), case
            assert all(0 <= n < N and 0 <= y < H and 0 <= x < W for n, y, x in hi)
    for case in CASES[OP_SPW]:
        _, N, (Cup, _), Cout, H, W = case[:6]
        hi, lo = wgrad_probe_plans(case)
        if "wprobe" in flags_of(case):
            assert len(hi) == Cout and hi_ok(hi, H // 2, W // 2, 8, 32), case
        if "xprobe" in flags_of(case):
            assert len(lo) == Cup and lo_ok(lo, H // 2, W // 2, 8, 32), case


def test_footprints_of_one_image_are_disjoint():
    from test_gpu_sp_variants import _cells
    for op, plans in ((OP_SP, fwd_probe_plans), (OP_SPD, lambda c: ([], dgrad_probe_plan(c)))):
        for case in CASES[op]:
            if "fprobe" not in flags_of(case):
                continue
            lo, hi = plans(case)
            for n in range(case[1]):
                r = [_cells("lo", y, x) for i, y, x in lo if i == n] + [_cells("hi", y, x) for i, y, x in hi if i == n]
                assert all(a[1] < b[0] or b[1] < a[0] or a[3] < b[2] or b[3] < a[2] for i, a in enumerate(r) for b in r[:i]), case


def test_rejected_arguments():
    def sp(**kw):
        a = sp_args(2, (16, 16), 32, 16, 64, "affine+raw", set(), 4)
        for k, v in kw.items():
            setattr(a, k, v)
        return query(OP_SP, a)
    assert sp() == 214
    for field, bad in (("ks", 1), ("terms", 0), ("terms", 2), ("terms", 3), ("N", 0), ("H", 15), ("W", 63), ("csplit", 16), ("nsrc", 3), ("accum0", 1), ("down0", 1)):
        assert sp(**{field: bad}) == -1, field
    assert sp(terms=1) == 211
    assert query(OP_SP, sp_args(2, (16, 16), 32, 16, 64, "bnbwd+raw", set(), 4)) == -1              # RAW or AFFINE sources only

    def spd(chans=(32, 16), **kw):
        a = spd_args(2, chans, 16, 16, 64, "bnbwd", set(), 4)
        for k, v in kw.items():
            setattr(a, k, v)
        return query(OP_SPD, a)
    assert spd() == 1214 and spd(terms=1) == 1211 and spd((32, 0)) == 214
    for field, bad in (("ks", 1), ("terms", 0), ("terms", 2), ("terms", 3), ("N", 0), ("H", 15), ("W", 63), ("csplit", 0), ("nsrc", 2), ("out1", None), ("stats", 0x10000)):
        assert spd(**{field: bad}) == -1, field
    assert query(OP_SPD, spd_args(2, (32, 16), 16, 16, 64, "raw", set(), 4)) == -1                   # the source is the BNBWD operand

    def spw(**kw):
        a = spw_args(2, (64, 8), 13, 16, 64, ("bnbwd", "affine"), set(), 4)
        for k, v in kw.items():
            setattr(a, k, v)
        return query(OP_SPW, a)
    assert spw() == 1
    for field, bad in (("ks", 1), ("terms", 1), ("terms", 0), ("terms", 3), ("N", 0), ("H", 15), ("W", 63), ("Cin", 63), ("nsrc", 2), ("Cout", 12)):
        assert spw(**{field: bad}) == -1, field
    assert query(OP_SPW, spw_args(2, (64, 8), 13, 16, 64, ("bnbwd", "bnbwd"), set(), 4)) == -1


def test_dispatch_thresholds():
    """the thresholds of the dispatch rules, one step either side"""
    def sp(N, H, W, cout, terms=4):
        return query(OP_SP, sp_args(N, (16, 0), cout, H, W, "raw", set(), terms))
    # 128 | 129 work-groups: 1 x (8 x 1 tiles of 8 x 32) x 16 output tiles = 128; 43 x 3 = 129
    assert sp(1, 128, 64, 512) == 214 and sp(1, 128, 64, 513) == 224
    assert sp(1, 16 * 43, 64, 96) == 224 and sp(1, 16 * 43, 64, 64) == 214 and sp(1, 16 * 43 - 16, 64, 96) == 214
    assert sp(1, 128, 32, 1024) == 114 and sp(1, 128, 32, 1025) == 124                              # 16 x 16 tiles: 4 x 32 = 128
    assert sp(2, 16, 62, 32) == 114 and sp(2, 16, 64, 32) == 214                                    # Wl 31 | 32

    def spd(N, H, W, chans, terms=4):
        return query(OP_SPD, spd_args(N, chans, 16, H, W, "bnbwd", set(), terms))
    # ntu enters the count: 65 pixel tiles x 1 = 65, x 2 = 130; 64 x 2 = 128
    assert spd(1, 16 * 65, 64, (128, 0)) == 214 and spd(1, 16 * 65, 64, (129, 0)) == 224 and spd(1, 16 * 64, 64, (129, 0)) == 214
    # vskip: one channel tile, 2 x 64 = 128 | 3 x 43 = 129
    assert spd(2, 16 * 64, 64, (64, 16)) == 1214 and spd(3, 16 * 43, 64, (64, 16)) == 1224 and spd(1, 16 * 43, 64, (64, 16)) == 1214
    # skip tiles enter the count: ntu + nts = 1 + 3 = 4 -> 32 pixel tiles = 128, 33 = 132; without them 33 tiles stay at NPP = 1
    assert spd(1, 16 * 32, 64, (32, 96)) == 2214 and spd(1, 16 * 33, 64, (32, 96)) == 2224 and spd(1, 16 * 33, 64, (32, 0)) == 214
    assert spd(1, 16 * 43, 64, (32, 64)) == 2224 and spd(1, 16 * 43, 64, (32, 33)) == 2224 and spd(1, 16 * 42, 64, (32, 64)) == 2214
    # the vskip limits: Cup 64 | 65, Cskip 16 | 17
    assert spd(2, 16, 64, (64, 16)) == 1214 and spd(2, 16, 64, (65, 16)) == 2214 and spd(2, 16, 64, (64, 17)) == 2214
    lib = _lib.load()
    assert lib.sc_spd_vskip_ok(64, 16) == 1 and lib.sc_spd_vskip_ok(65, 16) == 0 and lib.sc_spd_vskip_ok(64, 17) == 0
    assert spd(2, 16, 62, (32, 0)) == 114 and spd(2, 16, 64, (32, 0)) == 214                        # Wl 31 | 32

    def spw(cup):
        return query(OP_SPW, spw_args(2, (cup, 0), 13, 16, 64, ("raw", "raw"), set(), 4))
    assert spw(64) == 1 and spw(65) == 2 and spw(1) == 1 and spw(300) == 2
    assert spw_plan(3, 30, 100, 13, 40) == (2250, 2272, 1, 1, 1, 2, 36)                             # 71 stages: 35 slices of 2 and one of 1


def test_stat_rows_agree_with_the_queried_tile():
    lib = _lib.load()
    shapes = [(c[1], c[4], c[5], c[3]) for c in CASES[OP_SP]] + [(1, 128, 64, 512), (1, 128, 64, 513), (1, 128, 32, 1024), (1, 128, 32, 1025),
                                                                 (1, 688, 64, 96), (1, 672, 64, 96), (5, 14, 30, 7)]
    for N, H, W, cout in shapes:
        code = query(OP_SP, sp_args(N, (16, 0), cout, H, W, "raw", set(), 4))
        th, tw = tile_of(code)
        assert lib.sc_sp_stat_rows(N, H, W, cout) == N * -(-(H // 2) // th) * -(-(W // 2) // tw), (N, H, W, cout, code)


def test_helpers_mirror_the_library():
    """channel_tiles / work_groups2 (the host arithmetic of the size caps) against the NPP the queries report"""
    for op in (OP_SP, OP_SPD):
        for case in CASES[op]:
            assert ((case[0] // 10) % 10 == 2) == (work_groups2(op, case) > 128), case
            assert channel_tiles(op, case) >= 1
            assert query(op, case_args(op, case)) == case[0]
