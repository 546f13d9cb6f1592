"""The GPU case tables of tests/test_gpu_conv3_variants.py reach EVERY kernel variant the 3x3 matrix-core launchers can select (no GPU).

sc_conv3x3_bx3, sc_conv3x3_thin16, sc_conv3x3_wgrad_bx3 and sc_conv3x3_wgrad_thin16 switch on the functions behind the host-only queries
sc_conv3_variant, sc_thin16_variant, sc_wgrad3_variant and sc_wgrad_thin16_variant.  Here each query is swept over the arguments its
entry point accepts, and the set of codes it returns must EQUAL the set of codes of that op's case table and a literal WANT set:
deleting a case, or a launcher gaining a branch without a case, fails this test; so does a table entry whose arguments no longer select
the code written next to it, and a table that loses one of the edges or features it is there for."""
import os

import pytest

from test_gpu_conv3_variants import (CAPS, CASES, KNOBS, OP_CONV3, OP_THIN, OP_WGRAD3, OP_WTHIN, WIDE_AREA, _impulses, case_code, co_t_of,
                                     conv_args, flags_of, parse_src, positions, query, terms_of, tile_h, tile_w, wgrad3_plan, wgrad_args)

OPS = (OP_CONV3, OP_THIN, OP_WGRAD3, OP_WTHIN)
WANT = {
    OP_CONV3: {1000 * ws + 100 * q + 10 * b + m for ws in (0, 1) for q in (1, 2) for b in (0, 1) for m in (1, 2, 3, 4) if m == 4 or not ws},
    OP_THIN: {100, 110, 200, 210, 1200, 2110},      # (200: 32 channels, not up-sampled; up-sampled RAW / AFFINE: 1200)
    OP_WGRAD3: {1000 * m + 100 * wm + 10 * nci for m in (1, 2, 3, 4) for wm in (1, 2) for nci in (1, 2)} | {14111, 14121, 14210, 14221, 14131},
    OP_WTHIN: {100, 110, 200, 210},
}
NWANT = {OP_CONV3: 20, OP_THIN: 6, OP_WGRAD3: 21, OP_WTHIN: 4}
CHANNELS = (8, 12, 16, 17, 24, 32, 33, 48, 64, 65, 80, 96, 97, 128, 160, 240, 241, 256, 257, 288)


@pytest.fixture(scope="module", autouse=True)
def _no_dispatch_knobs():
    """the development knobs change what the queries answer (that is their meaning): the tables describe the default dispatch"""
    for k in KNOBS:
        if k in os.environ:
            pytest.fail(f"{k} is set: the case tables cover the default dispatch")


def _sweep_conv3():
    got = set()
    for co_t in (32, 64):
        for terms in (0, 1, 2, 3, 4):
            for srcs in ("raw", "affine", "bnbwd", "up:affine", "up:affine+raw", "raw+raw", "up:bnbwd"):
                for fl in ((), ("bnr",), ("down0",)):
                    for k in CHANNELS:
                        two = srcs.endswith("+raw")
                        chans = (k // 16 * 16, 8) if two else (k, 0)
                        for W in (34, 35):
                            got.add(query(OP_CONV3, conv_args(OP_CONV3, 1, chans, 40, 12, W, srcs, set(fl), co_t, terms)))
    return got


def _sweep_thin():
    got = set()
    for srcs in ("raw", "affine", "bnbwd", "up:raw", "up:affine", "up:bnbwd"):
        for fl in ((), ("bnr",), ("down0",), ("stats",)):
            for k in CHANNELS:
                for cout in (1, 9, 16, 17, 32):
                    for W in (34, 35):
                        got.add(query(OP_THIN, conv_args(OP_THIN, 1, (k, 0), cout, 12, W, srcs, set(fl), 16, 4)))
    return got


def _sweep_wgrad(op):
    got = set()
    for terms in (0, 1, 2, 3, 4):
        for dym in ("raw", "affine", "bnbwd"):
            for xs in ("raw", "affine", "up:affine", "up:affine+raw"):
                for fl in ((), ("offset",)):
                    for ci in CHANNELS:
                        chans = (ci - 8, 8) if xs.endswith("+raw") and ci > 8 else (ci, 0)
                        if xs.endswith("+raw") and ci <= 8:
                            continue
                        for co in (CHANNELS if op == OP_WGRAD3 else (1, 9, 16, 17)):
                            for W in (34, 35):
                                got.add(query(op, wgrad_args(1, chans, co, 12, W, (dym, xs), set(fl), terms)))
    return got


SWEEP = {OP_CONV3: _sweep_conv3, OP_THIN: _sweep_thin, OP_WGRAD3: lambda: _sweep_wgrad(OP_WGRAD3), OP_WTHIN: lambda: _sweep_wgrad(OP_WTHIN)}


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
    for case in CASES[op]:
        code, N, (C0, C1), Cout, H, W, srcs, _ = case
        fl = flags_of(case)
        if "wide" in fl:
            assert op == OP_CONV3 and code >= 1000 and H * W <= WIDE_AREA and C0 + C1 >= 241 and Cout <= CAPS["C"], case
            assert N <= CAPS["N"] or "fprobe" in fl, case      # (an impulse per channel: 250 footprints need more images)
            if (code // 10) % 10:
                assert C0 <= 256, case
        else:
            assert N <= CAPS["N"] and H <= CAPS["H"] and W <= CAPS["W"] and C0 + C1 <= CAPS["C"] and Cout <= CAPS["C"], case
    assert all(c[0] >= 1000 for c in CASES[OP_CONV3] if "wide" in flags_of(c))
    assert all("wide" in flags_of(c) for c in CASES[OP_CONV3] if c[0] >= 1000)


def _is_plain(op, case):
    code, N, (C0, C1), Cout, H, W, srcs, _ = case
    if op in (OP_CONV3, OP_THIN):
        return H % 8 == 0 and W % tile_w(op, code) == 0 and (C0 + C1) % 16 == 0 and Cout % co_t_of(op, code) == 0
    if op == OP_WTHIN:
        return H % 4 == 0 and W % 32 == 0 and Cout == 16
    nsl, T = wgrad3_plan(N, H, W, Cout, C0 + C1, code // 10000 == 1)[3:]
    return T % nsl == 0 and H % 2 == 0 and Cout % 32 == 0 and (C0 + C1) % 32 == 0


def _is_ragged(op, case):
    code, N, (C0, C1), Cout, H, W, srcs, _ = case
    tw = tile_w(op, code)
    tiles = -(-W // tw) * -(-H // tile_h(op))
    if op == OP_CONV3:
        return 1 <= W % tw <= 4 and H % 8 != 0 and (C0 + C1) % 16 != 0 and Cout % co_t_of(op, code) != 0 and (N * tiles) % 8 != 0
    if op == OP_THIN:      # (the channel counts of the thin kernels are fixed: 16 or 32 sources; the down0 kernel writes 32 outputs)
        return 1 <= W % tw <= 4 and H % 8 != 0 and (Cout % 16 != 0 or code == 2110 or "bnr" in flags_of(case)) and (N * tiles) % 8 != 0
    if op == OP_WTHIN:
        return W % 32 != 0 and H % 4 != 0 and Cout < 16
    nsl, T = wgrad3_plan(N, H, W, Cout, C0 + C1, code // 10000 == 1)[3:]
    return nsl > 1 and T % nsl != 0 and H % 2 == 1 and Cout % 32 != 0 and (C0 + C1) % 32 != 0


@pytest.mark.parametrize("op", OPS)
def test_every_variant_has_a_plain_a_ragged_case_and_probes(op):
    cases = CASES[op]
    probes = ("fprobe", "aprobe") if op in (OP_CONV3, OP_THIN) else ("wprobe", "xprobe")
    for code in sorted(WANT[op]):
        mine = [c for c in cases if c[0] == code]
        rand = [c for c in mine if not flags_of(c) & set(probes)]
        assert any(_is_plain(op, c) and "ragged" not in flags_of(c) for c in rand), (op, code, "no plain case")
        ragged = [c for c in rand if "ragged" in flags_of(c)]
        assert ragged, (op, code, "no ragged case")
        for c in mine:
            assert ("ragged" in flags_of(c)) <= _is_ragged(op, c), (c, "flagged ragged, but is not")
        for p in probes:      # each kind of probe, at a ragged shape
            assert any(p in flags_of(c) and "ragged" in flags_of(c) for c in mine), (op, code, p)
    if op == OP_CONV3:      # a channel count that is no multiple of 8, on every code
        for code in sorted(WANT[op]):
            assert any((c[2][0] + c[2][1]) % 8 != 0 for c in cases if c[0] == code and "ragged" in flags_of(c)), code


def _has(cases, code, pred):
    return any(pred(c, flags_of(c)) for c in cases if c[0] == code)


def test_required_features_are_on_every_code_that_accepts_them():
    # forward and data gradient
    for code in sorted(WANT[OP_CONV3]):
        cs = CASES[OP_CONV3]
        m, bnb, ws = code % 10, (code // 10) % 10, code // 1000
        if not bnb:
            assert _has(cs, code, lambda c, f: "stats" in f), code
            assert _has(cs, code, lambda c, f: c[6] == "up:affine+raw" and c[2][0] % 16 == 0 and c[2][1] > 0), code
            assert _has(cs, code, lambda c, f: c[6] == "up:affine" and c[2][1] == 0), code
        else:
            assert _has(cs, code, lambda c, f: "add" in f), code                              # add0 + accum0
            assert _has(cs, code, lambda c, f: "csplit" in f), code
            assert _has(cs, code, lambda c, f: "down0" in f), code
            assert ws or _has(cs, code, lambda c, f: "bnr" in f), code                        # (bnr launches never take k_conv3_ws)
            assert {c[6] for c in cs if c[0] == code} >= {"bnbwd", "bnbwd6"}, code            # ReLU and ReLU6 masks
            if m == 4:
                assert _has(cs, code, lambda c, f: "g3e-8" in f) and _has(cs, code, lambda c, f: "g2e4" in f), code
                assert _has(cs, code, lambda c, f: not f & {"g3e-8", "g2e4", "fprobe", "aprobe"}), code
    th = CASES[OP_THIN]
    for code in (100, 200, 1200):
        assert _has(th, code, lambda c, f: "stats" in f), code
    for code in (110, 210):
        assert _has(th, code, lambda c, f: "bnr" in f), code
    for code in (100, 1200):
        assert _has(th, code, lambda c, f: c[6].startswith("up:")), code
    for code in (110, 210, 2110):
        assert _has(th, code, lambda c, f: "g3e-8" in f) and _has(th, code, lambda c, f: "g2e4" in f), code
        assert {c[6] for c in th if c[0] == code} >= {"bnbwd", "bnbwd6"}, code
    assert _has(th, 2110, lambda c, f: "accum" in f)
    # weight gradients
    wg = CASES[OP_WGRAD3]
    for code in sorted(WANT[OP_WGRAD3]):
        pipe, m = code // 10000, (code // 1000) % 10
        assert _has(wg, code, lambda c, f: c[6][1] == "up:affine+raw"), code
        dys = {c[6][0] for c in wg if c[0] == code}
        assert dys >= {"bnbwd", "bnbwd6"}, code
        if not pipe:
            assert dys >= {"raw", "affine"}, code
        if m == 4:
            assert _has(wg, code, lambda c, f: "g3e-8" in f) and _has(wg, code, lambda c, f: "g2e4" in f), code
        if m == 4 and not pipe:      # each way out of the pipeline in a case of its own
            odd = [c for c in wg if c[0] == code and "oddw" in flags_of(c)]
            off = [c for c in wg if c[0] == code and "offset" in flags_of(c)]
            assert odd and all(c[5] % 2 == 1 and c[6][0].startswith("bnbwd") and "offset" not in flags_of(c) for c in odd), code
            assert off and all(c[5] % 2 == 0 and c[6][0].startswith("bnbwd") for c in off), code
            for c in odd + off:      # ... and the same arguments without it take the pipelined kernel
                a = wgrad_args(c[1], c[2], c[3], c[4], c[5] + ("oddw" in flags_of(c)), c[6], set(), 4)
                assert query(OP_WGRAD3, a) // 10000 == 1, c
    wt = CASES[OP_WTHIN]
    for code in sorted(WANT[OP_WTHIN]):
        assert _has(wt, code, lambda c, f: c[6][1] == "up:affine"), code
        assert _has(wt, code, lambda c, f: "g3e-8" in f) and _has(wt, code, lambda c, f: "g2e4" in f), code
        dys = {c[6][0] for c in wt if c[0] == code}
        assert dys >= ({"bnbwd", "bnbwd6"} if (code // 10) % 10 else {"raw", "affine"}), code


def test_probe_impulses_cover_the_borders_the_seams_and_every_channel():
    for op in (OP_CONV3, OP_THIN):
        for case in CASES[op]:
            code, N, (C0, C1), Cout, H, W, srcs, _ = case
            if "fprobe" not in flags_of(case):
                continue
            up = parse_src(srcs)[0]
            tw = tile_w(op, code) // 2 if up else tile_w(op, code)
            th = 4 if up else 8
            x = _impulses(N, C0 + C1, H >> up, W >> up, tw, th)
            assert float(x.sum()) == C0 + C1 and bool((x.sum((0, 2, 3)) == 1).all()), case       # one impulse in every input channel
            hit = x.sum(1)                                                                        # [N, H, W]
            assert float(hit.max()) == 1.0
            rows, cols = hit.sum((0, 2)) > 0, hit.sum((0, 1)) > 0
            assert bool(rows[0]) and bool(rows[-1]) and bool(cols[0]) and bool(cols[-1]), case
            assert bool(cols[tw - 1]) and bool(cols[tw]) and bool(rows[th - 1]) and bool(rows[th]), case
    for H, W, tw in ((12, 34, 32), (13, 34, 32), (10, 34, 32), (12, 66, 64), (6, 33, 32)):
        for image in (0, 1, 2):
            pos = positions(H, W, tw, image)
            assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 3 for i, a in enumerate(pos) for b in pos[:i]), (H, W)


def test_rejected_arguments():
    ok = conv_args(OP_CONV3, 1, (32, 0), 32, 8, 32, "affine", set(), 32, 3)
    assert query(OP_CONV3, ok) == 103
    for field, bad in (("ks", 1), ("co_t", 16), ("terms", 5), ("N", 0), ("csplit", 0), ("nsrc", 3)):
        a = conv_args(OP_CONV3, 1, (32, 0), 32, 8, 32, "affine", set(), 32, 3)
        setattr(a, field, bad)
        assert query(OP_CONV3, a) == -1, field
    assert query(OP_CONV3, conv_args(OP_CONV3, 1, (24, 8), 32, 8, 32, "affine+raw", set(), 32, 3)) == -1       # concat off a 16-channel boundary
    assert query(OP_CONV3, conv_args(OP_CONV3, 1, (32, 0), 32, 9, 33, "up:affine", set(), 32, 3)) == -1        # up-sampling to an odd plane
    assert query(OP_CONV3, conv_args(OP_CONV3, 1, (32, 0), 32, 8, 32, "affine", {"bnr"}, 32, 4)) == -1         # bnr without a BNBWD source
    # thin: 16 or 32 source channels, at most 16 outputs, two fp16 terms only
    assert query(OP_THIN, conv_args(OP_THIN, 1, (16, 0), 16, 8, 32, "raw", set(), 16, 4)) == 100
    assert query(OP_THIN, conv_args(OP_THIN, 1, (24, 0), 16, 8, 32, "raw", set(), 16, 4)) == -1
    assert query(OP_THIN, conv_args(OP_THIN, 1, (16, 0), 17, 8, 32, "raw", set(), 16, 4)) == -1
    assert query(OP_THIN, conv_args(OP_THIN, 1, (16, 0), 16, 8, 32, "raw", set(), 16, 3)) == -1
    assert query(OP_THIN, conv_args(OP_THIN, 1, (16, 0), 32, 8, 32, "raw", {"down0"}, 16, 4)) == -1            # down0 needs the BNBWD source
    # weight gradients
    assert query(OP_WGRAD3, wgrad_args(1, (32, 0), 32, 8, 32, ("raw", "raw"), set(), 3)) == 3110
    assert query(OP_WGRAD3, wgrad_args(1, (32, 0), 32, 8, 32, ("raw", "bnbwd"), set(), 3)) == -1
    assert query(OP_WGRAD3, wgrad_args(1, (32, 0), 32, 9, 33, ("raw", "up:affine"), set(), 3)) == -1
    assert query(OP_WTHIN, wgrad_args(1, (16, 0), 16, 8, 32, ("raw", "raw"), set(), 4)) == 100
    assert query(OP_WTHIN, wgrad_args(1, (16, 0), 16, 8, 33, ("raw", "raw"), set(), 4)) == -1                  # odd width
    assert query(OP_WTHIN, wgrad_args(1, (16, 0), 16, 8, 32, ("bnbwd", "raw"), {"offset"}, 4)) == -1           # gradient 4 bytes off
    assert query(OP_WTHIN, wgrad_args(1, (16, 0), 16, 8, 32, ("raw", "raw"), set(), 3)) == -1


def test_dispatch_thresholds():
    """the thresholds of the dispatch rules, one step either side"""
    def c3(k, srcs="affine", fl=(), terms=4):
        return query(OP_CONV3, conv_args(OP_CONV3, 1, (k, 0), 64, 8, 32, srcs, set(fl), 64, terms))
    assert c3(240) == 204 and c3(241) == 1204 and c3(288) == 1204                                   # 16 chunks of 16 channels
    assert c3(240, "bnbwd") == 214 and c3(241, "bnbwd") == 1214 and c3(256, "bnbwd") == 1214 and c3(257, "bnbwd") == 214
    assert c3(256, "bnbwd", ("bnr",)) == 214 and c3(256, terms=3) == 203 and c3(256, terms=0) == 203

    def wg(co, ci, dym="bnbwd", fl=(), terms=4, W=32):
        return query(OP_WGRAD3, wgrad_args(2, (ci, 0), co, 8, W, (dym, "raw"), set(fl), terms))
    assert wg(32, 32) == 14111 and wg(33, 32) == 14210 and wg(32, 33) == 14121 and wg(33, 33) == 14221
    assert wg(32, 64) == 14121 and wg(32, 65) == 14131 and wg(32, 96) == 14131 and wg(32, 97) == 14121 and wg(33, 80) == 14221
    assert wg(32, 80, "raw") == 4120 and wg(32, 80, W=33) == 4120 and wg(32, 80, fl=("offset",)) == 4120 and wg(32, 80, terms=3) == 3120
    assert terms_of(OP_WGRAD3, 14131) == 4 and terms_of(OP_CONV3, 1214) == 4
