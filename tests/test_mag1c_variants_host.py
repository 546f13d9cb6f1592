"""The case tables of tests/test_gpu_mag1c_variants.py reach EVERY launch form sc_mag1c_groups can take (no GPU).

sc_mag1c_groups switches on the host-only query sc_mag1c_variant.  Here the query is swept over S = 0..129 x {f32, f64} x {alpha 0,
!= 0} x {energy, none} x {direct, packed}; the set of codes it returns must EQUAL a literal list and the set of codes the GPU cases
assert: a kernel instantiation gaining a branch without a case, a case whose arguments no longer select the code written next to
it, or a dead code fails here.  Every refused combination is negative with a message, and the code changes between 64 and 65 bands
and nowhere else."""
import os
import re

import pytest

from test_gpu_mag1c_variants import (DIRECT_CASES, ENERGY_CASES, FALLBACK_SIZES, FLAG_CASES, GROUP_CASES, OPTIONS, SINGULAR_CASES, L,
                                     direct_sizes, stat_mask, swept_codes, table_codes, variant)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {
    "TILE4": 1100, "TILE4_SHRINK": 1101, "TILE4_ENERGY": 1110, "TILE4_ENERGY_SHRINK": 1111,          # fp32, S <= 64
    "TILE8_ENERGY": 1210, "TILE8_ENERGY_SHRINK": 1211, "TILE8_PAIR": 1220, "TILE8_PAIR_SHRINK": 1221,  # fp32, S > 64
    "TILE8_DIRECT": 1230, "TILE8_DIRECT_SHRINK": 1231,                                                # ... DIRECT mode
    "F64_FAST": 2000, "F64_512": 2100, "F64_512_ENERGY": 2110, "F64_1024": 2200, "F64_1024_ENERGY": 2210,
}


@pytest.fixture(scope="module")
def lib():
    from starcop_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_codes_mirror_the_header(lib):
    header = open(os.path.join(ROOT, "include", "starcop_hip.h")).read()
    body = re.search(r"enum sc_mag1c_launch \{(.*?)\};", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    in_header = {name: int(value) for name, value in re.findall(r"SC_MAG1C_([A-Z0-9_]+) = (\d+)", body)}
    assert in_header == L == WANT and len(set(WANT.values())) == len(WANT) == 15


def test_sweep_returns_exactly_the_enumerated_codes(lib):
    got = swept_codes()
    assert -1 in got
    assert got - {-1} == set(WANT.values()) == table_codes()


def test_the_rule_form_by_form(lib):
    v = lib.sc_mag1c_variant
    for S in range(1, 129):
        w = S > 64
        for a0 in (0, 1):
            sh = 1 - a0
            assert v(S, 0, a0, 0, 0) == (WANT["TILE8_PAIR"] if w else WANT["TILE4"]) + sh
            assert v(S, 0, a0, 1, 0) == (WANT["TILE8_ENERGY"] if w else WANT["TILE4_ENERGY"]) + sh
            if w:
                assert v(S, 0, a0, 0, 1) == WANT["TILE8_DIRECT"] + sh
        # fp64, alpha = 0: k_mag1c_fast whatever the band count, with compute_energy too (it branches on energy != NULL at run time)
        assert v(S, 1, 1, 0, 0) == v(S, 1, 1, 1, 0) == WANT["F64_FAST"]
        assert v(S, 1, 0, 0, 0) == (WANT["F64_1024"] if w else WANT["F64_512"])
        assert v(S, 1, 0, 1, 0) == (WANT["F64_1024_ENERGY"] if w else WANT["F64_512_ENERGY"])


def test_the_code_changes_between_64_and_65_bands_only(lib):
    v = lib.sc_mag1c_variant
    for f64 in (0, 1):
        for a0 in (0, 1):
            for en in (0, 1):
                codes = [v(S, f64, a0, en, 0) for S in range(1, 129)]
                steps = [S for S in range(1, 128) if codes[S - 1] != codes[S]]          # S | S + 1
                assert steps == ([] if f64 and a0 else [64]), (f64, a0, en, steps)
    assert v(64, 0, 1, 0, 0) == WANT["TILE4"] and v(65, 0, 1, 0, 0) == WANT["TILE8_PAIR"]
    assert v(64, 1, 0, 0, 0) == WANT["F64_512"] and v(65, 1, 0, 0, 0) == WANT["F64_1024"]


def test_refused_arguments(lib):
    v = lib.sc_mag1c_variant
    for S in (0, 129, -1, 1 << 20):
        for f64 in (0, 1):
            for a0 in (0, 1):
                for en in (0, 1):
                    for di in (0, 1):
                        assert v(S, f64, a0, en, di) == -1 and b"bands must be in [1,128]" in lib.sc_last_error(), (S, f64, a0, en, di)
    for S in range(1, 129):
        for f64 in (0, 1):
            for a0 in (0, 1):
                for en in (0, 1):
                    ok = not f64 and S > 64 and not en
                    got = v(S, f64, a0, en, 1)
                    assert (got > 0) == ok, (S, f64, a0, en)
                    if not ok:
                        assert got == -1 and b"DIRECT mode" in lib.sc_last_error()
                    assert v(S, f64, a0, en, 0) > 0
    # the entry point refuses through the same rule, before it looks at a pointer or launches anything
    from starcop_amd import _lib
    a = _lib.sc_mag1c_args()
    a.S = 129
    assert lib.sc_mag1c_groups(a, None) == -1 and b"bands must be in [1,128]" in lib.sc_last_error()
    a.S, a.cube = 64, 256
    assert lib.sc_mag1c_groups(a, None) == -1 and b"DIRECT mode" in lib.sc_last_error()
    a.S, a.x_is_f64 = 80, 1
    assert lib.sc_mag1c_groups(a, None) == -1 and b"DIRECT mode" in lib.sc_last_error()
    a.x_is_f64, a.cube = 0, None
    assert lib.sc_mag1c_groups(a, None) == -1 and b"null pointer" in lib.sc_last_error()


def _shapes():
    """(code, S, pixels per group) of every case of the GPU tables"""
    out = [(L[c[0]], c[1], c[4]) for c in GROUP_CASES]
    out += [(L[c[0]], c[2], (c[3], c[3])) for c in FLAG_CASES + ENERGY_CASES]
    out += [(L[c[0]], c[1], direct_sizes(c)) for c in DIRECT_CASES]
    return out


def test_every_case_selects_the_code_written_next_to_it(lib):
    for name, S, dt, alpha, sizes in GROUP_CASES:
        assert variant(S, dt, alpha) == L[name], (name, S)
        assert 0 in sizes[1:-1] and all(p == 0 or p >= S + 30 or (S, p) == (1, 11) for p in sizes), (name, S, sizes)
    for name, S, dt, sizes, bad in SINGULAR_CASES:
        assert variant(S, dt, 0.0) == L[name] and 0 < sizes[bad] <= S and 0 in sizes
        assert all(p == 0 or p >= S + 30 for i, p in enumerate(sizes) if i != bad)
    for name, dt, S, P, alpha in FLAG_CASES:
        assert variant(S, dt, alpha) == L[name] and P >= S + 30
    for name, dt, S, P, alpha in ENERGY_CASES:
        assert variant(S, dt, alpha, energy=True) == L[name] and P >= S + 30
    for c in DIRECT_CASES:
        assert variant(c[1], "f32", c[5], direct=True) == L[c[0]]
        sizes = direct_sizes(c)
        assert max(sizes) <= 512 and all(p == 0 or p >= c[1] + 30 for p in sizes)


def test_every_code_has_a_plain_and_a_ragged_case(lib):
    shapes = _shapes()
    for name, code in WANT.items():
        mine = [(S, sizes) for c, S, sizes in shapes if c == code]
        assert any(S % 16 == 0 and all(p % 512 == 0 for p in sizes) and any(sizes) for S, sizes in mine), (name, "no plain case")
        assert any(S % 16 == 1 and any(p % 16 for p in sizes) for S, sizes in mine), (name, "no ragged case")


def test_the_edges_the_tables_are_there_for(lib):
    groups = [(L[c[0]], c[1], c[2], c[4]) for c in GROUP_CASES]

    def bands(*names):
        return {S for code, S, _, _ in groups if code in {L[n] for n in names}}
    assert bands("TILE4", "TILE4_SHRINK") >= {1, 15, 16, 17, 48, 64} and bands("F64_512") >= {1, 15, 16, 17, 48, 64}
    assert bands("TILE8_PAIR", "TILE8_PAIR_SHRINK") >= {65, 80, 112, 113, 128} and bands("F64_1024") >= {65, 80, 112, 113, 128}
    for S in (65, 128):          # the pixel-count edges in one launch, around a skipped group: each group taken by exactly one kernel
        (sizes,) = [sz for code, s, _, sz in groups if code == L["TILE8_PAIR"] and s == S and len(sz) == 8]
        assert set(sizes) == {S + 30, 511, 512, 513, 1024, 1025, 1537, 0} and sizes.index(0) not in (0, 7)
    assert all(11 in sz for _, s, _, sz in groups if s == 1) and bands("F64_FAST") >= {1, 16, 17, 64, 65, 113, 128}
    # float64 radiances beyond 512 pixels: 1025 through k_mag1c_fast, k_mag1c<512> at 64 bands, k_mag1c<1024> at 65 and 128
    for name, S in (("F64_FAST", 65), ("F64_FAST", 64), ("F64_512", 64), ("F64_1024", 65), ("F64_1024", 128)):
        assert any(code == L[name] and s == S and dt == "f64" and 1025 in sz for code, s, dt, sz in groups), (name, S)
    assert max(sum(sz) * s for _, s, _, sz in groups) <= 6000 * 128
    # the option flags: the resident kernel (80 bands, 300 pixels), the streaming one (700) and both fp64 kernels at 80 bands
    assert {(c[1], c[2], c[3] <= 512) for c in FLAG_CASES} == {("f32", 80, True), ("f32", 80, False), ("f64", 80, False)}
    assert {L[c[0]] for c in FLAG_CASES} == {L["TILE8_PAIR"], L["TILE8_PAIR_SHRINK"], L["F64_FAST"], L["F64_1024"]}
    kws = [set(kw) for _, kw in OPTIONS]
    for key in ("albedo_override", "zero_override", "sparse_override", "covariance_update_scaling", "apply_scaling", "mask"):
        assert {key} in kws, key
    stat_mask(300, 300), stat_mask(700, 700), stat_mask(1025, 1026)
    # compute_energy beyond one chunk: fp32 at 1025 pixels for 64 and 65 bands and both alphas, fp64 at 65 bands
    en = {(c[1], c[2], c[3], c[4] == 0.0) for c in ENERGY_CASES}
    assert en >= {("f32", 64, 1025, True), ("f32", 64, 1025, False), ("f32", 65, 1025, True), ("f32", 65, 1025, False),
                  ("f64", 65, 1025, True), ("f64", 65, 1025, False)}
    # DIRECT mode: 65 and 128 bands, a column group of exactly 512 pixels; the 513-pixel group of the fall-back case
    assert {c[1] for c in DIRECT_CASES} == {65, 128} and any(512 in direct_sizes(c) for c in DIRECT_CASES)
    assert 513 in FALLBACK_SIZES and sum(FALLBACK_SIZES) <= 512 * (len(FALLBACK_SIZES) + 1)
    assert {(c[0], c[1], c[2]) for c in SINGULAR_CASES} == {("TILE4", 24, "f32"), ("TILE8_PAIR", 80, "f32"), ("F64_FAST", 80, "f64")}
    assert all(c[3][c[4]] <= 512 for c in SINGULAR_CASES)
