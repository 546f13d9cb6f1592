"""The GPU case tables of tests/test_gpu_elementwise_variants.py reach EVERY launch form and loop regime of the streaming kernels of
elementwise.hip, including every one the network reaches, and every bound in them is tight enough to see a realistic defect (no GPU).

sc_bn_finalize, sc_bn_bwd_finalize_rows32, sc_add_srcs_absmax, sc_bn_bwd_reduce and sc_bn_bwd_small dispatch on the host queries
sc_bn_finalize_form, sc_bn_bwd_rows32_form and sc_ew_vec_form.  Here each query is swept over its argument space (rows 1..9000 x
channels 1..600 in full where scratch is given in training, which is where both limits act; every row count at five channel counts
and every channel count at four row counts otherwise; HW 1..64 x both alignments), and the set of codes it returns must EQUAL the enum in include/starcop_hip.h and the set of codes of the case tables; the row and channel limits of the
pre-reduction lie where the header says and nowhere else.  HyperStarcopUNet's BatchNorm tensors are walked at the training shape and
at a small one: every (form, loop regime) the network reaches has a case.  The strength tests run a float64 model of each operator
with one defect -- a chunk's last float4 dropped, `>=` for `>` in the mask, eps inside Adam's square root, decoupled weight decay, the
second bilinear row not clamped, a pool tie going to the last maximum, a biased running variance, a gather window one row short -- on
the inputs of the GPU cases and assert that the result lies outside the case's bound."""
import math
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_elementwise_variants as T
from test_gpu_elementwise_variants import (ACTS, ADAM_CASES, ADD_CASES, ADD_SHAPE, BCE_CASES, BN_FIN_CASES, BN_REDUCE_CASES, BN_ROWS32_CASES,
                                           BN_SMALL_CASES, CLS_CASES, DOWNSUM_CASES, EW_SCALAR, EW_VEC4, FIN_EVAL, FIN_PRE64, FIN_ROWS4,
                                           FIN_ROWS16, MASK_CASES, POOL_CASES, R32_F32, R32_PRE64, U, UP_BWD_CASES, UP_CASES, UP_SHAPES,
                                           chain_reduce, chain_small, fin_form, fin_regime, rows32_form, small_regime, vec_form)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_enum(name, prefix):
    header = open(os.path.join(ROOT, "include", "starcop_hip.h")).read()
    body = re.search(r"enum %s \{(.*?)\};" % name, header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return {n: int(v) for n, v in re.findall(prefix + r"([A-Z0-9_]+) = (\d+)", body)}


def _fl(flags):
    return set(flags.split())


def test_codes_mirror_the_header():
    assert header_enum("sc_bn_finalize_form", "SC_BN_FIN_") == dict(EVAL=FIN_EVAL, ROWS4=FIN_ROWS4, ROWS16=FIN_ROWS16, PRE64=FIN_PRE64)
    assert header_enum("sc_bn_bwd_rows32_form", "SC_BN_ROWS_") == dict(F32=R32_F32, PRE64=R32_PRE64)
    assert header_enum("sc_ew_vec_form", "SC_EW_") == dict(SCALAR=EW_SCALAR, VEC4=EW_VEC4)


def test_finalize_form_sweep_and_limits():
    """nrows 1..9000 x C 1..600 x scratch x training: exactly the enumerated codes, the switch at 4096 rows and 512 channels only"""
    rows_axis = list(range(1, 9001))
    chans = list(range(1, 601))
    seen = set()
    for scratch in (0, 1):
        for training in (0, 1):
            by_rows = {C_: [fin_form(n, C_, scratch, training) for n in rows_axis] for C_ in (1, 24, 512, 513, 600)}
            by_chan = {n: [fin_form(n, C_, scratch, training) for C_ in chans] for n in (1, 4095, 4096, 9000)}
            for C_, codes in by_rows.items():
                seen.update(codes)
                steps = [rows_axis[i] for i in range(1, len(codes)) if codes[i] != codes[i - 1]]
                assert steps == ([4096] if training else []), (scratch, training, C_, steps)
                if training:
                    assert codes[0] == FIN_ROWS4 and codes[-1] == (FIN_PRE64 if scratch and C_ <= 512 else FIN_ROWS16)
            for n, codes in by_chan.items():
                seen.update(codes)
                steps = [chans[i] for i in range(1, len(codes)) if codes[i] != codes[i - 1]]
                assert steps == ([513] if training and scratch and n >= 4096 else []), (scratch, training, n, steps)
    # where both limits act (training with scratch): the whole product, against the rule written out
    f = T._lib.load().sc_bn_finalize_form
    for C_ in chans:
        want = [FIN_ROWS4] * 4095 + [FIN_PRE64 if C_ <= 512 else FIN_ROWS16] * (9000 - 4095)
        assert [f(n, C_, 1, 1) for n in rows_axis] == want, C_
    assert seen == {FIN_EVAL, FIN_ROWS4, FIN_ROWS16, FIN_PRE64} == {c[0] for c in BN_FIN_CASES}
    assert fin_form(0, 3, 0, 0) == FIN_EVAL and fin_form(0, 3, 1, 1) < 0 and fin_form(5, 0, 0, 1) < 0 and fin_form(5, 0, 0, 0) < 0


def test_rows32_form_sweep_and_limits():
    seen = set()
    for scratch in (0, 1):
        for C_ in (1, 5, 512, 513, 600):
            codes = [rows32_form(n, C_, scratch) for n in range(1, 9001)]
            seen.update(codes)
            steps = [i + 1 for i in range(1, len(codes)) if codes[i] != codes[i - 1]]
            assert steps == ([4096] if scratch and C_ <= 512 else []), (scratch, C_, steps)
        codes = [rows32_form(5000, C_, scratch) for C_ in range(1, 601)]
        assert [i + 1 for i in range(1, len(codes)) if codes[i] != codes[i - 1]] == ([513] if scratch else [])
    f = T._lib.load().sc_bn_bwd_rows32_form
    for C_ in range(1, 601):        # with scratch: the whole product
        want = [R32_F32] * 4095 + [R32_PRE64 if C_ <= 512 else R32_F32] * (9000 - 4095)
        assert [f(n, C_, 1) for n in range(1, 9001)] == want, C_
    assert seen == {R32_F32, R32_PRE64} == {c[0] for c in BN_ROWS32_CASES}
    assert rows32_form(0, 5, 1) < 0 and rows32_form(5, 0, 1) < 0


def test_vec_form_sweep():
    got = {(hw, al): vec_form(hw, al) for hw in range(1, 65) for al in (False, True)}
    assert all(code == (EW_VEC4 if hw % 4 == 0 and al else EW_SCALAR) for (hw, al), code in got.items())
    assert set(got.values()) == {EW_SCALAR, EW_VEC4}
    for table in (BN_REDUCE_CASES, BN_SMALL_CASES, ADD_CASES):
        assert {c[0] for c in table} == {EW_SCALAR, EW_VEC4}
    assert vec_form(0, True) < 0 and vec_form(4100, True) == EW_VEC4 and vec_form(4100, False) == EW_SCALAR


# what each table is there for
WANT_FIN = {(FIN_ROWS4, "tail"), (FIN_ROWS4, "loop"), (FIN_ROWS16, "tail"), (FIN_ROWS16, "loop"), (FIN_PRE64, "tail"), (FIN_EVAL, "tail")}
WANT_SMALL = {"scalar", "tail", "loop"}


def test_finalize_table():
    assert {(c[0], fin_regime(c[0], c[1])) for c in BN_FIN_CASES} == WANT_FIN
    for form, nrows, C_, scratch, flags in BN_FIN_CASES:
        assert fin_form(nrows, C_, scratch, form != FIN_EVAL) == form
        assert nrows * C_ * 8 <= 21 * 2 ** 20
    rows4 = {c[1] for c in BN_FIN_CASES if c[0] == FIN_ROWS4 and not c[4]}
    rows16 = {(c[1], c[2], c[3]) for c in BN_FIN_CASES if c[0] == FIN_ROWS16}
    assert rows4 == {5, 2500} and rows16 == {(4096, 3, 0), (8300, 3, 0), (4096, 520, 1)}
    assert 5 < 256 and 7 * 256 < 2500 and 2500 % (8 * 256) != 0 and 4096 <= 7 * 1024 < 8300 and 8300 % (8 * 1024) != 0
    assert {(c[1], c[2]) for c in BN_FIN_CASES if c[0] == FIN_PRE64} == {(n, C_) for n in (4096, 5000) for C_ in (1, 24, 512)}
    assert all(c[3] == 1 for c in BN_FIN_CASES if c[0] == FIN_PRE64) and 1024 % 48 != 0 and 4096 % 64 == 0 and 5000 % 64 != 0
    assert {c[4] for c in BN_FIN_CASES} == {"", "count1", "negvar"}
    # the negative-variance channel is negative in float64 (asserted where it is built) and is clamped: invstd = 1 / sqrt(eps)
    ins, checks = T.bn_fin_ref(next(c for c in BN_FIN_CASES if c[4] == "negvar"))
    assert abs(float(checks["cst"][0][1, 3]) - 1 / math.sqrt(T.f32(T.EPS))) < 1e-9
    ins, checks = T.bn_fin_ref(next(c for c in BN_FIN_CASES if c[4] == "count1"))
    assert ins["count"] == 1.0 and float(checks["act_bound"][0]) == float(ins["beta"].abs().max())
    # mixed signs in column 0
    ins, _ = T.bn_fin_ref(BN_FIN_CASES[0])
    assert bool((ins["rows"][:, :, 0] < 0).any()) and bool((ins["rows"][:, :, 0] > 0).any())


def test_backward_tables():
    assert {(c[3], c[0]) for c in BN_REDUCE_CASES if not c[5]} == {(3, EW_SCALAR), (320, EW_VEC4), (4096 + 8, EW_VEC4), (4099, EW_SCALAR)}
    assert {(c[0], c[4]) for c in BN_REDUCE_CASES} == {(f, a) for f in (EW_SCALAR, EW_VEC4) for a in ACTS}
    assert {(c[0], c[4]) for c in BN_SMALL_CASES} == {(f, a) for f in (EW_SCALAR, EW_VEC4) for a in ACTS}
    for form, N, C_, HW, act, flags in BN_REDUCE_CASES + BN_SMALL_CASES:
        off = "offset" in _fl(flags)
        assert vec_form(HW, not off) == form
        if off:         # the same shape, aligned, takes the 16-byte form and is in the table
            assert form == EW_SCALAR and vec_form(HW, True) == EW_VEC4
    assert all((2, 3) == c[1:3] for c in BN_REDUCE_CASES) and len(BN_REDUCE_CASES) == 15 and len(BN_SMALL_CASES) == 15
    assert sum("offset" in _fl(c[5]) for c in BN_REDUCE_CASES) == 3 and sum("offset" in _fl(c[5]) for c in BN_SMALL_CASES) == 3
    small = {(c[1], c[2], c[3]): small_regime(c[1], c[3], c[0] == EW_VEC4) for c in BN_SMALL_CASES if not c[5]}
    assert small == {(3, 5, 49): "scalar", (2, 4, 320): "tail", (5, 3, 1028): "loop", (16, 64, 1024): "loop"}
    assert set(small.values()) == WANT_SMALL
    assert 16 * 1024 == 16384 and (16 * 1024 // 4) % 1024 == 0 and (5 * 1028 // 4) % 1024 != 0 and 1028 // 4 % 256 != 0
    assert [(c[0], c[1], c[3]) for c in BN_ROWS32_CASES] == [(R32_F32, 40, 0), (R32_F32, 4096, 0), (R32_PRE64, 4100, 1)]
    for form, nrows, C_, scratch in BN_ROWS32_CASES:
        assert rows32_form(nrows, C_, scratch) == form
    assert ADD_SHAPE == (2, 3, 4100) and 4100 % 4 == 0 and 4100 % 2048 == 4
    assert {k for _, k in ADD_CASES} == {"record_only", "norm+raw", "raw+bnbwd_none", "raw+bnbwd_relu"} and len(ADD_CASES) == 8


def test_other_tables():
    assert {(c[1], c[2]) for c in POOL_CASES} == {(1, 1), (5, 7), (33, 35)} and 33 * 35 > 1024 and len(POOL_CASES) == 9
    assert set(UP_SHAPES) == {(1, 1), (1, 5), (4, 1), (5, 7), (17, 19), (256, 4)} and len(UP_CASES) == 18
    assert set(UP_BWD_CASES) == set(UP_SHAPES) | {(4, 256)}
    assert {c[:4] for c in DOWNSUM_CASES} == {(2, 3, 5, 7), (2, 9, 256, 256)} and {c[4] for c in DOWNSUM_CASES} == {0, 1}
    assert 2 * 9 * 256 * 256 > 4096 * 256 and 2 * 9 * 512 * 512 * 4 <= 20 * 2 ** 20
    assert {c[0] for c in BCE_CASES} == {1, 5000, 262144 + 257} and 262144 == 1024 * 256 and {c[1] for c in BCE_CASES} == {1.0, 15.0}
    assert {c[0] for c in ADAM_CASES} == {1, 4097, 1048576 + 257} and 1048576 == 4096 * 256
    assert {c[0] for c in MASK_CASES} == {7, 4096, 8192 + 37} and {c[1] for c in MASK_CASES} == {"all", "nopred", "nopb", "nodiff", "nocount"}
    assert CLS_CASES == [(130, 64, 64), (130, 50, 70)] and 130 > 128
    for case in CLS_CASES:
        cnt, ref, thr = T.cls_ref(case)
        assert {math.floor(thr), math.ceil(thr)} <= set(cnt.tolist()) and set(ref.tolist()) == {0, 1}
    assert (10 * 50 * 70) % 4096 != 0 and T.cls_ref(CLS_CASES[0])[2] == 10.0
    z, t, w = T.bce_inputs(5000)
    assert {30.0, -30.0, 90.0, -90.0, 104.0, -104.0} <= set(z.tolist()) and set(t.tolist()) == {0.0, 1.0}
    z, t = T.mask_inputs(4096)
    assert bool((z == 0).any()) and float(z[z != 0].abs().min()) >= 1e-3 and {0.5, 2.0, 0.0, 1.0} <= set(t.unique().tolist())
    p0, grads = T.adam_inputs(4097)
    mags = {float(v) for v in grads[0][:32].abs().unique()}
    assert 0.0 in mags and any(abs(m / 1e-20 - 1) < 1e-5 for m in mags) and any(abs(m / 1e4 - 1) < 1e-5 for m in mags)


def test_chain_counts():
    assert chain_reduce(3, False) == 1 and chain_reduce(320, True) == 4 and chain_reduce(320, False) == 2
    assert chain_reduce(4096 + 8, True) == 16 and chain_reduce(4099, False) == 16
    assert chain_small(3, 49, False) == 1 and chain_small(2, 320, True) == 4 and chain_small(5, 1028, True) == 16
    assert chain_small(16, 1024, True) == 16 and chain_small(2, 320, False) == 2


def network_forms(N, H, W):
    """(finalize form, regime) and (backward kernel, regime) of every BatchNorm tensor of HyperStarcopUNet at (N, H, W): the rule of
    plan construction (statistics rows by producer kind) and of bn_backward in starcop_amd/network.py"""
    from starcop_amd import _lib, network
    from starcop_amd._lib import STAT_CONV1, STAT_CONV1K, STAT_CONV3, STAT_DW, STAT_PW3, STAT_STEM
    lib = _lib.load()
    net = network.HyperStarcopUNet(4, 1)
    kind_of = {"stem": STAT_STEM, "dw": STAT_DW, "conv3": STAT_CONV3, "pw": STAT_CONV1}
    fin, bwd = set(), set()
    for op in net._ops:
        t = op["out"]
        if t.bn is None:
            continue
        Ho, Wo = H >> t.shift, W >> t.shift
        kind = kind_of[op["type"]]
        if op["type"] == "pw" and network._use_pw3(0, N, Ho * Wo, op["conv"].in_channels, op["conv"].out_channels):
            kind = STAT_PW3
        elif op["type"] == "pw" and network._use_ksplit(N, Ho * Wo, op["conv"].in_channels, op["conv"].out_channels):
            kind = STAT_CONV1K
        rows = lib.sc_stat_rows(kind, N, Ho, Wo)
        form = fin_form(rows, t.C, True, 1)
        fin.add((form, fin_regime(form, rows)))
        vec = vec_form(Ho * Wo, True) == EW_VEC4
        if N * Ho * Wo <= net.bn_small_max and t.C >= 64:
            bwd.add(("small", small_regime(N, Ho * Wo, vec), t.act))
        else:
            bwd.add(("reduce", vec, Ho * Wo > 4096, t.act))
    return fin, bwd


@pytest.mark.parametrize("shape", [(16, 512, 512), (2, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_network_forms_have_cases(shape):
    fin, bwd = network_forms(*shape)
    assert fin and bwd
    have_fin = {(c[0], fin_regime(c[0], c[1])) for c in BN_FIN_CASES}
    assert fin <= have_fin, fin - have_fin
    have = {("small", small_regime(c[1], c[3], c[0] == EW_VEC4), c[4]) for c in BN_SMALL_CASES}
    have |= {("reduce", c[0] == EW_VEC4, c[3] > 4096, c[4]) for c in BN_REDUCE_CASES}
    assert bwd <= have, bwd - have
    if shape[0] == 16:      # the training shape: the four-items-in-flight loop at the border N HW = bn_small_max, the pre-reduction
        assert any(b[:2] == ("small", "loop") for b in bwd) and (FIN_PRE64, "tail") in fin
    assert (FIN_EVAL, "tail") in have_fin         # inference: sc_bn_finalize(stats = NULL, training = 0)


def test_position_arithmetic_of_the_bilinear_kernels():
    """fl(fl((n - 1) / (2 n - 1)) Y) for every axis length of the cases: within u n of the exact position, and never on the other side
    of an integer: the weight matrices of kernel and reference have the same taps"""
    for n in sorted({v for s in UP_BWD_CASES for v in s}):
        if n == 1:
            continue
        s = np.float32(n - 1) / np.float32(2 * n - 1)
        fy = (s * np.arange(2 * n, dtype=np.float32)).astype(np.float32).astype(np.float64)
        p = np.arange(2 * n, dtype=np.float64) * (n - 1) / (2 * n - 1)
        assert np.abs(fy - p).max() <= U * n, n
        assert (np.floor(fy)[:-1] == np.floor(p)[:-1]).all() and fy[-1] <= n - 1, n


def test_loss_bound_is_no_looser_than_the_operator_test():
    """with the allowance recorded from an MI355X: per pixel and for the mean, bound <= 1e-5 max(1, |ref|)"""
    for case in BCE_CASES:
        n = case[0]
        _, checks = T.bce_ref(case, T.MEASURED_MATH)
        for key, scale in (("loss_px", 1), ("loss_sum", n)):
            ref, eb, _ = checks[key]
            assert bool((eb / scale <= 1e-5 * (ref.abs() / scale).clamp_min(1.0)).all()), (case, key)
        ref, eb, _ = checks["dz"]
        assert float(eb.max()) <= 1e-5 * float(ref.abs().max()), case


def violation(ref, bound, mutated):
    """the largest |mutated - ref| / bound; inf for a non-finite result or an error where the bound is zero"""
    if not bool(torch.isfinite(mutated).all()):
        return math.inf
    err = (mutated.double() - ref).abs()
    pos = bound > 0
    if bool((err[~pos] > 0).any()):
        return math.inf
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


def _checks_ok(name, checks):
    for key, (ref, bound, mutated) in checks.items():
        if bound is not None:
            assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), (name, key)


STRENGTH = ([(T.bn_fin_ref, c) for c in BN_FIN_CASES if c[0] != FIN_EVAL and "count1" not in _fl(c[4])]
            + [(T.bn_reduce_ref, c) for c in BN_REDUCE_CASES] + [(T.bn_small_ref, c) for c in BN_SMALL_CASES]
            + [(T.bn_rows32_ref, c) for c in BN_ROWS32_CASES] + [(T.add_ref, k) for k in sorted({c[1] for c in ADD_CASES})]
            + [(T.pool_ref, c) for c in POOL_CASES if (c[1], c[2]) != (1, 1)] + [(T.up_ref, c) for c in UP_CASES] + [(T.up_bwd_ref, c) for c in UP_BWD_CASES])


@pytest.mark.parametrize("ref_of,case", STRENGTH, ids=lambda v: v.__name__ if callable(v) else T._id(v))
def test_bounds_see_the_defect(ref_of, case):
    """a chunk's last float4 dropped (sums, add), a biased running variance, a tie going to the last maximum, the second bilinear row
    not clamped, a gather window one row short: outside the bound somewhere"""
    _, checks = ref_of(case)
    _checks_ok(ref_of.__name__, checks)
    seen = 0
    for key, (ref, bound, mutated) in checks.items():
        if mutated is None:
            continue
        r = violation(ref, bound, mutated)
        print(f"STRENGTH {ref_of.__name__} {case} {key} {r:.3g}")
        assert r > 2, (key, r)
        seen += 1
    assert seen


def test_pool_has_ties():
    for case in POOL_CASES:
        _, checks = T.pool_ref(case)
        if case[0] == "affine6" and case[1] > 1:
            assert float(checks["ties"][0]) > 0.1, case


@pytest.mark.parametrize("case", [c for c in ADAM_CASES if c[0] >= 64], ids=T._id)
def test_adam_bounds_see_the_defects(case):
    _, checks = T.adam_ref(case)
    _checks_ok("adam", checks)
    _, inside = T.adam_ref(case, eps_inside=True)
    assert violation(*checks["p"][:2], inside["p"][0]) > 100
    if case[1] == "wd":
        _, dec = T.adam_ref(case, decoupled=True)
        assert all(violation(*checks[k][:2], dec[k][0]) > 100 for k in ("m", "v", "p"))


@pytest.mark.parametrize("HW", sorted({c[0] for c in MASK_CASES}))
def test_masks_see_a_wrong_comparison(HW):
    (z, t), ref = T.mask_ref(HW, 0)
    _, wrong = T.mask_ref(HW, 0, strict=False)
    assert not torch.equal(ref["pb"], wrong["pb"]) and not torch.equal(ref["diff"], wrong["diff"]) and not torch.equal(ref["count"], wrong["count"])
    # sigmoid > .5 is decided alike in fp32 and float64 for these logits
    assert torch.equal((torch.sigmoid(z) > 0.5), (torch.sigmoid(z.double()) > 0.5))
