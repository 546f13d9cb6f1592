"""Every launch form and loop regime of the streaming kernels of elementwise.hip against float64, element by element.

sc_bn_finalize picks EVAL | ROWS4 | ROWS16 | PRE64 (host query sc_bn_finalize_form), sc_bn_bwd_finalize_rows32 picks ROWS_F32 | PRE64
(sc_bn_bwd_rows32_form), and sc_add_srcs_absmax, sc_bn_bwd_reduce and sc_bn_bwd_small pick SCALAR | VEC4 (sc_ew_vec_form, from HW and the
alignment of every tensor of the launch).  The launchers dispatch on those functions.  Every case names the code it was written for and
asserts it through the query before it launches; tests/test_elementwise_variants_host.py holds the tables below to the full set of
codes and loop regimes, to what the network reaches, and checks on the CPU that the bounds see one realistic defect each, which is why
the tables, the chain counts and the references sit at module level and touch no device.

References: the same operation in float64 on the CPU from the same fp32 inputs.  Bounds are derived, not measured (with one stated
exception, the two math calls of the loss), and hold element by element; u = 2^-24, d = 2^-53, "chain" = the longest sequence of fp32
additions one accumulator sees (chain_* below).

BatchNorm finalize.  The rows are summed in float64 on both sides, in different orders: S1, S2 carry (nrows + 8) d sum|row| (e1, ev
below, after the division by count and through var = S2 / count - mean^2).  Then
  mean    one cast                                     u |mean| + e1
  invstd  one cast of 1 / sqrt(var + eps)              u invstd + invstd^3 ev / 2
  scale   the cast and gamma * invstd                  |gamma| (2 u invstd + invstd^3 ev / 2)
  shift   beta - mean * scale: what scale and mean carry, the product, the subtraction
                                                       4 u |mean scale| + u (|beta| + |mean scale|) + the ev terms
  cst[4..8] exactly 0; the running statistics are one cast of a float64 expression: u |value| (+ momentum x e1 / ev)
  act_bound in [b, b (1 + 4 u)], b = max_c |gamma| sqrt(count - 1) + |beta|; never lowered; untouched in eval
BatchNorm backward.  A term of S1 is g' = g x mask (exact), a term of S2 is g' x_hat with x_hat = (y - mean) invstd rounded twice (the
product enters an FMA unrounded).  The masks are those of float64: the inputs are moved off the thresholds (below).
  sums    |S - ref| <= n u sum|terms| (+ 2 u sum|terms| for S2) + (rows + 512) d sum|terms|, n = chain_reduce / chain_small:
          a thread adds 16 elements of a 4096-chunk (sc_bn_bwd_reduce), 16 per unrolled pass, 4 per tail item or ceil(HW / 256) of
          a plane (sc_bn_bwd_small) in fp32 before the value goes to float64
  dbeta, dgamma = the cast of the sums: + u |S|;  cst_bwd {scale, shift, A} are copies (exact), B = -scale c2 invstd and
  D = -scale c1 + scale c2 invstd mean (c = S / count) carry what the sums carry, times those factors, + u |value|
  absmax within 2 u of max_c |scale_c| max |g'| (one product); act_absmax within 2 u of max |y_hat| (one FMA), capped at 6 behind
  ReLU6, and not below the fp32 value of max |act(y_hat)|; both unchanged when they start above the result
  sc_bn_bwd_finalize_rows32: float rows summed in float64 on both sides: only the d term and the casts
sc_add_srcs_absmax.  NORM = clamp((x - off) / fac): two roundings; BNBWD = fma(g', A, fma(y, B, D)): u |y B + D| + u |v|; the sum of
the two operands: u |sum|; all times (1 + 4 u) for the second order.  The record is the maximum of what was written, bit for bit.
Pool.  Inputs on a dyadic grid (multiples of 1/8, power-of-two scale): every value is exact in fp32, so torch.equal.
Bilinear x2 (align_corners).  The kernel forms the source position of output row Y as fl(fl((Hin - 1) / (Ho - 1)) Y): two roundings of
a value below Hin, so it is off by at most 2 u Hin (measured on the CPU for Hin = 1..1024: 1.26 u Hin at worst); that moves weight
between the two source rows by as much, and the result by that times the difference of the two row values, which lie within the four
taps.  Likewise for the columns.  The lerp itself is the prologue's rounding, 1 - l, three products and two sums per tap: at most
8 roundings.  Hence  |out - ref| <= 2 u (Hin + Win) max|v| over the four taps + 8 u sum |w| |v|.  (For taps of mixed sign the two
row values can differ by up to 2 max|v|: the bound then relies on the position error staying below u Hin, which the host test checks
with the kernel's own fp32 position arithmetic for every shape used here.)  The backward is the transpose: an input pixel collects
  |gin - ref| <= 2 u Hin sum over the outputs that tap its row (within 1 + 2 u Hin of it) of |wx| |g| + the same for columns
                 + (ky + kx + 2) u sum |w| |g|,   ky, kx = the most outputs per axis that tap one input (the two FMA chains), + 2 for
the two weights.  No contribution may be lost by the gather window: a lost one is a whole term, far outside this.
sc_downsum2x2: (a + b) + (c + d) in fp32 in that order, bit for bit (IEEE addition is the same on both sides).
Loss.  lw = 1 + (pos_weight - 1) y is exact for y in {0, 1}; L = log1p(exp(-|x|)) carries the two math calls, K = ke + kl in units of
u relative (an error of exp passes through log1p with a factor t / ((1 + t) log1p t) <= 1); sp = L + max(-x, 0): u sp; lw sp: u
lw sp unless lw = 1; the final sum: u |l|:
  |l - ref|  <= u (K lw L + lw sp + [lw != 1] lw sp + |l|) + lw 2^-126       (2^-126: results below the normal range may be flushed)
  |dz - ref| <= (w / n) (u (lw sig (ke + 3) + 4 |lw sig - pos_weight y|) + lw 2^-126)   sig = 1 / (1 + exp(-x)): exp, sum, division;
                                                                  then the product, the difference, times w, times fl(1 / n)
  loss_sum: the sum of the above times w, + u |l w| for the product, + (n / 2^18 + 1100) d (|start| + sum |l w|) for the float64 sums
ke, kl are not known here: they are MEASURED on the GPU against float64, not against the kernel -- torch's fp32 exp and log1p of the
test's own arguments -- and twice the worst seen is allowed.  Measured on an MI355X: see MEASURED_MATH below.  The total bound
must not exceed the 1e-5 max(1, |ref|) of test_bce_loss_and_grad; the host test asserts that with the allowance of MEASURED_MATH.
Adam.  The float64 recurrence of torch.optim.Adam (L2 decay) runs next to a recurrence of its error bound:
  g' = g s (+ wd p): u per operation;  m' = m + (g' - m)(1 - b1): b1 dm + (1 - b1) dg + u (2 |g' - m| (1 - b1) + |m'|);
  v' = b2 v + (1 - b2) g'^2: b2 dv + (1 - b2) 2 |g'| dg + u (|b2 v| + 3 (1 - b2) g'^2 + |v'|) + 2^-125;  1 - b1, 1 - b2 are exact in fp32;
  denom = sqrt(v') / bc2s + eps: sqrt(v' + dv) - sqrt(v' - dv) + (3 u) sqrt(v') / bc2s + u denom;
  p' = p - (lr / bc1) (m' / denom): dp + |upd| (dm / |m'| + ddenom / denom + 6 u) + u |p'|   (casts of the two corrections, lr / bc1,
  the quotient, the product, then the subtraction)
step and hp = {lr, 1 - b1^t, sqrt(1 - b2^t)} match float64 to 1 u.
Masks: integer outputs bit for bit; logits are exactly 0 or at least 1e-3 in magnitude, so sigmoid > .5 is decided alike in fp32 and
float64; prediction within (ke + 2) u.

The masks of ReLU / ReLU6 are discontinuous, so where scale y + shift lies within 1e-3 of 0 or 6 the input is moved by 0.01: no element
is excluded from any comparison.  Outputs start as NaN.  Every case prints its error-to-bound ratios before it asserts."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hip_ops import DEV, dev  # noqa: E402
from starcop_amd import _lib  # noqa: E402
from starcop_amd._lib import (ACT_NONE, ACT_RELU, ACT_RELU6, SC_CST, SRC_AFFINE, SRC_BNBWD, SRC_NORM, SRC_RAW, STAT_BNBWD, check, make_src,
                              ptr, stream)  # noqa: E402
from test_gpu_depthwise_variants import _bc, _off_threshold, dev_at  # noqa: E402
from test_gpu_ops import rnd  # noqa: E402

U = 2.0 ** -24
D = 2.0 ** -53
TINY = 2.0 ** -126
FIN_EVAL, FIN_ROWS4, FIN_ROWS16, FIN_PRE64 = 0, 1, 2, 3      # enum sc_bn_finalize_form
R32_F32, R32_PRE64 = 0, 1                                     # enum sc_bn_bwd_rows32_form
EW_SCALAR, EW_VEC4 = 0, 1                                     # enum sc_ew_vec_form
# the allowance for expf / log1pf in units of u relative: twice the worst error of torch's fp32 exp / log1p on an MI355X over the
# arguments of BCE_CASES (measured there: exp 1.334 u, log1p 1.045 u -- math_allowance() measures again in every run)
MEASURED_MATH = (2 * 1.334, 2 * 1.045)

# ---- case tables (no device)
# (form, nrows, C, scratch given, flags); flags: count1 (one sample), negvar (a channel whose E[x^2] - mean^2 is negative in float64)
BN_FIN_CASES = [
    (FIN_ROWS4, 5, 3, 0, ""),                 # tail loop only
    (FIN_ROWS4, 2500, 3, 0, ""),              # one unrolled pass of 8 x 256 rows, then the tail
    (FIN_ROWS4, 1, 3, 0, "count1"),
    (FIN_ROWS4, 300, 4, 1, "negvar"),
    (FIN_ROWS16, 4096, 3, 0, ""),             # tail only
    (FIN_ROWS16, 8300, 3, 0, ""),             # one unrolled pass of 8 x 1024 rows, then the tail
    (FIN_ROWS16, 4096, 520, 1, ""),           # scratch given, pre-reduction refused: 2 C > 1024
    (FIN_PRE64, 4096, 1, 1, ""), (FIN_PRE64, 5000, 1, 1, ""),          # E = 2
    (FIN_PRE64, 4096, 24, 1, ""), (FIN_PRE64, 5000, 24, 1, ""),        # E = 48 does not divide 1024
    (FIN_PRE64, 4096, 512, 1, ""), (FIN_PRE64, 5000, 512, 1, ""),      # E = 1024: one row per pass
    (FIN_EVAL, 0, 3, 0, ""), (FIN_EVAL, 0, 24, 1, ""),
]
ACTS = (ACT_NONE, ACT_RELU, ACT_RELU6)
# (form, N, C, HW, act, flags); offset: g and y start 4 bytes past a 16-byte boundary
BN_REDUCE_CASES = ([(EW_SCALAR, 2, 3, 3, a, "") for a in ACTS] + [(EW_VEC4, 2, 3, 320, a, "") for a in ACTS]
                   + [(EW_VEC4, 2, 3, 4096 + 8, a, "") for a in ACTS] + [(EW_SCALAR, 2, 3, 4099, a, "") for a in ACTS]
                   + [(EW_SCALAR, 2, 3, 320, a, "offset") for a in ACTS])
BN_SMALL_CASES = ([(EW_SCALAR, 3, 5, 49, a, "") for a in ACTS] + [(EW_VEC4, 2, 4, 320, a, "") for a in ACTS]
                  + [(EW_VEC4, 5, 3, 1028, a, "") for a in ACTS] + [(EW_VEC4, 16, 64, 1024, a, "") for a in ACTS]
                  + [(EW_SCALAR, 2, 4, 320, a, "offset") for a in ACTS])
# (form, nrows, C, scratch given)
BN_ROWS32_CASES = [(R32_F32, 40, 5, 0), (R32_F32, 4096, 5, 0), (R32_PRE64, 4100, 5, 1)]
# (form, kind); shape (2, 3, 4100): two full chunks of 2048 and one of 4 elements
ADD_SHAPE = (2, 3, 4100)
ADD_CASES = [(f, k) for k in ("record_only", "norm+raw", "raw+bnbwd_none", "raw+bnbwd_relu") for f in (EW_VEC4, EW_SCALAR)]
SRC_MODES = ("raw", "affine_relu", "affine6")
POOL_CASES = [(m, ho, wo) for m in SRC_MODES for ho, wo in ((1, 1), (5, 7), (33, 35))]
UP_SHAPES = ((1, 1), (1, 5), (4, 1), (5, 7), (17, 19), (256, 4))
UP_CASES = [(m, h, w) for h, w in UP_SHAPES for m in SRC_MODES]
UP_BWD_CASES = list(UP_SHAPES) + [(4, 256)]
DOWNSUM_CASES = [(2, 3, 5, 7, 0), (2, 3, 5, 7, 1), (2, 9, 256, 256, 0), (2, 9, 256, 256, 1)]
# (n, pos_weight, variant)
BCE_CASES = [(n, pw, v) for n in (1, 5000, 262144 + 257) for pw in (1.0, 15.0) for v in ("full", "noweight", "nodz", "nopx")]
# (n, variant): hp = device hyper-parameters, host = hp_dev NULL, wd = weight decay 1e-2, gscale = gradients times 1 / 1024
ADAM_CASES = [(n, v) for n in (1, 4097, 1048576 + 257) for v in ("hp", "host", "wd", "gscale")]
MASK_CASES = [(hw, v) for hw in (7, 4096, 8192 + 37) for v in ("all", "nopred", "nopb", "nodiff", "nocount")]
CLS_CASES = [(130, 64, 64), (130, 50, 70)]


# ---- host side (no device): the queries and chain counts
def fin_form(nrows, C_, scratch, training=1):
    return _lib.load().sc_bn_finalize_form(nrows, C_, int(scratch), int(training))


def rows32_form(nrows, C_, scratch):
    return _lib.load().sc_bn_bwd_rows32_form(nrows, C_, int(scratch))


def vec_form(HW, aligned=True):
    return _lib.load().sc_ew_vec_form(HW, int(aligned))


def fin_regime(form, nrows):
    """'loop' when the eight-loads-in-flight loop of k_bn_finalize<NW> runs (nrows > 7 x 64 NW), else 'tail'; PRE64 sums 64 rows"""
    nt = {FIN_ROWS4: 256, FIN_ROWS16: 1024}.get(form)
    return "loop" if nt is not None and nrows > 7 * nt else "tail"


def small_regime(N, HW, vec):
    """k_bn_bwd_small: 'scalar', or for the float4 form 'loop' (four items in flight: N HW / 4 > 768 items) | 'tail'"""
    return "scalar" if not vec else ("loop" if N * HW // 4 > 768 else "tail")


def chain_reduce(HW, vec):
    """k_bn_bwd_reduce: 256 threads share a 4096-chunk: 4 elements per 1024 (float4 form) or one per 256 (scalar form)"""
    n = min(HW, 4096)
    return 4 * -(-n // 1024) if vec else -(-n // 256)


def chain_small(N, HW, vec):
    """k_bn_bwd_small: the fp32 partial sums restart per unrolled pass (4 float4 items), per tail item, per plane (scalar form)"""
    return {"scalar": -(-HW // 256), "loop": 16, "tail": 4}[small_regime(N, HW, vec)]


def _flags(flags):
    return set(flags.split())


def f32(v):
    """the float64 value of v rounded to fp32, as a C float argument is"""
    return float(torch.tensor(v, dtype=torch.float64).float())


# ---- inputs and float64 references (CPU).  Each *_ref returns (inputs, checks); checks: name -> (reference, bound, mutated reference or
# None).  The mutated reference is what a kernel with one realistic defect would give; the host test asserts that it violates the bound.
MOMENTUM, EPS = 0.1, 1e-5


@functools.lru_cache(maxsize=2)
def bn_fin_ref(case):
    form, nrows, C_, scratch, flags = case
    fl = _flags(flags)
    training = form != FIN_EVAL
    gamma, beta = rnd(C_, seed=2) * 0.2 + 1, rnd(C_, seed=3) * 0.5 + 1.0
    gamma[0], beta[-1] = -gamma[0], -beta[-1].abs()
    rm, rv = rnd(C_, seed=4) * 0.1, rnd(C_, seed=5).abs() + 0.5
    mom, eps = f32(MOMENTUM), f32(EPS)
    rows, count = None, 1.0
    if training:
        count = 1.0 if "count1" in fl else 8.0 * nrows
        rows = torch.stack((rnd(nrows, C_, seed=6) + 0.3, rnd(nrows, C_, seed=7) ** 2 + 1.0), dim=2)      # column 0: mixed signs
        if "count1" in fl:
            x = rnd(C_, seed=8) * 2
            rows = torch.stack((x, x * x), dim=1)[None]
        if "negvar" in fl:
            rows[:, 1, 0], rows[:, 1, 1], count = 2.0, 3.9, float(nrows)
        r = rows.double()
        S, A = r.sum(0), r.abs().sum(0)
        mean = S[:, 0] / count
        var_raw = S[:, 1] / count - mean * mean
        if "negvar" in fl:
            assert float(var_raw[1]) < -0.05
        k = (nrows + 8) * D
        e1 = k * A[:, 0] / count
        ev = k * A[:, 1] / count + 2 * mean.abs() * e1 + 4 * D * (S[:, 1].abs() / count + mean * mean)
        var = var_raw.clamp_min(0)
    else:
        mean, var = rm.double(), rv.double()
        e1 = ev = torch.zeros(C_, dtype=torch.float64)
    invstd = 1 / torch.sqrt(var + eps)
    dinv = 0.5 * invstd ** 3 * ev + 4 * D * invstd
    g, b = gamma.double(), beta.double()
    scale = g * invstd
    shift = b - mean * scale
    cst = torch.zeros(C_, SC_CST, dtype=torch.float64)
    cst[:, 0], cst[:, 1], cst[:, 2], cst[:, 3] = scale, shift, mean, invstd
    bs = g.abs() * (2 * U * invstd + dinv) * (1 + 2 * U)
    ms = (mean * scale).abs()
    eb = torch.zeros_like(cst)
    eb[:, 0] = bs
    eb[:, 1] = (4 * U * ms + U * (b.abs() + ms) + mean.abs() * g.abs() * dinv + scale.abs() * e1) * (1 + 4 * U)
    eb[:, 2] = U * mean.abs() + e1
    eb[:, 3] = U * invstd + dinv
    checks = {"cst": (cst, eb, None)}
    if training:
        unb = var * count / (count - 1) if count > 1 else var
        new_rm, new_rv = (1 - mom) * rm.double() + mom * mean, (1 - mom) * rv.double() + mom * unb
        checks["running_mean"] = (new_rm, U * new_rm.abs() + mom * e1 + 4 * D * new_rm.abs(), None)
        checks["running_var"] = (new_rv, U * new_rv.abs() + mom * ev * 2 + 4 * D * new_rv.abs(), (1 - mom) * rv.double() + mom * var)
        bound = float((g.abs() * math.sqrt(count - 1) + b.abs()).max())
        checks["act_bound"] = (torch.tensor([bound], dtype=torch.float64), None, None)
    else:
        checks["running_mean"] = (rm.double(), torch.zeros(C_, dtype=torch.float64), None)
        checks["running_var"] = (rv.double(), torch.zeros(C_, dtype=torch.float64), None)
    return dict(rows=rows, count=count, gamma=gamma, beta=beta, rm=rm, rv=rv), checks


def make_bn_input(N, C_, HW, act, seed):
    """g, y and the forward constants of a BatchNorm'd tensor; y moved off the thresholds of the activation"""
    g = rnd(N, C_, HW, 1, seed=seed)
    sc, sh = rnd(C_, seed=seed + 1) * 0.3 + 1.0, rnd(C_, seed=seed + 2) * 0.5 + 1.0
    sc[0] = -sc[0]
    mean, invstd = rnd(C_, seed=seed + 3) * 0.2 + 1.0, rnd(C_, seed=seed + 4).abs() + 0.5
    y = _off_threshold(rnd(N, C_, HW, 1, seed=seed + 5) * 2.0 + 1.0, sc, sh)
    cst = torch.zeros(C_, SC_CST)
    cst[:, 0], cst[:, 1], cst[:, 2], cst[:, 3] = sc, sh, mean, invstd
    yh = y.double() * _bc(sc.double()) + _bc(sh.double())
    lo, hi = (-math.inf if act == ACT_NONE else 0.0), (6.0 if act == ACT_RELU6 else math.inf)
    live = (yh > lo) & (yh < hi)
    acted = yh if act == ACT_NONE else (yh.clamp(0, 6) if act == ACT_RELU6 else yh.clamp_min(0))
    return dict(g=g, y=y, cst=cst, yh=yh, live=live, acted=acted)


def bwd_const_checks(S, eS, Sm, cst, count):
    """dbeta, dgamma and cst_bwd from the two sums S [C][2] known to within eS; Sm: the sums of the defective kernel"""
    c = cst.double()
    scale, shift, mean, invstd = c[:, 0], c[:, 1], c[:, 2], c[:, 3]

    def consts(s):
        o = torch.zeros(s.shape[0], SC_CST, dtype=torch.float64)
        c1, c2 = s[:, 0] / count, s[:, 1] / count
        o[:, 0], o[:, 1], o[:, 2] = scale, shift, scale
        o[:, 3] = -scale * c2 * invstd
        o[:, 4] = -scale * c1 + scale * c2 * invstd * mean
        return o
    ref = consts(S)
    eb = torch.zeros_like(ref)
    e1, e2 = eS[:, 0] / count, eS[:, 1] / count
    eb[:, 3] = (scale * invstd).abs() * e2 + (U + 8 * D) * ref[:, 3].abs()
    eb[:, 4] = (scale.abs() * e1 + (scale * invstd * mean).abs() * e2 + U * ref[:, 4].abs()
                + 8 * D * ((scale * S[:, 0]).abs() + (scale * S[:, 1] * invstd * mean).abs()) / count)
    return {"dbeta": (S[:, 0], eS[:, 0] + U * S[:, 0].abs(), Sm[:, 0]), "dgamma": (S[:, 1], eS[:, 1] + U * S[:, 1].abs(), Sm[:, 1]),
            "cst_bwd": (ref, eb, consts(Sm))}


def _bn_bwd_checks(N, C_, HW, act, n, rows, chunk):
    """the checks of one BatchNorm-backward case with chain n; the defect drops the last float4 of every chunk of `chunk` elements"""
    d = make_bn_input(N, C_, HW, act, seed=31)
    zero = torch.zeros((), dtype=torch.float64)
    gb = torch.where(d["live"], d["g"].double(), zero)
    c = d["cst"].double()
    xh = (d["y"].double() - _bc(c[:, 2])) * _bc(c[:, 3])
    t = torch.stack((gb, gb * xh), dim=-1)[:, :, :, 0]                      # [N][C][HW][2]
    S, A = t.sum((0, 2)), t.abs().sum((0, 2))
    eS = (n * U + (rows + 512) * D) * A
    eS[:, 1] += 2 * U * A[:, 1] * (1 + 2 * U)
    keep = torch.ones(HW, dtype=torch.bool)
    for end in list(range(chunk, HW, chunk)) + [HW]:
        keep[max(end - 4, 0):end] = False
    Sm = t[:, :, keep].sum((0, 2))
    checks = {"sums": (S, eS, Sm)}
    checks.update(bwd_const_checks(S, eS, Sm, d["cst"], float(N * HW)))
    amax = (gb.abs().amax((0, 2, 3)) * c[:, 0].abs()).max().reshape(1)
    checks["absmax"] = (amax, 2 * U * amax, None)
    aa = d["yh"].abs().max().reshape(1)
    aa = aa.clamp_max(6.0) if act == ACT_RELU6 else aa
    checks["act_absmax"] = (aa, 2 * U * aa, None)
    checks["act_floor"] = (d["acted"].abs().max().float().double().reshape(1), None, None)      # the record may not be below this
    return d, checks


@functools.lru_cache(maxsize=2)
def bn_reduce_ref(case):
    form, N, C_, HW, act, flags = case
    return _bn_bwd_checks(N, C_, HW, act, chain_reduce(HW, form == EW_VEC4), N * -(-HW // 4096), 4096)


@functools.lru_cache(maxsize=2)
def bn_small_ref(case):
    form, N, C_, HW, act, flags = case
    return _bn_bwd_checks(N, C_, HW, act, chain_small(N, HW, form == EW_VEC4), 1, HW)


@functools.lru_cache(maxsize=2)
def bn_rows32_ref(case):
    form, nrows, C_, scratch = case
    rows = torch.stack((rnd(nrows, C_, seed=51), rnd(nrows, C_, seed=52) * 2 + 0.1), dim=2)
    cst = torch.zeros(C_, SC_CST)
    cst[:, 0], cst[:, 1], cst[:, 2], cst[:, 3] = rnd(C_, seed=53) * 0.3 + 1, rnd(C_, seed=54), rnd(C_, seed=55) * 0.2 + 1, rnd(C_, seed=56).abs() + 0.5
    r = rows.double()
    S, eS = r.sum(0), (nrows + 512) * D * r.abs().sum(0)
    return dict(rows=rows, cst=cst, count=32.0 * nrows), bwd_const_checks(S, eS, r[:-1].sum(0), cst, 32.0 * nrows)


@functools.lru_cache(maxsize=2)
def add_ref(kind):
    N, C_, HW = ADD_SHAPE
    a, b = rnd(N, C_, HW, 1, seed=71, scale=2.0), rnd(N, C_, HW, 1, seed=72)
    z64 = torch.zeros((), dtype=torch.float64)
    ins = dict(a=a, b=b)
    if kind == "record_only":        # max |relu6(BN(a))|, nothing written
        sc, sh = rnd(C_, seed=73) * 0.3 + 1, rnd(C_, seed=74) * 0.5 + 1
        a = _off_threshold(a, sc, sh)
        cst = torch.zeros(C_, SC_CST)
        cst[:, 0], cst[:, 1] = sc, sh
        v = (a.double() * _bc(sc.double()) + _bc(sh.double())).clamp(0, 6)
        ins.update(a=a, b=None, cst_a=cst)
        ref, eb = v, U * v.abs()
    elif kind == "norm+raw":
        off, fac, lo, hi = rnd(C_, seed=73) * 0.1, rnd(C_, seed=74).abs() + 0.5, -1.0, 1.5
        f64 = lambda t: (t.double() - _bc(off.double())) / _bc(fac.double())      # noqa: E731
        near = lambda t: ((f64(t) - lo).abs() < 1e-3) | ((f64(t) - hi).abs() < 1e-3)      # noqa: E731
        a = torch.where(near(a), a + 0.01 * _bc(fac), a)
        assert not bool(near(a).any())
        cst = torch.zeros(C_, SC_CST)
        cst[:, 0], cst[:, 1], cst[:, 2], cst[:, 3] = off, fac, lo, hi
        raw = f64(a)
        vn = raw.clamp(lo, hi)
        ins.update(a=a, cst_a=cst)
        ref = vn + b.double()
        eb = U * (torch.where(raw == vn, 2 * vn.abs(), z64) + ref.abs()) * (1 + 4 * U)
    else:
        act = ACT_NONE if kind.endswith("none") else ACT_RELU
        sc, sh = rnd(C_, seed=73) * 0.3 + 1, rnd(C_, seed=74) * 0.5 + 1
        y = _off_threshold(rnd(N, C_, HW, 1, seed=75) * 2 + 1, sc, sh)
        cst = torch.zeros(C_, SC_CST)
        cst[:, 0], cst[:, 1], cst[:, 2], cst[:, 3], cst[:, 4] = sc, sh, rnd(C_, seed=76), rnd(C_, seed=77) * 0.1, rnd(C_, seed=78) * 0.1
        yh = y.double() * _bc(sc.double()) + _bc(sh.double())
        gm = b.double() if act == ACT_NONE else torch.where(yh > 0, b.double(), z64)
        inner = y.double() * _bc(cst[:, 3].double()) + _bc(cst[:, 4].double())
        v = gm * _bc(cst[:, 2].double()) + inner
        ins.update(y=y, cst_b=cst, act=act)
        ref = a.double() + v
        eb = U * (inner.abs() + v.abs() + ref.abs()) * (1 + 4 * U)
    mutated = ref.clone()
    mutated[:, :, 2044:2048] = 0          # a chunk's last float4 never written
    return ins, {"out": (ref, eb, mutated)}


def make_dyadic(mode, N, C_, H, W, seed):
    """x on a grid of 1/8 in [-4, 4), scale a power of two, shift a multiple of 1/8: the prologue is exact in fp32.  ReLU6 clamps whole
    windows to 0 or 6 (scale 4): ties are plentiful"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-32, 32, (N, C_, H, W), generator=g).float() / 8
    if mode == "raw":
        return dict(x=x, cst=None, mode=SRC_RAW, actc=ACT_NONE, v=x.double())
    sc = torch.tensor([4.0, 2.0, 0.5, 1.0, 8.0])[torch.arange(C_) % 5]
    sh = torch.randint(-8, 9, (C_,), generator=g).float() / 8
    cst = torch.zeros(C_, SC_CST)
    cst[:, 0], cst[:, 1] = sc, sh
    pre = x.double() * _bc(sc.double()) + _bc(sh.double())
    actc = ACT_RELU6 if mode == "affine6" else ACT_RELU
    return dict(x=x, cst=cst, mode=SRC_AFFINE, actc=actc, v=pre.clamp(0, 6) if actc == ACT_RELU6 else pre.clamp_min(0))


def pool_windows(v):
    """[N][C][Ho][Wo][4]: the 2x2 windows in row-major order"""
    N, C_, H, W = v.shape
    return v.reshape(N, C_, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C_, H // 2, W // 2, 4)


def pool_scatter(best, gp):
    """gin of a pool backward that sends gp to window element `best`"""
    N, C_, Ho, Wo = gp.shape
    w = torch.zeros(N, C_, Ho, Wo, 4, dtype=gp.dtype)
    w.scatter_(4, best[..., None], gp[..., None])
    return w.reshape(N, C_, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C_, 2 * Ho, 2 * Wo)


@functools.lru_cache(maxsize=2)
def pool_ref(case):
    mode, Ho, Wo = case
    N, C_ = 2, 3
    xin = make_dyadic(mode, N, C_, 2 * Ho, 2 * Wo, seed=81)
    g = torch.Generator().manual_seed(82)
    gp = torch.randint(-32, 32, (N, C_, Ho, Wo), generator=g).double() / 8
    gin0 = torch.randint(-32, 32, (N, C_, 2 * Ho, 2 * Wo), generator=g).double() / 8
    win = pool_windows(xin["v"])
    first = torch.zeros(win.shape[:-1], dtype=torch.long)
    last = torch.zeros_like(first)
    for k in range(1, 4):
        vk = win[..., k]
        first = torch.where(vk > win.gather(4, first[..., None])[..., 0], torch.full_like(first, k), first)
        last = torch.where(vk >= win.gather(4, last[..., None])[..., 0], torch.full_like(last, k), last)
    zero = torch.zeros_like(gp)
    return (xin, gp, gin0), {"out": (F.max_pool2d(xin["v"], 2), zero, None),
                             "gin": (pool_scatter(first, gp), torch.zeros_like(gin0), pool_scatter(last, gp)),
                             "ties": (((win == win.amax(4, keepdim=True)).sum(4) > 1).double().mean().reshape(1), None, None)}


def lerp_matrix(n_in, clamp=True):
    """[2 n_in][n_in + 1] float64 weights of F.interpolate(scale_factor=2, bilinear, align_corners=True) along one axis (the spare
    column collects what an unclamped second tap reads past the end), and the mask of the inputs within 1 + 2 u n_in of the position"""
    n_out = 2 * n_in
    Wm = torch.zeros(n_out, n_in + 1, dtype=torch.float64)
    pos = torch.arange(n_out, dtype=torch.float64) * ((n_in - 1) / (n_out - 1))
    i0 = pos.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1) if clamp else i0 + 1
    l = pos - i0
    Wm[torch.arange(n_out), i0] += 1 - l
    Wm[torch.arange(n_out), i1] += l
    near = (pos[:, None] - torch.arange(n_in, dtype=torch.float64)[None, :]).abs() < 1 + 2 * U * n_in
    return Wm, i0, i1, near.double()


def make_up_input(mode, N, C_, H, W, seed):
    x = rnd(N, C_, H, W, seed=seed, scale=2.0)
    if mode == "raw":
        return dict(x=x, cst=None, mode=SRC_RAW, actc=ACT_NONE, v=x.double())
    sc, sh = rnd(C_, seed=seed + 1) * 0.3 + 1.5, rnd(C_, seed=seed + 2) * 0.5 + 1.0
    x = _off_threshold(x, sc, sh)
    cst = torch.zeros(C_, SC_CST)
    cst[:, 0], cst[:, 1] = sc, sh
    pre = x.double() * _bc(sc.double()) + _bc(sh.double())
    actc = ACT_RELU6 if mode == "affine6" else ACT_RELU
    return dict(x=x, cst=cst, mode=SRC_AFFINE, actc=actc, v=pre.clamp(0, 6) if actc == ACT_RELU6 else pre.clamp_min(0))


@functools.lru_cache(maxsize=2)
def up_ref(case):
    mode, H, W = case
    N, C_ = 2, 3
    xin = make_up_input(mode, N, C_, H, W, seed=91)
    v = xin["v"]
    ref = F.interpolate(v, scale_factor=2, mode="bilinear", align_corners=True)
    Wy, y0, y1, _ = lerp_matrix(H)
    Wx, x0, x1, _ = lerp_matrix(W)
    va = v.abs()
    assert float((torch.einsum("ya,ncab,xb->ncyx", Wy[:, :H], v, Wx[:, :W]) - ref).abs().max()) <= 1e-12 * float(va.max())
    taps = torch.stack([va[:, :, ya][:, :, :, xa] for ya in (y0, y1) for xa in (x0, x1)]).amax(0)
    eb = 2 * U * (H + W) * taps + 8 * U * torch.einsum("ya,ncab,xb->ncyx", Wy[:, :H], va, Wx[:, :W])
    # the defect: the second row tap not clamped; behind a plane lies the next one, behind the last memory that is not the tensor's (NaN)
    # (the weight of that tap is 0 at the last row in exact arithmetic: 0 x the next plane's row changes nothing, 0 x NaN is NaN)
    Wyu, _, y1u, _ = lerp_matrix(H, clamp=False)
    flat = v.reshape(N * C_, H, W)
    behind = torch.cat((flat[1:, 0], torch.full((1, W), float("nan"), dtype=torch.float64))).reshape(N, C_, 1, W)
    rows = torch.einsum("ya,ncab->ncyb", Wyu[:, :H], v) + torch.where((y1u == H)[None, None, :, None], Wyu[:, H][None, None, :, None] * behind,
                                                                      torch.zeros((), dtype=torch.float64))
    mutated = torch.einsum("ncyb,xb->ncyx", rows, Wx[:, :W])
    return xin, {"out": (ref, eb, mutated)}


@functools.lru_cache(maxsize=2)
def up_bwd_ref(case):
    H, W = case
    N, C_ = 2, 3
    gout = rnd(N, C_, 2 * H, 2 * W, seed=95)
    Wy, _, _, By = lerp_matrix(H)
    Wx, _, _, Bx = lerp_matrix(W)
    Wy, Wx = Wy[:, :H], Wx[:, :W]
    g, ga = gout.double(), gout.double().abs()
    tr = lambda a, m, b: torch.einsum("ya,ncyx,xb->ncab", a, m, b)      # noqa: E731
    ref = tr(Wy, g, Wx)
    v = gout.double().requires_grad_(False)
    xin = torch.zeros(N, C_, H, W, dtype=torch.float64, requires_grad=True)
    F.interpolate(xin, scale_factor=2, mode="bilinear", align_corners=True).backward(v)
    assert float((xin.grad - ref).abs().max()) <= 1e-12 * float(ga.max()) * 8
    k = int((Wy != 0).sum(0).max()) + int((Wx != 0).sum(0).max()) + 2
    eb = 2 * U * H * tr(By, ga, Wx) + 2 * U * W * tr(Wy, ga, Bx) + k * U * tr(Wy, ga, Wx)
    # the defect: a gather window one output row short at its far end
    Wyd = Wy.clone()
    for a in range(H):
        nz = (Wy[:, a] != 0).nonzero()
        Wyd[int(nz.max()), a] = 0
    return gout, {"gin": (ref, eb, tr(Wyd, g, Wx))}


@functools.lru_cache(maxsize=2)
def downsum_ref(case):
    N, C_, Ho, Wo, accum = case
    x, out0 = rnd(N, C_, 2 * Ho, 2 * Wo, seed=61), rnd(N, C_, Ho, Wo, seed=62)
    s = (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + (x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2])      # fp32, in the kernel's order
    return (x, out0), out0 + s if accum else s


def bce_inputs(n, seed=1):
    z = rnd(n, seed=seed) * 3
    t = (rnd(n, seed=seed + 1) > 0.5).float()
    w = rnd(n, seed=seed + 2).abs().clamp(0.1, 1)
    sat = torch.tensor([30.0, -30.0, 90.0, -90.0, 104.0, -104.0])
    if n >= 24:       # each saturating logit with both targets, at the front and in the last partial block
        for base in (0, n - 12):
            z[base:base + 12] = sat.repeat(2)
            t[base:base + 12] = torch.tensor([0.0] * 6 + [1.0] * 6)
    else:
        z[0], t[0] = -104.0, 1.0
    return z, t, w


def bce_ref(case, math_k=MEASURED_MATH):
    """float64 loss, gradient and sum with their bounds for the allowance (ke, kl) of the two math calls"""
    n, pw, variant = case
    ke, kl = math_k
    z, t, w = bce_inputs(n)
    if variant == "noweight":
        w = None
    x, y = z.double(), t.double()
    wt = w.double() if w is not None else torch.ones(n, dtype=torch.float64)
    lw = 1 + (f32(pw) - 1) * y
    L = torch.log1p(torch.exp(-x.abs()))
    sp = L + (-x).clamp_min(0)
    l = (1 - y) * x + lw * sp
    sig = torch.sigmoid(x)
    dzr = wt * (lw * sig - f32(pw) * y) / n
    eb_l = U * ((ke + kl) * lw * L + lw * sp + (lw != 1).double() * lw * sp + l.abs()) + lw * TINY
    eb_dz = wt / n * (U * (lw * sig * (ke + 3) + 4 * (lw * sig - f32(pw) * y).abs()) + lw * TINY) * (1 + 8 * U)
    start = 3.25
    tot = (l * wt).sum()
    eb_sum = (eb_l * wt).sum() + U * (l * wt).abs().sum() + (n / 2 ** 18 + 1100) * D * (abs(start) + (l * wt).abs().sum())
    checks = {"loss_px": (l, eb_l, None), "dz": (dzr, eb_dz, None), "loss_sum": ((start + tot).reshape(1), eb_sum.reshape(1), None)}
    return dict(z=z, t=t, w=w, start=start), checks


ADAM = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, steps=4)


def adam_inputs(n):
    p0 = rnd(n, seed=1)
    grads = [rnd(n, seed=10 + i) for i in range(ADAM["steps"])]
    if n >= 64:
        for g in grads:         # exact zeros (denom = eps), tiny, huge and small gradients
            g[0:8], g[8:16], g[16:24], g[24:32] = 0.0, 1e-20 * g[8:16].sign(), 1e4 * g[16:24].sign(), 1e-6 * g[24:32].sign()
        p0[4:8] = 0.0
        p0[28:32] = 0.0
    return p0, grads


def adam_ref(case, decoupled=False, eps_inside=False):
    """m, v, p after four steps in float64 with the bound recurrence of the module docstring -> (inputs, checks)"""
    n, variant = case
    p0, grads = adam_inputs(n)
    wd = f32(1e-2) if variant == "wd" else 0.0
    gs = f32(1.0 / 1024) if variant == "gscale" else 1.0
    lr, b1, b2, eps = f32(ADAM["lr"]), f32(ADAM["b1"]), f32(ADAM["b2"]), f32(ADAM["eps"])
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    dp, dm, dv = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    hps = []
    for t, g32 in enumerate(grads, start=1):
        bc1, bc2s = 1 - b1 ** t, math.sqrt(1 - b2 ** t)
        hps.append((lr, bc1, bc2s))
        g = g32.double() * gs
        dg = U * g.abs()
        if wd and not decoupled:
            g = g + wd * p
            dg = dg + wd * dp + U * g.abs()
        m_new = m + (g - m) * (1 - b1)
        dm = b1 * dm + (1 - b1) * dg + U * (2 * (g - m).abs() * (1 - b1) + m_new.abs())
        v_new = b2 * v + (1 - b2) * g * g
        dv = b2 * dv + (1 - b2) * 2 * g.abs() * dg + U * (b2 * v + 3 * (1 - b2) * g * g + v_new) + 2 * TINY
        m, v = m_new, v_new
        sq = torch.sqrt(v)
        denom = torch.sqrt(v / bc2s ** 2 + eps) if eps_inside else sq / bc2s + eps
        dden = (torch.sqrt(v + dv) - torch.sqrt((v - dv).clamp_min(0))) / bc2s + 3 * U * sq / bc2s + U * denom
        upd = lr / bc1 * m / denom
        dupd = lr / bc1 * dm / denom + upd.abs() * (dden / denom + 6 * U)
        if wd and decoupled:
            p = p * (1 - lr * wd)
        p = p - upd
        dp = dp + dupd + U * p.abs()
    return dict(p0=p0, grads=grads, wd=wd, gs=gs, hps=hps), {"m": (m, dm, None), "v": (v, dv, None), "p": (p, dp, None)}


def mask_inputs(HW, N=3):
    z = rnd(N, HW, seed=1)
    z = torch.where(z.abs() < 1e-3, torch.full_like(z, 1e-3), z)
    z[:, 0::5] = 0.0                                    # logit == 0: ">= 0" true, "sigmoid > .5" false
    t = (rnd(N, HW, seed=2) > 0.3).float()
    t[:, 1::7], t[:, 2::7] = 0.5, 2.0                   # only == 1 counts
    return z, t


def mask_ref(HW, ge0, strict=True):
    z, t = mask_inputs(HW)
    sig = torch.sigmoid(z.double())
    b = (z >= 0) if ge0 else ((sig > 0.5) if strict else (sig >= 0.5))
    b = b.long()
    return (z, t), dict(pred=sig, pb=b, diff=2 * b + (t == 1).long(), count=b.sum(1))


def cls_ref(case):
    N, H, W = case
    thr = 10.0 * H * W / 4096.0
    lo, hi = math.floor(thr), math.ceil(thr)
    vals = [0, lo - 1, lo, hi, hi + 1, int(thr) if thr == int(thr) else lo, 10 * H * W, H * W]
    cnt = torch.tensor([vals[i % len(vals)] for i in range(N)], dtype=torch.int64)
    return cnt, (cnt.double() > thr).long(), thr


# ---- the device side
def within(name, got, ref, bound):
    """element-wise |got - ref| <= bound with no NaN left; prints and returns the largest error-to-bound ratio"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
    err = (got - ref).abs()
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    print(f"EWRATIO {name} {ratio:.4f}")
    bad = err > bound
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements outside the bound, worst ratio {ratio:.3f}, first at {bad.nonzero()[0].tolist()}"
    return ratio


def _id(case):
    return "-".join(str(v) for v in case).replace(" ", "+").rstrip("-") if isinstance(case, tuple) else str(case)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _src(d, C_, offset=False):
    return make_src(dev_at(d["x"], offset), C_, d["mode"], act=d["actc"], cst=dev(d["cst"]) if d["cst"] is not None else None)


def run_bn_finalize(lib, case):
    form, nrows, C_, scratch, flags = case
    training = form != FIN_EVAL
    assert fin_form(nrows, C_, scratch, training) == form
    ins, checks = bn_fin_ref(case)
    name = f"bn_finalize {_id(case)}"
    scr = _nan(64 * 2 * C_, dtype=torch.float64) if scratch else None
    gd, bd = dev(ins["gamma"]), dev(ins["beta"])
    rows = dev(ins["rows"]) if training else None
    want_b = float(checks["act_bound"][0]) if training else 0.0
    for start in (0.0, f32(2.0 * want_b + 1.0)):         # the record: raised from 0, left alone when it starts higher
        rm, rv, cst, slot = dev(ins["rm"]), dev(ins["rv"]), _nan(C_, SC_CST), torch.tensor([start], device=DEV)
        check(lib.sc_bn_finalize(ptr(rows), nrows, ins["count"], ptr(gd), ptr(bd), ptr(rm), ptr(rv), MOMENTUM, EPS, int(training),
                                 ptr(cst), C_, ptr(scr), ptr(slot), stream()))
        within(name + " cst", cst, *checks["cst"][:2])
        within(name + " running_mean", rm, *checks["running_mean"][:2])
        within(name + " running_var", rv, *checks["running_var"][:2])
        got = float(slot)
        if training and start == 0.0:
            print(f"EWRATIO {name} act_bound {(got / want_b - 1) / (4 * U) if want_b else 0.0:.4f}")
            assert want_b <= got <= want_b * (1 + 4 * U), (got, want_b)
        else:
            assert got == start
    if training:      # without the record: the same constants
        rm2, rv2, cst2 = dev(ins["rm"]), dev(ins["rv"]), _nan(C_, SC_CST)
        check(lib.sc_bn_finalize(ptr(rows), nrows, ins["count"], ptr(gd), ptr(bd), ptr(rm2), ptr(rv2), MOMENTUM, EPS, 1, ptr(cst2), C_,
                                 ptr(scr), None, stream()))
        torch.cuda.synchronize()
        assert torch.equal(cst, cst2) and torch.equal(rm, rm2) and torch.equal(rv, rv2)


def _check_records(name, checks, amax, aact):
    within(name + " absmax", amax, *checks["absmax"][:2])
    within(name + " act_absmax", aact, *checks["act_absmax"][:2])
    assert float(aact) >= float(checks["act_floor"][0]), (float(aact), float(checks["act_floor"][0]))


def _records(checks, mode):
    """(absmax, act_absmax) slots: off | from zero | above the result (must stay)"""
    if mode == "off":
        return None, None
    hi = mode == "above"
    return (torch.tensor([2 * float(checks["absmax"][0]) + 1 if hi else 0.0], device=DEV),
            torch.tensor([2 * float(checks["act_absmax"][0]) + 1 if hi else 0.0], device=DEV))


def run_bn_reduce(lib, case):
    form, N, C_, HW, act, flags = case
    off = "offset" in _flags(flags)
    assert vec_form(HW, not off) == form
    d, checks = bn_reduce_ref(case)
    name = f"bn_bwd_reduce {_id(case)}"
    gd, yd, cst = dev_at(d["g"], off), dev_at(d["y"], off), dev(d["cst"])
    nrows = lib.sc_stat_rows(STAT_BNBWD, N, 1, HW)
    first = None
    for mode in ("off", "zero", "above"):
        amax, aact = _records(checks, mode)
        before = (amax.clone(), aact.clone()) if amax is not None else None
        sums = _nan(nrows, C_, 2, dtype=torch.float64)
        check(lib.sc_bn_bwd_reduce(ptr(gd), ptr(yd), ptr(cst), act, ptr(sums), N, C_, HW, ptr(amax), ptr(aact), stream()))
        within(f"{name} [{mode}] sums", sums.sum(0), *checks["sums"][:2])
        dg, db, cb = _nan(C_), _nan(C_), _nan(C_, SC_CST)
        check(lib.sc_bn_bwd_finalize(ptr(sums), nrows, float(N * HW), ptr(cst), ptr(dg), ptr(db), ptr(cb), C_, stream()))
        within(f"{name} [{mode}] dgamma", dg, *checks["dgamma"][:2])
        within(f"{name} [{mode}] dbeta", db, *checks["dbeta"][:2])
        within(f"{name} [{mode}] cst_bwd", cb, *checks["cst_bwd"][:2])
        if mode == "zero":
            _check_records(name, checks, amax, aact)
        elif mode == "above":
            assert torch.equal(amax, before[0]) and torch.equal(aact, before[1])
        first = sums if first is None else first
        assert torch.equal(first, sums)         # the records change nothing else


def run_bn_small(lib, case):
    form, N, C_, HW, act, flags = case
    off = "offset" in _flags(flags)
    assert vec_form(HW, not off) == form
    d, checks = bn_small_ref(case)
    name = f"bn_bwd_small {_id(case)} {small_regime(N, HW, form == EW_VEC4)}"
    gd, yd, cst = dev_at(d["g"], off), dev_at(d["y"], off), dev(d["cst"])
    first = None
    for mode in ("off", "zero", "above"):
        amax, aact = _records(checks, mode)
        before = (amax.clone(), aact.clone()) if amax is not None else None
        dg, db, cb = _nan(C_), _nan(C_), _nan(C_, SC_CST)
        check(lib.sc_bn_bwd_small(ptr(gd), ptr(yd), ptr(cst), act, N, C_, HW, ptr(dg), ptr(db), ptr(cb), ptr(amax), ptr(aact), stream()))
        within(f"{name} [{mode}] dgamma", dg, *checks["dgamma"][:2])
        within(f"{name} [{mode}] dbeta", db, *checks["dbeta"][:2])
        within(f"{name} [{mode}] cst_bwd", cb, *checks["cst_bwd"][:2])
        if mode == "zero":
            _check_records(name, checks, amax, aact)
        elif mode == "above":
            assert torch.equal(amax, before[0]) and torch.equal(aact, before[1])
        first = (dg, db, cb) if first is None else first
        assert all(torch.equal(a, b) for a, b in zip(first, (dg, db, cb)))
    # dgamma / dbeta are optional
    cb2 = _nan(C_, SC_CST)
    check(lib.sc_bn_bwd_small(ptr(gd), ptr(yd), ptr(cst), act, N, C_, HW, None, None, ptr(cb2), None, None, stream()))
    torch.cuda.synchronize()
    assert torch.equal(cb2, first[2])


def run_bn_rows32(lib, case):
    form, nrows, C_, scratch = case
    assert rows32_form(nrows, C_, scratch) == form
    ins, checks = bn_rows32_ref(case)
    name = f"bn_bwd_finalize_rows32 {_id(case)}"
    scr = _nan(64 * 2 * C_, dtype=torch.float64) if scratch else None
    dg, db, cb = _nan(C_), _nan(C_), _nan(C_, SC_CST)
    check(lib.sc_bn_bwd_finalize_rows32(ptr(dev(ins["rows"])), nrows, ins["count"], ptr(dev(ins["cst"])), ptr(dg), ptr(db), ptr(cb), C_,
                                        ptr(scr), stream()))
    within(name + " dgamma", dg, *checks["dgamma"][:2])
    within(name + " dbeta", db, *checks["dbeta"][:2])
    within(name + " cst_bwd", cb, *checks["cst_bwd"][:2])


def run_add(lib, case):
    form, kind = case
    N, C_, HW = ADD_SHAPE
    off = form == EW_SCALAR
    assert vec_form(HW, not off) == form
    ins, checks = add_ref(kind)
    name = f"add_srcs {_id(case)}"
    ref, eb, _ = checks["out"]
    if kind == "record_only":
        sa, sb = make_src(dev_at(ins["a"], off), C_, SRC_AFFINE, act=ACT_RELU6, cst=dev(ins["cst_a"])), None
    elif kind == "norm+raw":
        sa, sb = make_src(dev_at(ins["a"], off), C_, SRC_NORM, cst=dev(ins["cst_a"])), make_src(dev_at(ins["b"], off), C_, SRC_RAW)
    else:
        sa = make_src(dev_at(ins["a"], off), C_, SRC_RAW)
        sb = make_src(dev_at(ins["b"], off), C_, SRC_BNBWD, act=ins["act"], cst=dev(ins["cst_b"]), aux=dev_at(ins["y"], off))
    out = dev_at(torch.empty(N, C_, HW, 1), off, fill=float("nan"))
    amax = torch.zeros(1, device=DEV)
    check(lib.sc_add_srcs_absmax(C.byref(sa), C.byref(sb) if sb is not None else None, ptr(out), N, C_, HW, ptr(amax), stream()))
    within(name + " out", out, ref, eb)
    assert float(amax) == float(out.abs().max())
    # the record alone: nothing written, the same maximum; and a record that starts higher stays
    for start in (0.0, f32(2 * float(amax) + 1)):
        rec = torch.tensor([start], device=DEV)
        check(lib.sc_add_srcs_absmax(C.byref(sa), C.byref(sb) if sb is not None else None, None, N, C_, HW, ptr(rec), stream()))
        assert float(rec) == (float(amax) if start == 0.0 else start)
    if kind != "record_only":       # without the record: the same output
        out2 = dev_at(torch.empty(N, C_, HW, 1), off, fill=float("nan"))
        check(lib.sc_add_srcs(C.byref(sa), C.byref(sb), ptr(out2), N, C_, HW, stream()))
        torch.cuda.synchronize()
        assert torch.equal(out, out2)


def run_pool(lib, case):
    mode, Ho, Wo = case
    N, C_ = 2, 3
    (xin, gp, gin0), checks = pool_ref(case)
    print(f"EWRATIO pool {_id(case)} windows with a tie: {float(checks['ties'][0]):.3f}")
    src = _src(xin, C_)
    out = _nan(N, C_, Ho, Wo)
    check(lib.sc_maxpool2x2(C.byref(src), ptr(out), N, C_, Ho, Wo, stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.double().cpu(), checks["out"][0])
    gpd = dev(gp.float())
    for accum in (0, 1):
        gin = dev(gin0.float()) if accum else _nan(N, C_, 2 * Ho, 2 * Wo)
        check(lib.sc_maxpool2x2_bwd(C.byref(src), ptr(gpd), ptr(gin), accum, N, C_, Ho, Wo, stream()))
        torch.cuda.synchronize()
        assert torch.equal(gin.double().cpu(), checks["gin"][0] + (gin0 if accum else 0))


def run_up(lib, case):
    mode, H, W = case
    N, C_ = 2, 3
    xin, checks = up_ref(case)
    out = _nan(N, C_, 2 * H, 2 * W)
    check(lib.sc_upsample_bilinear2x(C.byref(_src(xin, C_)), ptr(out), N, C_, H, W, stream()))
    within(f"upsample {_id(case)} out", out, *checks["out"][:2])


def run_up_bwd(lib, case):
    H, W = case
    N, C_ = 2, 3
    gout, checks = up_bwd_ref(case)
    gin = _nan(N, C_, H, W)
    check(lib.sc_upsample_bilinear2x_bwd(ptr(dev(gout)), ptr(gin), N, C_, H, W, stream()))
    within(f"upsample_bwd {_id(case)} gin", gin, *checks["gin"][:2])


def run_downsum(lib, case):
    N, C_, Ho, Wo, accum = case
    (x, out0), ref = downsum_ref(case)
    out = dev(out0) if accum else _nan(N, C_, Ho, Wo)
    check(lib.sc_downsum2x2(ptr(dev(x)), ptr(out), accum, N, C_, Ho, Wo, stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)


@functools.lru_cache(maxsize=1)
def math_allowance():
    """twice the worst relative error, in units of u, of torch's fp32 exp and log1p on the GPU over the arguments the loss cases use
    (results in the normal range), against float64"""
    zs = torch.cat([bce_inputs(n)[0] for n in sorted({c[0] for c in BCE_CASES})])
    a = dev(-zs.abs())
    t32 = torch.exp(a)
    t64 = torch.exp(a.double())
    ok = t64 > 2 * TINY
    ke = float(((t32.double() - t64).abs() / t64)[ok].max()) / U
    l32 = torch.log1p(t32)
    l64 = torch.log1p(t32.double())
    ok = l64 > 2 * TINY
    kl = float(((l32.double() - l64).abs() / l64)[ok].max()) / U
    print(f"EWRATIO measured math error in u: exp {ke:.3f} log1p {kl:.3f}")
    return 2 * ke, 2 * kl


def run_bce(lib, case):
    n, pw, variant = case
    k = math_allowance()
    assert k[0] <= 8 and k[1] <= 8, k          # a math library this far off would be a finding of its own
    ins, checks = bce_ref(case, k)
    name = f"bce {_id(case)}"
    for key in ("loss_px", "loss_sum"):        # the condition: no looser than test_bce_loss_and_grad
        ref, eb, _ = checks[key]
        scale = n if key == "loss_sum" else 1
        assert bool((eb / scale <= 1e-5 * (ref.abs() / scale).clamp_min(1.0)).all()), key
    acc = torch.tensor([ins["start"]], dtype=torch.float64, device=DEV)
    dz = None if variant == "nodz" else _nan(n)
    px = None if variant == "nopx" else _nan(n)
    wd = dev(ins["w"]) if ins["w"] is not None else None
    check(lib.sc_bce_logits_weighted(ptr(dev(ins["z"])), ptr(dev(ins["t"])), ptr(wd), pw, n, ptr(acc), ptr(dz), ptr(px), stream()))
    within(name + " loss_sum", acc, *checks["loss_sum"][:2])
    if px is not None:
        within(name + " loss_px", px, *checks["loss_px"][:2])
    if dz is not None:
        within(name + " dz", dz, *checks["dz"][:2])


def run_adam(lib, case):
    n, variant = case
    ins, checks = adam_ref(case)
    name = f"adam {_id(case)}"
    p, m, v = dev(ins["p0"]), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    step, lr_d, hp = torch.zeros(1, dtype=torch.int64, device=DEV), torch.full((1,), ADAM["lr"], device=DEV), _nan(4)
    for t, g in enumerate(ins["grads"], start=1):
        lr, bc1, bc2s = ins["hps"][t - 1]
        if variant == "host":
            check(lib.sc_adam_step(ptr(p), ptr(dev(g)), ptr(m), ptr(v), n, lr, ADAM["b1"], ADAM["b2"], ADAM["eps"], ins["wd"], bc1, bc2s, ins["gs"],
                                   None, stream()))
            continue
        check(lib.sc_adam_prepare(ptr(step), ptr(lr_d), ADAM["b1"], ADAM["b2"], ptr(hp), stream()))
        assert int(step) == t
        want = torch.tensor([lr, bc1, bc2s], dtype=torch.float64)
        within(f"{name} hp step {t}", hp[:3], want, U * want)
        # the host values passed next to hp_dev are not looked at
        check(lib.sc_adam_step(ptr(p), ptr(dev(g)), ptr(m), ptr(v), n, 0.0, ADAM["b1"], ADAM["b2"], ADAM["eps"], ins["wd"], 1.0, 1.0, ins["gs"],
                               ptr(hp), stream()))
    for key, t in (("m", m), ("v", v), ("p", p)):
        within(f"{name} {key}", t, *checks[key][:2])


def run_masks(lib, case):
    HW, variant = case
    N = 3
    ke = math_allowance()[0]
    for ge0 in (0, 1):
        (z, t), ref = mask_ref(HW, ge0)
        pred = None if variant == "nopred" else _nan(N, HW)
        pb = None if variant == "nopb" else torch.full((N, HW), -7, dtype=torch.int64, device=DEV)
        df = None if variant == "nodiff" else torch.full((N, HW), -7, dtype=torch.int64, device=DEV)
        start = torch.tensor([5, 0, 1 << 40], dtype=torch.int64)
        cnt = None if variant == "nocount" else dev(start)
        tgt = dev(t) if (df is not None or variant == "all") else None
        check(lib.sc_threshold_masks(ptr(dev(z)), ptr(tgt), ge0, ptr(pred), ptr(pb), ptr(df), ptr(cnt), N, HW, stream()))
        torch.cuda.synchronize()
        if pb is not None:
            assert torch.equal(pb.cpu(), ref["pb"])
        if df is not None:
            assert torch.equal(df.cpu(), ref["diff"])
        if cnt is not None:
            assert torch.equal(cnt.cpu(), start + ref["count"])
        if pred is not None:
            within(f"masks {_id(case)} ge0={ge0} prediction", pred, ref["pred"], (ke + 2) * U * ref["pred"] + TINY)


def run_cls(lib, case):
    N, H, W = case
    cnt, ref, thr = cls_ref(case)
    cls = torch.full((N,), -7, dtype=torch.int64, device=DEV)
    check(lib.sc_pred_classification(ptr(dev(cnt)), ptr(cls), N, H, W, stream()))
    torch.cuda.synchronize()
    assert torch.equal(cls.cpu(), ref)


@pytest.mark.parametrize("case", BN_FIN_CASES, ids=_id)
def test_bn_finalize_variant(hip, case):
    run_bn_finalize(hip, case)


@pytest.mark.parametrize("case", BN_REDUCE_CASES, ids=_id)
def test_bn_bwd_reduce_variant(hip, case):
    run_bn_reduce(hip, case)


@pytest.mark.parametrize("case", BN_SMALL_CASES, ids=_id)
def test_bn_bwd_small_variant(hip, case):
    run_bn_small(hip, case)


@pytest.mark.parametrize("case", BN_ROWS32_CASES, ids=_id)
def test_bn_bwd_finalize_rows32_variant(hip, case):
    run_bn_rows32(hip, case)


@pytest.mark.parametrize("case", ADD_CASES, ids=_id)
def test_add_srcs_variant(hip, case):
    run_add(hip, case)


@pytest.mark.parametrize("case", POOL_CASES, ids=_id)
def test_maxpool_and_backward(hip, case):
    run_pool(hip, case)


@pytest.mark.parametrize("case", UP_CASES, ids=_id)
def test_upsample_bilinear(hip, case):
    run_up(hip, case)


@pytest.mark.parametrize("case", UP_BWD_CASES, ids=_id)
def test_upsample_bilinear_backward(hip, case):
    run_up_bwd(hip, case)


@pytest.mark.parametrize("case", DOWNSUM_CASES, ids=_id)
def test_downsum(hip, case):
    run_downsum(hip, case)


@pytest.mark.parametrize("case", BCE_CASES, ids=_id)
def test_bce_variant(hip, case):
    run_bce(hip, case)


@pytest.mark.parametrize("case", ADAM_CASES, ids=_id)
def test_adam_variant(hip, case):
    run_adam(hip, case)


@pytest.mark.parametrize("case", MASK_CASES, ids=_id)
def test_threshold_masks_variant(hip, case):
    run_masks(hip, case)


@pytest.mark.parametrize("case", CLS_CASES, ids=_id)
def test_pred_classification(hip, case):
    run_cls(hip, case)
