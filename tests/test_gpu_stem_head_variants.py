"""Every launch form of the stem and head kernels (the non-depthwise half of conv_valu.hip) against float64, element by element.

sc_stem_conv_fwd picks k_stem_fwd4m | k_stem_fwd<4> | k_stem_fwd<8> | k_stem_fwd16 (host query sc_stem_fwd_kernel), sc_stem_conv_wgrad
picks k_stem_wgrad<3 | 5> (sc_stem_wgrad_njb) on min(tiles, 1024) work-groups (sc_stem_wgrad_rows) whose partial rows take zero, one
or two k_reduce16 levels before the final sum, sc_head_conv_fwd picks k_head_fwd<0> | k_head_fwd16 | k_head_fwd16v (sc_head_fwd_kernel),
and sc_head_conv_bwd runs k_head_bwd16<BNS> on sc_head_bwd_bn_rows work-groups.  The launchers dispatch on those functions.  Every case
names the code it was written for and asserts it through the query before it launches; tests/test_stem_head_variants_host.py holds
the tables below to the full set of codes and checks on the CPU that every bound is tight enough to see a one-pixel shift, which is
why the tables, the chain counts and the references sit at module level and touch no device.

References: the same op sequence in float64 on the CPU from the same fp32 inputs -- F.conv2d of the prologue'd input and its
gradients, the prologue formed as sc_pro_affine, sc_pro_bnbwd and the NORM clamp form it.  Bounds are derived, not measured, and hold
element by element (u = 2^-24):
  forward         |out - ref| <= (9 Cin + 8) u conv(|act(x)|, |w|) + u |bias|     9 Cin FMA roundings, the prologue's, the rest slack
  data gradient   |gin - ref| <= 16 u convT(|dl|, |w|)                            nine FMA roundings
  sums            |s - ref|   <= n u sum |terms| per output, n = the longest fp32 chain of the case (chain_* below) -- filter
                  gradients (terms = (the magnitudes the dy prologue adds up) x |act|), bias gradient, statistics rows and the
                  BatchNorm-backward sums; where the summed values are themselves kernel outputs (statistics, g') what their own
                  element-wise bound allows is added.  Rows are summed over in float64 here, as the consumers do.
  bn_absmax       within 2 u of the float64 max |scale g'|
The masks of ReLU / ReLU6 are discontinuous, so the inputs they are taken from are moved off the thresholds (by 0.01 where a value
lies within 1e-3 of 0 or 6, likewise at the limits of the NORM clamp): no element is excluded from any comparison.  Outputs start as
NaN.  Every case prints its error-to-bound ratios before it asserts."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hip_ops import DEV, dev  # noqa: E402
from starcop_amd import _lib  # noqa: E402
from starcop_amd._lib import (ACT_NONE, ACT_RELU, ACT_RELU6, SC_CST, SRC_AFFINE, SRC_NORM, SRC_RAW, STAT_STEM, check, ptr,
                              stream)  # noqa: E402
from test_gpu_depthwise_variants import OP_WGRAD, _bc, chain_wgrad, dev_at, dw_code, make_dy, src_of  # noqa: E402
from test_gpu_ops import rnd  # noqa: E402

U = 2.0 ** -24
K_MFMA4, K_VALU4, K_VALU8, K_VALU16 = 0, 1, 2, 3       # enum sc_stem_kernel
HK_GENERIC, HK_FWD16, HK_FWD16V = 0, 1, 2              # enum sc_head_kernel
STEM_CO = 32

# ---- case tables.  Input modes: raw | norm (clamp((x - off) / fac, lo, hi)) | affine_relu | affine6; dy modes: raw | affine | bnbwd6
# (BatchNorm backward behind a ReLU6 mask).  Flags: ragged (both axes off the tile, see the host test), offset / offset_in / offset_out
# (that tensor starts 4 bytes past a 16-byte boundary: the 16-byte forms must not be chosen; the shape is that of an aligned case),
# tiny (a 1 x 3 plane), loop (more tiles than work-groups: the only cases outside N <= 3, H <= 40, W <= 72).
# (code of sc_stem_fwd_kernel, N, Cin, Hin, Win, input mode, flags); tile = 8 x 32 outputs
STEM_FWD_CASES = [
    (K_MFMA4, 2, 4, 32, 64, "norm", ""),
    (K_MFMA4, 1, 3, 37, 72, "affine_relu", "ragged"),       # Wout = 36: the last column tile holds 4 columns
    (K_VALU4, 2, 4, 32, 60, "raw", ""),
    (K_VALU4, 3, 1, 37, 69, "norm", "ragged"),
    (K_VALU4, 2, 4, 32, 64, "norm", "offset"),
    (K_VALU4, 1, 2, 1, 3, "affine_relu", "tiny"),
    (K_VALU8, 1, 8, 32, 64, "norm", ""),
    (K_VALU8, 2, 5, 37, 71, "affine_relu", "ragged"),
    (K_VALU8, 1, 6, 16, 40, "raw", ""),
    (K_VALU16, 1, 16, 32, 64, "raw", ""),
    (K_VALU16, 2, 13, 37, 71, "norm", "ragged"),
    (K_VALU16, 1, 9, 1, 3, "affine_relu", "tiny"),
]

# (NJB of sc_stem_wgrad_njb, N, Cin, Hin, Win, (dy mode, input mode), flags); tile = 4 x 32 outputs, one partial row per work-group
STEM_WGRAD_CASES = [
    (3, 1, 4, 16, 64, ("raw", "norm"), ""),                     # 2 rows
    (3, 3, 5, 40, 64, ("bnbwd6", "norm"), ""),                  # 15 rows
    (3, 2, 1, 37, 71, ("bnbwd6", "raw"), "ragged"),             # 20 rows: one k_reduce16 level
    (3, 1, 5, 21, 39, ("affine", "norm"), "ragged"),            # 3 rows
    (3, 33, 4, 64, 256, ("bnbwd6", "norm"), "loop"),            # 1056 tiles on 1024 work-groups: two levels
    (5, 1, 8, 16, 64, ("raw", "norm"), ""),
    (5, 2, 6, 37, 71, ("bnbwd6", "norm"), "ragged"),            # 20 rows
    (5, 3, 8, 37, 69, ("affine", "raw"), "ragged"),             # 30 rows
    (5, 33, 8, 64, 256, ("bnbwd6", "norm"), "loop"),
]

# (code of sc_head_fwd_kernel, N, Cin, H, W, input mode, flags); tiles: 8 x 32 (generic), 16 x 64 (Cin = 16)
HEAD_FWD_CASES = [
    (HK_GENERIC, 2, 5, 16, 32, "raw", ""),
    (HK_GENERIC, 1, 32, 37, 70, "affine_relu", "ragged"),
    (HK_GENERIC, 1, 5, 1, 3, "affine_relu", "tiny"),
    (HK_FWD16, 2, 16, 16, 62, "raw", ""),
    (HK_FWD16, 1, 16, 33, 70, "affine_relu", "ragged"),
    (HK_FWD16, 1, 16, 32, 64, "affine_relu", "offset_in"),
    (HK_FWD16, 1, 16, 32, 64, "affine_relu", "offset_out"),
    (HK_FWD16, 1, 16, 1, 3, "raw", "tiny"),
    (HK_FWD16V, 1, 16, 32, 64, "affine_relu", ""),
    (HK_FWD16V, 3, 16, 37, 68, "raw", "ragged"),                # the last column tile holds 4 columns
]

# (N, Cin, H, W, flags); tile = 8 x 32
HEAD_DGRAD_CASES = [
    (2, 5, 16, 32, ""), (1, 5, 37, 70, "ragged"),
    (1, 16, 8, 64, ""), (3, 16, 33, 35, "ragged"),
    (1, 32, 16, 32, ""), (1, 32, 37, 70, "ragged"),
]

# (N, Cin, H, W, input mode, flags); k_dw_wgrad at stride 1 with dlogits as every channel's dy, min(tiles, 4096 / Cin) work-groups
HEAD_WGRAD_CASES = [
    (2, 5, 16, 32, "raw", ""), (1, 5, 37, 70, "affine_relu", "ragged"),
    (1, 16, 8, 64, "affine_relu", ""), (3, 16, 33, 35, "raw", "ragged"),
    (1, 32, 16, 32, "affine_relu", ""), (1, 32, 37, 70, "affine_relu", "ragged"),
    (65, 32, 32, 16, "affine_relu", "loop"),                    # 130 tiles of 16 x 16 on 4096 / 32 = 128 work-groups
]

# (BNS, N, H, W, input mode, flags), Cin = 16; tile = 32 rows x 64 columns, rows loaded 4 ahead
HEAD_BWD_CASES = [
    (0, 2, 32, 64, "raw", ""),
    (0, 1, 3, 5, "affine_relu", "ragged"),                      # H below the look-ahead
    (0, 1, 33, 70, "affine6", "ragged"),                        # a second row tile of one row, a second column tile of 6 columns
    (0, 1, 36, 64, "raw", "ragged"),                            # a second row tile of exactly the look-ahead
    (0, 129, 256, 8, "raw", "loop"),                            # 1032 tiles on 1024 work-groups
    (1, 2, 32, 64, "affine_relu", ""),
    (1, 1, 3, 5, "affine6", "ragged"),
    (1, 1, 33, 70, "affine_relu", "ragged"),
    (1, 2, 36, 64, "affine6", "ragged"),
    (1, 129, 256, 8, "affine6", "loop"),
]


# ---- host side (no device): the queries, tile counts and chain counts
def _flags(flags):
    return set(flags.split())


def stem_fwd_code(Cin, Win, out_aligned=True):
    return _lib.load().sc_stem_fwd_kernel(Cin, Win, int(out_aligned))


def stem_wgrad_njb(Cin):
    return _lib.load().sc_stem_wgrad_njb(Cin)


def stem_wgrad_rows(N, Hin, Win):
    return _lib.load().sc_stem_wgrad_rows(N, Hin, Win)


def head_fwd_code(Cin, W, in_aligned=True, out_aligned=True):
    return _lib.load().sc_head_fwd_kernel(Cin, W, int(in_aligned), int(out_aligned))


def head_bwd_rows(N, H, W):
    return _lib.load().sc_head_bwd_bn_rows(N, H, W)


def out_size(h):
    return (h - 1) // 2 + 1


def stem_wgrad_tiles(N, Hin, Win):
    return N * -(-out_size(Hin) // 4) * -(-out_size(Win) // 32)


def reduce_levels(rows):
    """k_reduce16 launches of sc_reduce_rows before its final sum of <= 16 rows"""
    n = 0
    while rows > 16:
        rows, n = -(-rows // 16), n + 1
    return n


def chain_stem_wgrad(N, Hin, Win):
    """k_stem_wgrad: a wave's accumulator takes 32 MFMA K terms per tile (8 steps of 4) for every tile its work-group walks, then 3
    additions across the four waves, then 16 per k_reduce16 level (the final sum is one); + 3 for the roundings of a term itself (two
    of the dy prologue, counted against the magnitudes it adds up, and the input prologue's -- the MFMA does not round the product)"""
    rows = stem_wgrad_rows(N, Hin, Win)
    return 32 * -(-stem_wgrad_tiles(N, Hin, Win) // rows) + 3 + 16 * (reduce_levels(rows) + 1) + 3


def chain_stem_stats(code):
    """statistics rows of the stem forward: the VALU forms add 32 lanes in 5 butterfly steps and then 8 half-wave partials; the MFMA
    form adds a lane's 4 pixels in 2 steps (the squares in a chain of 4), a 16-lane row in 4 and four waves in 2"""
    return 4 + 4 + 2 if code == K_MFMA4 else 5 + 8


def head_bwd_tiles(N, H, W):
    return N * -(-H // 32) * -(-W // 64)


def chain_head_bwd(N, H, W):
    """k_head_bwd16: a lane adds one term per row of every tile its work-group walks (rows past H add exact zeros), then the 6 steps
    of the wave sum; k_head_bwd_reduce sums the rows in float64"""
    return min(H, 32) * -(-head_bwd_tiles(N, H, W) // head_bwd_rows(N, H, W)) + 6


def chain_head_wgrad(N, Cin, H, W):
    """sc_head_conv_wgrad: k_dw_wgrad's chain (float64 atomics behind it) + the rounding of the cast to float"""
    return chain_wgrad(dw_code(OP_WGRAD, N, Cin, H, W, 1), N, Cin, H, W, 1) + 1


def chain_head_dbias(N, H, W):
    """k_sum_f32_to_f64: min(512, ceil(px / 4096)) work-groups of 256 threads stride over the pixels, then 6 + 3 steps of the block
    sum, float64 atomics, the cast"""
    npx = N * H * W
    grid = min(512, -(-npx // 4096))
    return -(-npx // (grid * 256)) + 9 + 1


# ---- inputs and float64 references (CPU)
def _off_limits(t, f64_of, limits, step):
    """move the elements of t whose float64 image f64_of(t) lies within 1e-3 of one of `limits` by `step`; none may remain"""
    def near(v):
        p = f64_of(v)
        m = torch.zeros_like(p, dtype=torch.bool)
        for lim in limits:
            m |= (p - lim).abs() < 1e-3
        return m
    t = torch.where(near(t), t + step, t)
    assert not bool(near(t).any())
    return t


def make_in(mode, N, C_, H, W, seed):
    """-> dict(x fp32, cst [C][SC_CST] or None, src mode, act code, act = float64 activated input, live = where the activation passes a
    gradient, scale, xhat = float64 (x - mean) invstd of an AFFINE input)"""
    x = rnd(N, C_, H, W, seed=seed, scale=2.0)
    if mode == "raw":
        return dict(x=x, cst=None, mode=SRC_RAW, actc=ACT_NONE, act=x.double(), live=torch.ones_like(x, dtype=torch.bool))
    cst = torch.zeros(C_, SC_CST)
    if mode == "norm":
        off, fac, lo, hi = rnd(C_, seed=seed + 1) * 0.1, rnd(C_, seed=seed + 2).abs() + 0.5, -1.0, 1.5
        cst[:, 0], cst[:, 1], cst[:, 2], cst[:, 3] = off, fac, lo, hi
        f64 = lambda v: (v.double() - _bc(off.double())) / _bc(fac.double())      # noqa: E731
        x = _off_limits(x, f64, (lo, hi), 0.01 * _bc(fac))
        return dict(x=x, cst=cst, mode=SRC_NORM, actc=ACT_NONE, act=f64(x).clamp(lo, hi), live=None)
    sc, sh = rnd(C_, seed=seed + 1) * 0.3 + 1.0, rnd(C_, seed=seed + 2) * 0.5 + 1.0
    mean, invstd = rnd(C_, seed=seed + 3) * 0.2, rnd(C_, seed=seed + 4).abs() + 0.5
    cst[:, 0], cst[:, 1], cst[:, 2], cst[:, 3] = sc, sh, mean, invstd
    f64 = lambda v: v.double() * _bc(sc.double()) + _bc(sh.double())      # noqa: E731
    x = _off_limits(x, f64, (0.0, 6.0), 0.01 / _bc(sc))
    pre = f64(x)
    actc = ACT_RELU6 if mode == "affine6" else ACT_RELU
    act = pre.clamp(0, 6) if actc == ACT_RELU6 else pre.clamp_min(0)
    live = (pre > 0) & (pre < 6) if actc == ACT_RELU6 else pre > 0
    xhat = (x.double() - _bc(mean.double())) * _bc(invstd.double())
    return dict(x=x, cst=cst, mode=SRC_AFFINE, actc=actc, act=act, live=live, xhat=xhat, scale=sc.double())


def shift_cols(t):
    """the plane moved one column to the right (zeros enter): what a kernel with its taps off by one column would read"""
    return F.pad(t, (1, 0))[..., :-1]


def wgrad64(act, dy, cout, stride):
    return torch.nn.grad.conv2d_weight(act, (cout, act.shape[1], 3, 3), dy, stride=stride, padding=1)


def _sum_checks(name, n, vals, err, n_sq=None):
    """per-channel sums over (N, H, W) of kernel outputs `vals` (element-wise bound `err`): reference, bound for a chain of n, and the
    reference with the last row dropped"""
    dims = (0, 2, 3)
    out = {name: (vals.sum(dims), n * U * (vals.abs() + err).sum(dims) + err.sum(dims), vals[:, :, :-1].sum(dims))}
    if n_sq is not None:
        out[name + "sq"] = ((vals ** 2).sum(dims), n_sq * U * ((vals.abs() + err) ** 2).sum(dims) + (2 * vals.abs() * err + err ** 2).sum(dims),
                            (vals[:, :, :-1] ** 2).sum(dims))
    return out


# Each *_ref returns (inputs, checks); checks: name -> (float64 reference, element-wise bound, mutated reference).  The mutated
# reference is what a subtly wrong kernel would give: taps shifted by one column for convolutions and filter gradients, the last row
# dropped for sums.  The GPU tests compare against the first two; the host test asserts that the third violates the bound 10-fold.
@functools.lru_cache(maxsize=2)
def stem_fwd_ref(case):
    code, N, Cin, H, W, mode, flags = case
    xin, w = make_in(mode, N, Cin, H, W, seed=41), rnd(STEM_CO, Cin, 3, 3, seed=42, scale=0.3)
    conv = lambda a, k: F.conv2d(a, k, stride=2, padding=1)      # noqa: E731
    ref = conv(xin["act"], w.double())
    eb = (9 * Cin + 8) * U * conv(xin["act"].abs(), w.double().abs())
    checks = {"out": (ref, eb, conv(shift_cols(xin["act"]), w.double()))}
    if Cin <= 8:
        n = chain_stem_stats(code)
        checks.update(_sum_checks("sum", n, ref, eb, n_sq=n + 1))
    return (xin, w), checks


@functools.lru_cache(maxsize=2)
def stem_wgrad_ref(case):
    njb, N, Cin, H, W, modes, flags = case
    d, xin = make_dy(modes[0], N, STEM_CO, out_size(H), out_size(W), seed=7), make_in(modes[1], N, Cin, H, W, seed=41)
    n = chain_stem_wgrad(N, H, W)
    checks = {"dw": (wgrad64(xin["act"], d["dy"], STEM_CO, 2), n * U * wgrad64(xin["act"].abs(), d["dabs"], STEM_CO, 2),
                     wgrad64(shift_cols(xin["act"]), d["dy"], STEM_CO, 2))}
    return (d, xin), checks


def _head_filter(Cin):
    return rnd(1, Cin, 3, 3, seed=12, scale=0.3), torch.tensor([-0.21])


@functools.lru_cache(maxsize=2)
def head_fwd_ref(case):
    code, N, Cin, H, W, mode, flags = case
    xin, (w, b) = make_in(mode, N, Cin, H, W, seed=11), _head_filter(Cin)
    ref = F.conv2d(xin["act"], w.double(), b.double(), padding=1)
    eb = (9 * Cin + 8) * U * F.conv2d(xin["act"].abs(), w.double().abs(), padding=1) + U * float(b.abs())
    return (xin, w, b), {"out": (ref, eb, F.conv2d(shift_cols(xin["act"]), w.double(), b.double(), padding=1))}


def _head_dgrad_checks(dl, w):
    convT = lambda g, k: F.conv_transpose2d(g, k, padding=1)      # noqa: E731
    return (convT(dl.double(), w.double()), 16 * U * convT(dl.double().abs(), w.double().abs()), convT(shift_cols(dl.double()), w.double()))


@functools.lru_cache(maxsize=2)
def head_dgrad_ref(case):
    N, Cin, H, W, flags = case
    dl, (w, _) = rnd(N, 1, H, W, seed=5), _head_filter(Cin)
    return (dl, w), {"gin": _head_dgrad_checks(dl, w)}


def _head_wgrad_checks(xin, dl, n_dw, n_db):
    d = dl.double()
    return {"dw": (wgrad64(xin["act"], d, 1, 1), n_dw * U * wgrad64(xin["act"].abs(), d.abs(), 1, 1), wgrad64(shift_cols(xin["act"]), d, 1, 1)),
            "dbias": (d.sum().reshape(1), n_db * U * d.abs().sum().reshape(1), d[:, :, :-1].sum().reshape(1))}


@functools.lru_cache(maxsize=2)
def head_wgrad_ref(case):
    N, Cin, H, W, mode, flags = case
    xin, dl = make_in(mode, N, Cin, H, W, seed=11), rnd(N, 1, H, W, seed=5)
    return (xin, dl), _head_wgrad_checks(xin, dl, chain_head_wgrad(N, Cin, H, W), chain_head_dbias(N, H, W))


@functools.lru_cache(maxsize=2)
def head_bwd_ref(case):
    bns, N, H, W, mode, flags = case
    Cin = 16
    xin, dl, (w, _) = make_in(mode, N, Cin, H, W, seed=11), rnd(N, 1, H, W, seed=5), _head_filter(Cin)
    n = chain_head_bwd(N, H, W)
    checks = {"gin": _head_dgrad_checks(dl, w)}
    # dW: + 2 for the prologue's and the product's rounding, + 1 for the cast of the float64 row sum; dbias: the cast
    checks.update(_head_wgrad_checks(xin, dl, n + 3, n + 1))
    if bns:
        gin, eb, _ = checks["gin"]
        zero = torch.zeros((), dtype=torch.float64)
        gbn, gerr = torch.where(xin["live"], gin, zero), torch.where(xin["live"], eb, zero)      # the mask of the float64 pre-activation
        checks.update(_sum_checks("sum_g", n, gbn, gerr))
        # x_hat costs two roundings and its product one
        xh = xin["xhat"]
        dims = (0, 2, 3)
        checks["sum_gx"] = ((gbn * xh).sum(dims), (n + 3) * U * ((gbn.abs() + gerr) * xh.abs()).sum(dims) + (gerr * xh.abs()).sum(dims),
                            (gbn * xh)[:, :, :-1].sum(dims))
        amax = (gbn * _bc(xin["scale"])).abs().max().reshape(1)
        checks["absmax"] = (amax, 2 * U * amax, None)
    return (xin, dl, w), checks


# ---- the device side
def within(name, got, ref, bound):
    """element-wise |got - ref| <= bound with no NaN left; prints and returns the largest error-to-bound ratio"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
    err = (got - ref).abs()
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    print(f"SHRATIO {name} {ratio:.4f}")
    bad = err > bound
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements outside the bound, worst ratio {ratio:.3f}, first at {bad.nonzero()[0].tolist()}"
    return ratio


def _id(case):
    return "-".join(str(v) if not isinstance(v, tuple) else "+".join(v) for v in case).replace(" ", "+").rstrip("-")


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def run_stem_fwd(lib, case):
    code, N, Cin, H, W, mode, flags = case
    off = "offset" in _flags(flags)
    assert stem_fwd_code(Cin, W, not off) == code
    name = f"stem_fwd {_id(case)}"
    (xin, w), checks = stem_fwd_ref(case)
    Ho, Wo = out_size(H), out_size(W)
    out = dev_at(torch.empty(N, STEM_CO, Ho, Wo), off, fill=float("nan"))
    stats = _nan(lib.sc_stat_rows(STAT_STEM, N, Ho, Wo), STEM_CO, 2) if Cin <= 8 else None
    check(lib.sc_stem_conv_fwd(C.byref(src_of(xin, Cin, False)), ptr(dev(w)), ptr(out), N, Cin, H, W, ptr(stats), stream()))
    within(name + " out", out, *checks["out"][:2])
    if stats is not None:
        tot = stats.double().sum(0)
        within(name + " sum", tot[:, 0], *checks["sum"][:2])
        within(name + " sumsq", tot[:, 1], *checks["sumsq"][:2])
        # without statistics rows: the same outputs
        out2 = dev_at(torch.empty(N, STEM_CO, Ho, Wo), off, fill=float("nan"))
        check(lib.sc_stem_conv_fwd(C.byref(src_of(xin, Cin, False)), ptr(dev(w)), ptr(out2), N, Cin, H, W, None, stream()))
        torch.cuda.synchronize()
        assert torch.equal(out, out2)


def run_stem_wgrad(lib, case):
    njb, N, Cin, H, W, modes, flags = case
    assert stem_wgrad_njb(Cin) == njb
    rows = stem_wgrad_rows(N, H, W)
    if "loop" in _flags(flags):
        assert stem_wgrad_tiles(N, H, W) > rows
    (d, xin), checks = stem_wgrad_ref(case)
    n = lib.sc_stem_wgrad_workspace_floats(N, Cin, H, W)
    ws, dw = _nan(n), _nan(STEM_CO, Cin, 3, 3)
    check(lib.sc_stem_conv_wgrad(C.byref(src_of(d, STEM_CO, False, "g")), C.byref(src_of(xin, Cin, False)), ptr(ws), n, ptr(dw), N, Cin, H, W, stream()))
    within(f"stem_wgrad {_id(case)} rows={rows} dw", dw, *checks["dw"][:2])


def run_head_fwd(lib, case):
    code, N, Cin, H, W, mode, flags = case
    fl = _flags(flags)
    off_in, off_out = "offset_in" in fl, "offset_out" in fl
    assert head_fwd_code(Cin, W, not off_in, not off_out) == code
    (xin, w, b), checks = head_fwd_ref(case)
    out = dev_at(torch.empty(N, 1, H, W), off_out, fill=float("nan"))
    check(lib.sc_head_conv_fwd(C.byref(src_of(xin, Cin, off_in)), ptr(dev(w)), ptr(dev(b)), ptr(out), N, Cin, H, W, stream()))
    within(f"head_fwd {_id(case)} out", out, *checks["out"][:2])


def run_head_dgrad(lib, case):
    N, Cin, H, W, flags = case
    (dl, w), checks = head_dgrad_ref(case)
    gin = _nan(N, Cin, H, W)
    check(lib.sc_head_conv_dgrad(ptr(dev(dl)), ptr(dev(w)), ptr(gin), N, Cin, H, W, stream()))
    within(f"head_dgrad {_id(case)} gin", gin, *checks["gin"][:2])


def run_head_wgrad(lib, case):
    N, Cin, H, W, mode, flags = case
    if "loop" in _flags(flags):
        code = dw_code(OP_WGRAD, N, Cin, H, W, 1)
        assert chain_wgrad(code, N, Cin, H, W, 1) > chain_wgrad(code, 1, Cin, H, W, 1)      # a work-group walks more than one tile
    (xin, dl), checks = head_wgrad_ref(case)
    n = lib.sc_head_wgrad_workspace_floats(N, Cin, H, W)
    ws, dw, db = _nan(n), _nan(1, Cin, 3, 3), _nan(1)
    check(lib.sc_head_conv_wgrad(ptr(dev(dl)), C.byref(src_of(xin, Cin, False)), ptr(ws), n, ptr(dw), ptr(db), N, Cin, H, W, stream()))
    name = f"head_wgrad {_id(case)}"
    within(name + " dw", dw, *checks["dw"][:2])
    within(name + " dbias", db, *checks["dbias"][:2])


def run_head_bwd(lib, case):
    bns, N, H, W, mode, flags = case
    Cin = 16
    rows = head_bwd_rows(N, H, W)
    assert rows == min(head_bwd_tiles(N, H, W), 1024)
    if "loop" in _flags(flags):
        assert head_bwd_tiles(N, H, W) > rows
    (xin, dl, w), checks = head_bwd_ref(case)
    assert not bns or xin["mode"] == SRC_AFFINE
    dld, wd, src = dev(dl), dev(w), src_of(xin, Cin, False)
    n = lib.sc_head_wgrad_workspace_floats(N, Cin, H, W)
    ws, gin, dw, db = _nan(n), _nan(N, Cin, H, W), _nan(1, Cin, 3, 3), _nan(1)
    sums = _nan(rows, Cin, 2, dtype=torch.float64) if bns else None
    amax = torch.zeros(1, device=DEV) if bns else None
    check(lib.sc_head_conv_bwd(ptr(dld), C.byref(src), ptr(wd), ptr(gin), ptr(ws), n, ptr(dw), ptr(db), N, Cin, H, W, ptr(sums), ptr(amax), stream()))
    name = f"head_bwd {_id(case)} rows={rows}"
    within(name + " gin", gin, *checks["gin"][:2])
    within(name + " dw", dw, *checks["dw"][:2])
    within(name + " dbias", db, *checks["dbias"][:2])
    if bns:
        tot = sums.sum(0)
        within(name + " sum_g", tot[:, 0], *checks["sum_g"][:2])
        within(name + " sum_gx", tot[:, 1], *checks["sum_gx"][:2])
        within(name + " absmax", amax, *checks["absmax"][:2])
    # gin is what the separate data-gradient kernel writes, bit for bit
    gin2 = _nan(N, Cin, H, W)
    check(lib.sc_head_conv_dgrad(ptr(dld), ptr(wd), ptr(gin2), N, Cin, H, W, stream()))
    torch.cuda.synchronize()
    assert torch.equal(gin, gin2)


@pytest.mark.parametrize("case", STEM_FWD_CASES, ids=_id)
def test_stem_fwd_variant(hip, case):
    run_stem_fwd(hip, case)


@pytest.mark.parametrize("case", STEM_WGRAD_CASES, ids=_id)
def test_stem_wgrad_variant(hip, case):
    run_stem_wgrad(hip, case)


@pytest.mark.parametrize("case", HEAD_FWD_CASES, ids=_id)
def test_head_fwd_variant(hip, case):
    run_head_fwd(hip, case)


@pytest.mark.parametrize("case", HEAD_DGRAD_CASES, ids=_id)
def test_head_dgrad_variant(hip, case):
    run_head_dgrad(hip, case)


@pytest.mark.parametrize("case", HEAD_WGRAD_CASES, ids=_id)
def test_head_wgrad_variant(hip, case):
    run_head_wgrad(hip, case)


@pytest.mark.parametrize("case", HEAD_BWD_CASES, ids=_id)
def test_head_bwd_variant(hip, case):
    run_head_bwd(hip, case)
