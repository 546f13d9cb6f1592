"""Every kernel variant the depthwise 3x3 dispatchers can reach, against float64, element by element.

sc_dwconv3x3_fwd / _fwd_bn, _dgrad, _wgrad and _bwd_fused pick a template instantiation from the shape: stride {1, 2} x tile width
{64, 32, 16} (x float4 | element-wise staging for the forward and the fused backward) and the wave-per-plane kernels.  The host query
sc_dw_variant names the instantiation, and the launchers dispatch on the same function.  Here every code it can return has a plain case
and a ragged one; every case asserts the code it was written for before it launches.  tests/test_depthwise_variants_host.py holds the
tables below to the full set of codes on a box without a GPU, which is why the tables, `dw_code` and the chain counts sit at module
level and touch no device.

References: the same op sequence in float64 on the CPU from the same fp32 inputs -- F.conv2d(act(x sc + sh), w) and its autograd, dy
formed as sc_pro_bnbwd / sc_pro_affine form it.  Bounds are derived, not measured, and hold element by element (u = 2^-24):
  forward         |out - ref| <= 16 u conv(|act|, |w|)         nine FMA roundings, one of the prologue, the rest is slack
  data gradient   |dx - ref|  <= 16 u convT(dabs, |w|) (+ u |prev| with accum);  dabs = |g A| mask + |y B| + |D| (BNBWD),
                  |g a| + |b| (AFFINE), |g| (RAW): the sum of the magnitudes the prologue adds up
  filter gradient |dw - ref|  <= n u sum |dy| |act| per (channel, tap), n = the longest fp32 chain of the case (chain_wgrad)
  statistics      sum and sum of squares per channel over all rows: n u sum |.| for the chain (chain_tile), plus what the element-wise
                  bound of the summed values allows
  in_sums         sum g_bn and sum g_bn x_hat in the same way
With accum the last rounding is that of prev + acc, which is all of u |prev| where the gradient is small next to prev: those cases come
close to their bound by construction.
The masks of ReLU / ReLU6 are discontinuous, so the inputs they are taken from are moved off the thresholds (by 0.01 where a value
lies within 1e-3 of 0 or 6): no element is excluded from any comparison.  Every case prints its error-to-bound ratios before it asserts."""
import ctypes as C
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import hip_ops  # noqa: E402
from hip_ops import DEV, dev  # noqa: E402
from starcop_amd import _lib  # noqa: E402
from starcop_amd._lib import (ACT_NONE, ACT_RELU, ACT_RELU6, SC_CST, SRC_AFFINE, SRC_BNBWD, SRC_RAW, STAT_DW, check, make_src, ptr,
                              sc_bn_tail, stream)  # noqa: E402
from test_gpu_ops import rnd  # noqa: E402

U = 2.0 ** -24
OP_FWD, OP_DGRAD, OP_WGRAD, OP_BWD = 0, 1, 2, 3

# ---- case tables: (code, N, C, H, W, stride, source modes, flags).  code = 1000 stride + 10 TW + V4, or 9016 for the plane kernels (16 x 16 planes).
# H, W: the INPUT plane of the layer.  The work-groups tile the output plane in the forward and the filter gradient and the input
# plane in the data gradient and the fused backward; TW = 64 above 32 columns of that plane (64 x 32 tiles), 32 above 16 (32 x 32), else
# 16 (16 x 16).  Input modes: raw (no activation) | affine6 (BatchNorm constants + ReLU6) | affine_relu; dy modes: raw | affine |
# bnbwd6 (BatchNorm backward behind a ReLU6 mask).  Flags: ragged (see the host test for what that must hold), offset (every tensor
# starts 4 bytes past a 16-byte boundary: the float4 forms must not be chosen; the shape is that of an aligned case of the table),
# plane_fallback, accum, nosums (in_sums = NULL), loop.
DW_FWD_CASES = [
    (1641, 1, 8, 32, 64, 1, "affine6", ""),
    (1641, 1, 5, 37, 68, 1, "affine_relu", "ragged"),       # 2 x 2 tiles, the last tile column holds 4 columns
    (1640, 1, 8, 16, 66, 1, "raw", ""),
    (1640, 3, 3, 37, 70, 1, "affine6", "ragged"),
    (1640, 1, 6, 5, 33, 1, "affine6", "ragged"),            # the narrowest plane on the 64-wide tile
    (1640, 1, 8, 32, 64, 1, "affine6", "offset"),
    (1321, 2, 4, 32, 32, 1, "affine6", ""),
    (1321, 1, 7, 37, 20, 1, "raw", "ragged"),
    (1320, 1, 8, 20, 18, 1, "affine_relu", ""),
    (1320, 3, 3, 37, 27, 1, "affine6", "ragged"),
    (1320, 2, 4, 32, 32, 1, "affine6", "offset"),
    (1161, 1, 8, 8, 16, 1, "affine6", ""),
    (1161, 1, 7, 20, 12, 1, "affine6", "ragged"),
    (1161, 1, 6, 16, 16, 1, "affine6", "plane_fallback"),
    (1160, 1, 8, 7, 9, 1, "raw", ""),
    (1160, 3, 5, 20, 13, 1, "affine6", "ragged"),
    (1160, 2, 4, 16, 16, 1, "affine6", "offset"),           # unaligned: neither the plane kernel nor float4 staging
    (2641, 1, 8, 16, 68, 2, "affine6", ""),
    (2641, 3, 5, 37, 72, 2, "affine6", "ragged"),
    (2640, 1, 8, 20, 66, 2, "affine_relu", ""),
    (2640, 1, 7, 37, 71, 2, "affine6", "ragged"),
    (2640, 1, 8, 16, 68, 2, "affine6", "offset"),
    (2321, 2, 4, 32, 64, 2, "raw", ""),
    (2321, 1, 5, 39, 36, 2, "affine6", "ragged"),
    (2320, 1, 8, 16, 34, 2, "affine6", ""),
    (2320, 3, 3, 39, 37, 2, "affine6", "ragged"),
    (2320, 2, 4, 32, 64, 2, "affine6", "offset"),
    (2161, 2, 4, 32, 32, 2, "affine6", ""),
    (2161, 1, 7, 40, 12, 2, "affine_relu", "ragged"),
    (2160, 1, 8, 8, 6, 2, "affine6", ""),
    (2160, 3, 5, 9, 13, 2, "raw", "ragged"),
    (2160, 2, 4, 32, 32, 2, "affine6", "offset"),
    (9016, 2, 4, 16, 16, 1, "affine6", ""),
    (9016, 1, 12, 16, 16, 1, "raw", "ragged"),
]

# dy mode only
DW_DGRAD_CASES = [
    (1640, 1, 8, 32, 64, 1, "raw", ""),
    (1640, 3, 3, 37, 70, 1, "bnbwd6", "ragged"),
    (1640, 1, 6, 5, 33, 1, "affine", "ragged accum"),
    (1320, 2, 4, 32, 32, 1, "bnbwd6", ""),
    (1320, 1, 7, 37, 27, 1, "affine", "ragged accum"),
    (1160, 1, 8, 16, 16, 1, "raw", ""),
    (1160, 3, 5, 20, 13, 1, "bnbwd6", "ragged"),
    (2640, 1, 8, 32, 64, 2, "bnbwd6", ""),
    (2640, 3, 3, 39, 37, 2, "affine", "ragged"),
    (2640, 1, 7, 37, 71, 2, "bnbwd6", "ragged accum"),
    (2320, 2, 4, 32, 32, 2, "raw", ""),
    (2320, 1, 7, 37, 27, 2, "bnbwd6", "ragged"),
    (2160, 1, 8, 16, 16, 2, "affine", ""),
    (2160, 3, 5, 9, 13, 2, "bnbwd6", "ragged accum"),
]

# (dy mode, input mode)
DW_WGRAD_CASES = [
    (1640, 1, 8, 32, 64, 1, ("raw", "affine6"), ""),
    (1640, 3, 3, 37, 70, 1, ("bnbwd6", "affine_relu"), "ragged"),
    (1640, 1, 6, 5, 33, 1, ("affine", "raw"), "ragged"),
    (1320, 2, 4, 32, 32, 1, ("bnbwd6", "affine6"), ""),
    (1320, 1, 7, 37, 27, 1, ("affine", "raw"), "ragged"),
    (1160, 1, 8, 16, 16, 1, ("raw", "affine6"), ""),
    (1160, 3, 5, 20, 13, 1, ("bnbwd6", "affine6"), "ragged"),
    (1160, 8, 960, 8, 8, 1, ("bnbwd6", "affine6"), "loop"),       # 8 tiles on a grid of 4 work-groups per channel
    (2640, 1, 8, 16, 68, 2, ("raw", "affine6"), ""),
    (2640, 3, 3, 37, 71, 2, ("bnbwd6", "affine6"), "ragged"),
    (2320, 2, 4, 32, 64, 2, ("affine", "affine6"), ""),
    (2320, 3, 3, 39, 37, 2, ("bnbwd6", "raw"), "ragged"),
    (2160, 1, 8, 16, 32, 2, ("raw", "affine6"), ""),
    (2160, 3, 5, 9, 13, 2, ("affine", "affine_relu"), "ragged"),
    (2160, 8, 960, 16, 16, 2, ("bnbwd6", "affine6"), "loop"),
]

# (dy mode, input mode); in_sums need an AFFINE input
DW_BWD_CASES = [
    (1641, 1, 8, 32, 64, 1, ("bnbwd6", "affine6"), ""),
    (1641, 1, 5, 37, 68, 1, ("bnbwd6", "affine_relu"), "ragged"),
    (1640, 1, 8, 16, 66, 1, ("raw", "affine6"), ""),
    (1640, 3, 3, 37, 70, 1, ("bnbwd6", "affine6"), "ragged"),
    (1640, 1, 6, 5, 33, 1, ("affine", "raw"), "ragged nosums"),
    (1640, 1, 8, 32, 64, 1, ("bnbwd6", "affine6"), "offset"),
    (1321, 2, 4, 32, 32, 1, ("bnbwd6", "affine6"), ""),
    (1321, 1, 7, 37, 20, 1, ("affine", "affine6"), "ragged"),
    (1320, 1, 8, 20, 18, 1, ("bnbwd6", "affine6"), ""),
    (1320, 1, 4, 20, 18, 1, ("bnbwd6", "affine6"), "nosums"),
    (1320, 3, 3, 37, 27, 1, ("bnbwd6", "affine6"), "ragged"),
    (1320, 2, 4, 32, 32, 1, ("bnbwd6", "affine6"), "offset"),
    (1161, 1, 8, 8, 16, 1, ("bnbwd6", "affine6"), ""),
    (1161, 1, 7, 20, 12, 1, ("raw", "affine_relu"), "ragged"),
    (1161, 1, 6, 16, 16, 1, ("bnbwd6", "affine6"), "plane_fallback"),
    (1160, 1, 8, 7, 9, 1, ("bnbwd6", "affine6"), ""),
    (1160, 1, 4, 7, 9, 1, ("bnbwd6", "raw"), "nosums"),
    (1160, 3, 5, 20, 13, 1, ("bnbwd6", "affine6"), "ragged"),
    (1160, 2, 4, 16, 16, 1, ("bnbwd6", "affine6"), "offset"),
    (2641, 1, 8, 32, 64, 2, ("bnbwd6", "affine6"), ""),
    (2641, 1, 5, 40, 72, 2, ("bnbwd6", "affine6"), "ragged"),     # 2 x 2 tiles, the last tile column holds 8 columns
    (2640, 1, 8, 16, 36, 2, ("affine", "affine6"), ""),           # 18 output columns: no float4 rows of dy
    (2640, 3, 3, 38, 70, 2, ("bnbwd6", "affine6"), "ragged"),
    (2640, 1, 8, 32, 64, 2, ("bnbwd6", "affine6"), "offset"),
    (2321, 2, 4, 32, 32, 2, ("bnbwd6", "affine6"), ""),
    (2321, 1, 7, 38, 24, 2, ("bnbwd6", "affine_relu"), "ragged"),
    (2320, 1, 8, 16, 20, 2, ("raw", "affine6"), ""),
    (2320, 3, 3, 38, 26, 2, ("bnbwd6", "affine6"), "ragged"),
    (2320, 2, 4, 32, 32, 2, ("bnbwd6", "affine6"), "offset"),
    (2161, 2, 4, 16, 16, 2, ("bnbwd6", "affine6"), ""),
    (2161, 1, 7, 20, 8, 2, ("bnbwd6", "affine6"), "ragged nosums"),
    (2160, 1, 8, 8, 12, 2, ("bnbwd6", "affine6"), ""),
    (2160, 3, 5, 18, 14, 2, ("affine", "raw"), "ragged nosums"),
    (2160, 2, 4, 16, 16, 2, ("bnbwd6", "affine6"), "offset"),
    (9016, 2, 4, 16, 16, 1, ("bnbwd6", "affine6"), ""),
    (9016, 1, 12, 16, 16, 1, ("raw", "affine_relu"), "ragged"),
    (9016, 1, 4, 16, 16, 1, ("bnbwd6", "raw"), "nosums"),
]

DW_CASES = {OP_FWD: DW_FWD_CASES, OP_DGRAD: DW_DGRAD_CASES, OP_WGRAD: DW_WGRAD_CASES, OP_BWD: DW_BWD_CASES}


# ---- host side (no device)
def dw_code(op, N, C_, H, W, stride, aligned16=True):
    return _lib.load().sc_dw_variant(op, N, C_, H, W, stride, int(aligned16))


def dw_tile(code):
    """(tile width, tile height, R = pixels of a thread) of a tile-kernel code"""
    tw = code % 1000 // 10
    return {64: (64, 32, 8), 32: (32, 32, 4), 16: (16, 16, 1)}[tw]


def dw_tiled_plane(op, H, W, stride):
    """the plane the work-groups of `op` tile"""
    if op in (OP_FWD, OP_WGRAD):
        return (H - 1) // stride + 1, (W - 1) // stride + 1
    return H, W


def dw_tiles(op, code, H, W, stride):
    tw, th, _ = dw_tile(code)
    ph, pw = dw_tiled_plane(op, H, W, stride)
    return -(-ph // th) * -(-pw // tw)


def wgrad_tiles_per_group(code, N, C_, H, W, stride):
    """k_dw_wgrad: a grid of min(N tiles, 4096 / C) work-groups per channel strides over the N tiles"""
    T = N * dw_tiles(OP_WGRAD, code, H, W, stride)
    return -(-T // min(T, max(4096 // C_, 1)))


# Chain counts: the number of fp32 roundings on the longest path from a term to the value the kernel stores, + 3 for the roundings of
# the terms themselves (prologue, product).  The rows / atomics are summed in fp64.
def chain_wgrad(code, N, C_, H, W, stride):
    """k_dw_wgrad: a thread adds R products per tile it visits to a register, then 6 butterfly steps of the wave sum and 3 additions
    across the four waves"""
    return dw_tile(code)[2] * wgrad_tiles_per_group(code, N, C_, H, W, stride) + 9 + 3


def chain_tile(code, stride=1):
    """per-tile sums of k_dw_fwd (statistics) and k_dw_bwd (filter gradient, in_sums): a thread adds its R pixels (stride-2 backward: the
    4 pixels of each of its max(R / 4, 1) 2 x 2 blocks, so at most max(R, 4) terms), then the 6 + 3 steps of the block sum.  Plane
    kernels: a lane adds its 4 pixels (one float4 of a 16 x 16 plane), then the 6 steps of the wave sum."""
    if code == 9016:
        return 4 + 6 + 3
    R = dw_tile(code)[2]
    return (R if stride == 1 else max(R, 4)) + 9 + 3


# ---- inputs and float64 references
def _bc(v):
    return v[None, :, None, None]


def _off_threshold(t, scale, shift):
    """move the elements of t whose float64 scale * t + shift lies within 1e-3 of 0 or 6 by 0.01 / scale; none may remain"""
    def near(v):
        p = v.double() * _bc(scale.double()) + _bc(shift.double())
        return (p.abs() < 1e-3) | ((p - 6).abs() < 1e-3)
    t = torch.where(near(t), t + 0.01 / _bc(scale), t)
    assert not bool(near(t).any())
    return t


def make_input(mode, N, C_, H, W, seed, off_threshold=False):
    """-> dict(x fp32, cst [C][SC_CST] or None, src mode, act code, act = float64 activated input, pre = float64 pre-activation,
    live = where the activation passes a gradient, xhat = float64 (x - mean) invstd of an AFFINE input)"""
    x = rnd(N, C_, H, W, seed=seed, scale=2.0)
    if mode == "raw":
        return dict(x=x, cst=None, mode=SRC_RAW, actc=ACT_NONE, act=x.double(), pre=x.double(), live=torch.ones_like(x, dtype=torch.bool))
    sc, sh = rnd(C_, seed=seed + 1) * 0.3 + 1.0, rnd(C_, seed=seed + 2) * 0.5 + 1.0
    mean, invstd = rnd(C_, seed=seed + 3) * 0.2, rnd(C_, seed=seed + 4).abs() + 0.5
    if off_threshold:
        x = _off_threshold(x, sc, sh)
    cst = torch.zeros(C_, SC_CST)
    cst[:, 0], cst[:, 1], cst[:, 2], cst[:, 3] = sc, sh, mean, invstd
    pre = x.double() * _bc(sc.double()) + _bc(sh.double())
    actc = ACT_RELU6 if mode == "affine6" else ACT_RELU
    act = pre.clamp(0, 6) if actc == ACT_RELU6 else pre.clamp_min(0)
    live = (pre > 0) & (pre < 6) if actc == ACT_RELU6 else pre > 0
    xhat = (x.double() - _bc(mean.double())) * _bc(invstd.double())
    return dict(x=x, cst=cst, mode=SRC_AFFINE, actc=actc, act=act, pre=pre, live=live, xhat=xhat)


def make_dy(mode, N, C_, Ho, Wo, seed):
    """-> dict(g fp32, y fp32 or None, cst, src mode, act code, dy = float64 gradient as the prologue forms it, dabs = the sum of the
    magnitudes the prologue adds up)"""
    g = rnd(N, C_, Ho, Wo, seed=seed)
    if mode == "raw":
        return dict(g=g, y=None, cst=None, mode=SRC_RAW, actc=ACT_NONE, dy=g.double(), dabs=g.double().abs())
    a, b = rnd(C_, seed=seed + 1) * 0.2 + 1.0, rnd(C_, seed=seed + 2) * 0.2
    cst = torch.zeros(C_, SC_CST)
    cst[:, 0], cst[:, 1] = a, b
    if mode == "affine":
        ga = g.double() * _bc(a.double())
        return dict(g=g, y=None, cst=cst, mode=SRC_AFFINE, actc=ACT_NONE, dy=ga + _bc(b.double()), dabs=ga.abs() + _bc(b.double().abs()))
    assert mode == "bnbwd6"
    A, B, D = rnd(C_, seed=seed + 3), rnd(C_, seed=seed + 4) * 0.1, rnd(C_, seed=seed + 5) * 0.1
    cst[:, 2], cst[:, 3], cst[:, 4] = A, B, D
    y = _off_threshold(rnd(N, C_, Ho, Wo, seed=seed + 6, scale=3.0) + 2.0, a, b)
    yh = y.double() * _bc(a.double()) + _bc(b.double())
    gm = torch.where((yh > 0) & (yh < 6), g.double(), torch.zeros((), dtype=torch.float64)) * _bc(A.double())
    yb = y.double() * _bc(B.double())
    return dict(g=g, y=y, cst=cst, mode=SRC_BNBWD, actc=ACT_RELU6, dy=gm + yb + _bc(D.double()),
                dabs=gm.abs() + yb.abs() + _bc(D.double().abs()))


def make_filter(C_, seed=2):
    return rnd(C_, 1, 3, 3, seed=seed, scale=0.4)


def conv64(act, w, stride):
    return F.conv2d(act, w, stride=stride, padding=1, groups=act.shape[1])


def conv_bwd64(act, w, dy, stride):
    """(gradient w.r.t. the activated input, gradient w.r.t. the filter) of conv64 under dy, by float64 autograd"""
    a_, w_ = act.clone().requires_grad_(True), w.clone().requires_grad_(True)
    conv64(a_, w_, stride).backward(dy)
    return a_.grad, w_.grad


def dev_at(t, offset, fill=None):
    """device copy of host tensor t; offset: it starts one float past a 16-byte boundary (a view into a larger buffer)"""
    if not offset:
        d = dev(t)
    else:
        buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
        d = buf[1:1 + t.numel()].view(t.shape)
        d.copy_(t)
        hip_ops._KEEP.append(d)      # alive until the end of the test, like what dev() returns
        assert d.data_ptr() % 16 == 4 and d.is_contiguous()
    if fill is not None:
        d.fill_(fill)
    return d


def src_of(d, C_, offset, x_key="x"):
    """sc_src of make_input / make_dy on the device"""
    aux = dev_at(d["y"], offset) if d.get("y") is not None else None
    return make_src(dev_at(d[x_key], offset), C_, d["mode"], act=d["actc"], cst=dev(d["cst"]) if d["cst"] is not None else None, aux=aux)


def within(name, got, ref, bound):
    """element-wise |got - ref| <= bound with no NaN left; prints and returns the largest error-to-bound ratio"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
    err = (got - ref).abs()
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    print(f"DWRATIO {name} {ratio:.4f}")
    bad = err > bound
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements outside the bound, worst ratio {ratio:.3f}, first at {bad.nonzero()[0].tolist()}"
    return ratio


def _flags(flags):
    return set(flags.split())


def _id(case):
    return "-".join(str(v) if not isinstance(v, tuple) else "+".join(v) for v in case).replace(" ", "+").rstrip("-")


# ---- the ops
def run_fwd(lib, code, N, C_, H, W, stride, mode, flags):
    fl = _flags(flags)
    off = "offset" in fl
    assert dw_code(OP_FWD, N, C_, H, W, stride, not off) == code
    name = f"fwd {code} {N}x{C_}x{H}x{W}/{stride} {mode} {flags}".rstrip()
    xin, w = make_input(mode, N, C_, H, W, seed=1), make_filter(C_)
    ref = conv64(xin["act"], w.double(), stride)
    cabs = conv64(xin["act"].abs(), w.double().abs(), stride)
    Ho, Wo = ref.shape[-2:]
    src, wd = src_of(xin, C_, off), dev(w)
    rows = lib.sc_stat_rows(STAT_DW, N, Ho, Wo)
    out = dev_at(torch.empty(N, C_, Ho, Wo), off, fill=float("nan"))
    stats = torch.full((rows, C_, 2), float("nan"), device=DEV)
    check(lib.sc_dwconv3x3_fwd(C.byref(src), ptr(wd), ptr(out), N, C_, H, W, stride, ptr(stats), stream()))
    ebound = 16 * U * cabs
    within(name + " out", out, ref, ebound)
    # statistics rows: the fp32 chain over the launch's outputs + what the outputs themselves may be off
    n = chain_tile(code)
    dims = (0, 2, 3)
    within(name + " sum", stats.double().sum(0)[:, 0], ref.sum(dims), n * U * (ref.abs() + ebound).sum(dims) + ebound.sum(dims))
    within(name + " sumsq", stats.double().sum(0)[:, 1], (ref ** 2).sum(dims),
           n * U * ((ref.abs() + ebound) ** 2).sum(dims) + (2 * ref.abs() * ebound + ebound ** 2).sum(dims))
    # the launch that also finalizes the BatchNorm is the same kernel: identical outputs and rows
    out2 = dev_at(torch.empty(N, C_, Ho, Wo), off, fill=float("nan"))
    stats2 = torch.full((rows, C_, 2), float("nan"), device=DEV)
    bt = sc_bn_tail()
    keep = [dev(rnd(C_, seed=5) * 0.2 + 1), dev(rnd(C_, seed=6) * 0.1), torch.zeros(C_, device=DEV), torch.ones(C_, device=DEV),
            torch.full((C_, SC_CST), float("nan"), device=DEV), torch.zeros(1, device=DEV), torch.zeros(C_, dtype=torch.int32, device=DEV)]
    bt.gamma, bt.beta, bt.running_mean, bt.running_var, bt.cst, bt.act_bound, bt.tickets = (t.data_ptr() for t in keep)
    bt.momentum, bt.eps = 0.1, 1e-5
    check(lib.sc_dwconv3x3_fwd_bn(C.byref(src), ptr(wd), ptr(out2), N, C_, H, W, stride, ptr(stats2), C.byref(bt), stream()))
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(stats, stats2)
    assert bool(torch.isfinite(keep[4][:, :4]).all()) and bool((keep[6] == rows).all())


def run_dgrad(lib, code, N, C_, H, W, stride, mode, flags):
    fl = _flags(flags)
    assert dw_code(OP_DGRAD, N, C_, H, W, stride) == code
    name = f"dgrad {code} {N}x{C_}x{H}x{W}/{stride} {mode} {flags}".rstrip()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    d, w = make_dy(mode, N, C_, Ho, Wo, seed=7), make_filter(C_)
    zero = torch.zeros(N, C_, H, W, dtype=torch.float64)
    ref, _ = conv_bwd64(zero, w.double(), d["dy"], stride)
    bound = 16 * U * conv_bwd64(zero, w.double().abs(), d["dabs"], stride)[0]
    accum = "accum" in fl
    prev = rnd(N, C_, H, W, seed=20) if accum else torch.full((N, C_, H, W), float("nan"))
    if accum:
        ref, bound = ref + prev.double(), bound + U * prev.double().abs()
    dx = dev(prev).clone()
    check(lib.sc_dwconv3x3_dgrad(C.byref(src_of(d, C_, False, "g")), ptr(dev(w)), ptr(dx), int(accum), N, C_, H, W, stride, stream()))
    within(name + " dx", dx, ref, bound)


def run_wgrad(lib, code, N, C_, H, W, stride, modes, flags):
    fl = _flags(flags)
    assert dw_code(OP_WGRAD, N, C_, H, W, stride) == code
    if "loop" in fl:
        assert wgrad_tiles_per_group(code, N, C_, H, W, stride) >= 2
    name = f"wgrad {code} {N}x{C_}x{H}x{W}/{stride} {'+'.join(modes)} {flags}".rstrip()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    d, xin = make_dy(modes[0], N, C_, Ho, Wo, seed=7), make_input(modes[1], N, C_, H, W, seed=1)
    w0 = torch.zeros(C_, 1, 3, 3, dtype=torch.float64)
    _, ref = conv_bwd64(xin["act"], w0, d["dy"], stride)
    _, sabs = conv_bwd64(xin["act"].abs(), w0, d["dy"].abs(), stride)
    acc = torch.zeros(C_ * 9, dtype=torch.float64, device=DEV)
    check(lib.sc_dwconv3x3_wgrad(C.byref(src_of(d, C_, False, "g")), C.byref(src_of(xin, C_, False)), ptr(acc), N, C_, H, W, stride, stream()))
    within(name + " dw", acc, ref, chain_wgrad(code, N, C_, H, W, stride) * U * sabs)


def run_bwd(lib, code, N, C_, H, W, stride, modes, flags):
    fl = _flags(flags)
    off = "offset" in fl
    assert dw_code(OP_BWD, N, C_, H, W, stride, not off) == code
    name = f"bwd {code} {N}x{C_}x{H}x{W}/{stride} {'+'.join(modes)} {flags}".rstrip()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    want_sums = "nosums" not in fl
    d, xin, w = make_dy(modes[0], N, C_, Ho, Wo, seed=7), make_input(modes[1], N, C_, H, W, seed=1, off_threshold=True), make_filter(C_)
    assert not want_sums or xin["mode"] == SRC_AFFINE
    dx_ref, dw_ref = conv_bwd64(xin["act"], w.double(), d["dy"], stride)
    ebound = 16 * U * conv_bwd64(xin["act"], w.double().abs(), d["dabs"], stride)[0]
    _, sabs = conv_bwd64(xin["act"].abs(), w.double(), d["dy"].abs(), stride)
    dsrc, xsrc, wd = src_of(d, C_, off, "g"), src_of(xin, C_, off), dev(w)
    dx = dev_at(torch.empty(N, C_, H, W), off, fill=float("nan"))
    acc = torch.zeros(C_ * 9, dtype=torch.float64, device=DEV)
    rows = lib.sc_stat_rows(STAT_DW, N, H, W)
    sums = torch.full((rows, C_, 2), float("nan"), dtype=torch.float64, device=DEV) if want_sums else None
    check(lib.sc_dwconv3x3_bwd_fused(C.byref(dsrc), C.byref(xsrc), ptr(wd), ptr(dx), ptr(acc), ptr(sums), N, C_, H, W, stride, stream()))
    n = chain_tile(code, stride)
    within(name + " dx", dx, dx_ref, ebound)
    within(name + " dw", acc, dw_ref, n * U * sabs)
    if want_sums:
        # g_bn = dx behind the mask of the input's own activation; x_hat costs two more roundings and its product one
        dims = (0, 2, 3)
        zero = torch.zeros((), dtype=torch.float64)
        gbn, gerr = torch.where(xin["live"], dx_ref, zero), torch.where(xin["live"], ebound, zero)
        tot = sums.sum(0)
        within(name + " sum_g", tot[:, 0], gbn.sum(dims), n * U * (gbn.abs() + gerr).sum(dims) + gerr.sum(dims))
        xh = xin["xhat"].abs()
        within(name + " sum_gx", tot[:, 1], (gbn * xin["xhat"]).sum(dims), (n + 3) * U * ((gbn.abs() + gerr) * xh).sum(dims) + (gerr * xh).sum(dims))
    # dx is what the separate data-gradient kernel writes, bit for bit
    dx2 = dev_at(torch.empty(N, C_, H, W), off, fill=float("nan"))
    check(lib.sc_dwconv3x3_dgrad(C.byref(dsrc), ptr(wd), ptr(dx2), 0, N, C_, H, W, stride, stream()))
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2)


@pytest.mark.parametrize("case", DW_FWD_CASES, ids=_id)
def test_dw_fwd_variant(hip, case):
    run_fwd(hip, *case)


@pytest.mark.parametrize("case", DW_DGRAD_CASES, ids=_id)
def test_dw_dgrad_variant(hip, case):
    run_dgrad(hip, *case)


@pytest.mark.parametrize("case", DW_WGRAD_CASES, ids=_id)
def test_dw_wgrad_variant(hip, case):
    run_wgrad(hip, *case)


@pytest.mark.parametrize("case", DW_BWD_CASES, ids=_id)
def test_dw_bwd_fused_variant(hip, case):
    run_bwd(hip, *case)
