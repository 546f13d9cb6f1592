"""Every launch geometry and ABI mode of the fused training block (csrc/conv_irt.hip) against float64.

conv_irt.hip has no kernel variants, but its launch geometry decides which code runs: five loops (the grid-stride loops of k_irt_stats
and k_irt_fix, the persistent tile loop of k_irt_fwd, the tile walk of k_irt_bwd, the K loop of k_irt_xmom) take one trip or several, a
chunk group holds 1 to 3 chunks of 32 hidden channels, the last chunk is full or partial, the last k_irt_bwd work-group is full or short.
The host query sc_irt_geometry reports all of it (the launchers read the same function), and a geometry CLASS is the tuple
    (NKS, nch, hidden % 32 == 0, loops that iterate as a subset of "sfbmx" = stats / fwd / bwd / moments / fix, last bwd work-group short)
tests/test_irt_variants_host.py holds the table below to the classes a sweep of the query reaches under the size caps of an ordinary
case (N <= 3, 4096 pixels per image); every case asserts its class before it launches.  Ordinary cases: the 24 classes of small planes
(no loop iterates) and the 24 of narrow planes 344 | 348 x 8, where two chunk groups leave 256 k_irt_bwd work-groups for 258 | 261 tiles
(tiles_per_wg = 2, last work-group full | short).  Two large cases make the other four loops iterate:
    (2, 24, 168, 164, 208)   68,224 pixels: stats and moments grids capped; 294 forward tiles on 256 work-groups (per_cu = 1 at nch 6,
                             NKS 2); 574 backward tiles, two chunk groups (3 + 3 chunks, the last partial), tiles_per_wg 3, last short
    (3, 8, 8, 152, 296)      134,976 pixels: the fix grid capped at 1,024; 1,140 backward tiles, one chunk group of one 8-channel chunk
(the first is (2, 24, 168, 164, 232) three tile columns narrower: the query confirms every loop still iterates, and the plane stays off
all three tilings; 160 rows would do too, but 80 output rows are whole tiles.)  A flat 32-pixel block
ragged against the batch (N H W % 32 != 0) cannot occur: sc_irt_supported asks H % 4 == 0 and W % 8 == 0 (the host test asserts this).

Inputs.  The backward pass is discontinuous at the ReLU6 switches, so the seed advances until no BatchNorm output of the float64
reference lies within 2e-5 of 0 or 6.  Small cases use Gaussian inputs; at 1e7 elements no seed reaches that margin, so the large cases
draw every pixel from a palette of P = 64 (P = 256 for Cin 8) random Cin-vectors by an independent random index: a channel's BatchNorm
output takes at most P values, every pixel still differs from its neighbours.  No element is excluded from any comparison.
AFFINE inputs with ACT_RELU / ACT_RELU6 spread over about +-6; the prologue value is formed as the kernels form it (one fma, rounded to
fp32 once) and the ACTIVATED input is the leaf of the reference's dx.  BNBWD gradient sources have their BatchNorm outputs moved off the
mask thresholds.

Forward, element by element.  cst_expand is teacher-forced from the float64 batch statistics rounded to fp32; the reference forms
y = scale e + shift from those fp32 constants in float64.  With u = 2^-24, D3 = 4 u + 2^-31 (sc_split.h: each operand's three-term split
is exact to 2^-24, the dropped products a1 b2 and a2 b1 weigh 2^-8 2^-16 each, a2 b2 2^-32) and n = 6 * 16 * NKS + 2:
    |de| <= (D3 + n u) sum_c |W_e||x_a|        |dy| <= |scale| |de| + u |y|        |dd| <= sum_taps |w_d| |dy| + 10 u sum_taps |w_d||e_hat|
every element of d must lie within |dd| (a zero bound asks for an exact zero); the aggregate gate 1e-5 stays.  sc_irt_fwd with
stats_d = NULL must write the same bits.  Statistics rows of e and of d, summed in float64, against float64 sums of the reference e and
of the launch's own d: 2e-5 of the largest channel.

Backward.  The aggregate gates of tests/test_gpu_irt.py, unchanged (2e-5 of the tensor's maximum), and a per-channel error: the largest
difference in a channel over that channel's own maximum -- per hidden channel for dW_dw, dgamma, dbeta and the rows of dW_e, per image and
input channel for dx.  A channel whose reference maximum is below 1e-3 of the tensor's maximum is compared against the tensor's maximum
(printed per case as "low": 4 of the table's 26,856 channels, 0.015 %; at most 2 of 584 in a case, and each case asserts < 5 %).  The
gate is per tensor, 4 x the worst value measured over the table on the MI355X and never above 2e-5 (PER_CHANNEL_GATE).  For dgamma and
dbeta a channel is ONE number, so this is an element-wise relative error; the gradient of the depthwise output is therefore d itself
(the loss |d|^2 / 2) and the depthwise taps have a positive mean, see make_gradient.  All four (add0, accum) modes of sc_irt_bwd_fix.

Guard bands.  d_out, both statistics buffers, esums, dw_acc, dx, dW_e and the workspace (exactly sc_irt_bwd_workspace_floats floats) are
views inside NaN-filled allocations with 256 elements either side, 16-byte aligned; the bands must be all NaN after the launches.

Measured on the MI355X (profiles/irt_variants.txt has both lines of every case).  Worst over the 50 cases: forward error / bound 0.084,
aggregate d 1.7e-7, statistics rows 1.2e-7; backward aggregate dW_dw 1.0e-7, dgamma 2.1e-7, dbeta 6.8e-8, dx 5.6e-7 (4.7e-7 to 5.0e-7
with add0 / accum), dW_e 2.4e-6; per channel dW_dw 1.7e-7, dgamma 7.7e-6, dbeta 1.2e-7, dx 8.5e-7, rows of dW_e 1.8e-5.
                                                   class                 d err/bound  per channel: dW_dw  dgamma   dbeta    dW_e     dx
  nch 1, hidden 8     (2, 8, 8, 20, 40)            (1, 1, F, "", F)      0.033                     6.8e-8 1.0e-7   6.6e-8   2.2e-6   2.2e-7
  nch 1, hidden 32    (1, 16, 32, 4, 8)            (1, 1, T, "", F)      0.027                     1.3e-7 3.9e-7   1.2e-7   9.3e-7   4.6e-7
  3 + 1 chunks, 104   (2, 8, 104, 28, 56)          (1, 4, F, "", F)      0.040                     1.0e-7 3.4e-7   7.2e-8   9.4e-6   4.9e-7
  3 + 1 chunks, 128   (1, 16, 128, 40, 72)         (1, 4, T, "", F)      0.048                     9.8e-8 4.9e-7   5.7e-8   4.3e-6   5.0e-7
  3 + 2, 3 + 3        nch 5 and 6, small planes                          <= 0.052                  1.3e-7 1.5e-6   9.7e-8   6.7e-6   7.2e-7
  bwd loop (b)        24 cases 3 x 344 | 348 x 8   (., 4..6, ., "b", .)  <= 0.084                  1.6e-7 2.5e-6   6.5e-8   1.5e-5   8.5e-7
  stats, fwd, bwd,    (2, 24, 168, 164, 208)       (2, 6, F, "sfbm", T)  0.028                     1.0e-7 8.2e-7   6.0e-8   1.8e-5   6.4e-7
    moments loops
  stats, bwd,         (3, 8, 8, 152, 296)          (1, 1, F, "sbmx", F)  0.037                     4.5e-8 1.1e-7   3.5e-8   1.7e-6   3.5e-7
    moments, fix
The rows of dW_e are the one figure near its gate: dW_e = A G + B (W_e M) + D s is exact algebra but a difference of large sums, G
in fp32 partial rows, and with ReLU'd (non-negative) inputs M and s are large: 1.1e-5 to 1.8e-5 of a row's maximum in six such cases,
against 2.4e-6 of the tensor's.  It is deterministic from run to run (no atomics on that path) and inside 2e-5, but without the
factor 4.  No defect was found in conv_irt.hip."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hip_ops import DEV, cst_affine, dev, relerr  # noqa: E402
from starcop_amd import _lib  # noqa: E402
from starcop_amd._lib import (ACT_NONE, ACT_RELU, ACT_RELU6, SC_CST, SRC_AFFINE, SRC_BNBWD, SRC_RAW, check, make_src, ptr, sc_irt_args,  # noqa: E402
                              stream)
from test_gpu_irt import EPS, _reference, _switch_margin  # noqa: E402

U = 2.0 ** -24
D3 = 4 * U + 2.0 ** -31
MARGIN = 2e-5
BAND = 256
CAPS = dict(N=3, pixels=4096)            # an ordinary case; only the rows flagged "big" exceed it
LOOPS = "sfbmx"                          # stats, fwd, bwd (tiles_per_wg > 1), moments, fix
# per tensor: 4 x the worst per-channel error measured over the table on the MI355X (MEASURED_WORST; the factor allows for the fp64-atomic
# order of dw_acc, which varies from run to run, and for other seeds), never above the aggregate gate of 2e-5
MEASURED_WORST = dict(dW_dw=1.7e-7, dgamma=7.7e-6, dbeta=1.2e-7, dW_e=1.8e-5, dx=8.5e-7)
PER_CHANNEL_GATE = {k: min(4 * v, 2e-5) for k, v in MEASURED_WORST.items()}


def geo_class(g, hidden):
    """the geometry class of a block from the dict of _lib.irt_geometry"""
    trips = (g["pixel_blocks"] > 4 * g["stats_grid"], g["fwd_tiles"] > g["fwd_grid"], g["tiles_per_wg"] > 1, g["mom_ksteps"] > 16,
             g["pixel_blocks"] > 4 * g["fix_grid"])
    return (g["nks"], g["nch"], hidden % 32 == 0, "".join(l for l, t in zip(LOOPS, trips) if t), g["bwd_tiles"] % g["tiles_per_wg"] != 0)


# ---- the case table.  Rows: (class, N, Cin, hidden, H, W, flags).  Flags: the input source raw | affine | relu | relu6 (AFFINE with
# that activation); bnb6 | bnbn = a BNBWD gradient source with ACT_RELU6 | ACT_NONE; fix4 = all four (add0, accum) modes of
# sc_irt_bwd_fix; nostats = also sc_irt_fwd(stats_d = NULL); ragged = off all the tilings (checked by the host test); palette inputs; big.
_HIDDEN_PARTIAL = {1: 8, 2: 40, 3: 72, 4: 104, 5: 136, 6: 168}
# (N, H, W) per nch: the smallest plane, planes off the 4 x 16 output tiles and the 4 x 32 input tiles, several tiles per image
_SMALL = {1: ((1, 4, 8), (2, 20, 40)), 2: ((2, 16, 64), (3, 12, 24)), 3: ((2, 8, 32), (3, 20, 40)), 4: ((1, 40, 72), (2, 28, 56)),
          5: ((1, 32, 64), (1, 28, 40)), 6: ((1, 16, 32), (3, 12, 40))}
_SMALL_FLAGS = {(1, True): "relu6 fix4", (1, False): "relu fix4", (2, True): "raw nostats", (2, False): "affine nostats ragged",
                (3, True): "affine", (3, False): "raw bnb6 ragged", (4, True): "relu fix4 nostats", (4, False): "affine fix4 ragged",
                (5, True): "raw", (5, False): "relu6 bnbn ragged", (6, True): "affine fix4", (6, False): "raw fix4 ragged"}


def _rows():
    rows = []
    for nks in (1, 2):
        for nch in range(1, 7):
            for full in (True, False):
                hd = 32 * nch if full else _HIDDEN_PARTIAL[nch]
                cin = {(1, True): 16, (1, False): 8, (2, True): 32, (2, False): 24}[(nks, full)]
                n, h, w = _SMALL[nch][0 if full else 1]
                rows.append(((nks, nch, full, "", False), n, cin, hd, h, w, _SMALL_FLAGS[(nch, full)]))
    # narrow planes: 3 x 86 | 87 tiles of 4 x 32 on 512 / 2 = 256 work-groups per chunk group
    for nks in (1, 2):
        for nch in (4, 5, 6):
            for full in (True, False):
                hd = 32 * nch if full else _HIDDEN_PARTIAL[nch]
                cin = {(1, True): 8, (1, False): 16, (2, True): 24, (2, False): 32}[(nks, full)]
                for short in (False, True):
                    fl = ("raw", "affine", "relu6", "relu")[(nch + full + 2 * short) % 4] + (" fix4" if nch == 5 and short else "")
                    rows.append(((nks, nch, full, "b", short), 3, cin, hd, 348 if short else 344, 8, fl + " palette"))
    rows.append(((2, 6, False, "sfbm", True), 2, 24, 168, 164, 208, "relu bnb6 fix4 nostats ragged palette big"))
    rows.append(((1, 1, False, "sbmx", False), 3, 8, 8, 152, 296, "raw bnbn fix4 nostats palette big"))
    return rows


CASES = _rows()


def flags_of(case):
    return set(case[6].split())


def source_of(case):
    return next(f for f in ("raw", "affine", "relu", "relu6") if f in flags_of(case))


def case_id(case):
    cls, N, Cin, Hd, H, W, fl = case
    return f"N{N}_Cin{Cin}_Hd{Hd}_{H}x{W}_" + fl.replace(" ", "-")


def is_ragged(case):
    """off the 4 x 16 output tiles of k_irt_fwd in both directions and off the 4 x 32 input tiles of k_irt_bwd"""
    _, N, Cin, Hd, H, W, _ = case
    return (H // 2) % 4 != 0 and (W // 2) % 16 != 0 and W % 32 != 0


# ---- inputs and references (CPU) ----------------------------------------------------------------------------------------------------
def make_inputs(case):
    """fp32 host tensors of a case, at the first seed whose float64 BatchNorm outputs keep MARGIN from the ReLU6 switches"""
    cls, N, Cin, Hd, H, W, _ = case
    fl, src = flags_of(case), source_of(case)
    spread = 3.0 if src in ("relu", "relu6") else 1.5
    base = 1000 + 7 * Cin + Hd + H + W
    for seed in range(base, base + 200):
        g = torch.Generator().manual_seed(seed)
        if "palette" in fl:
            P = 256 if Cin == 8 else 64
            pal = torch.randn(P, Cin, generator=g) * spread + 0.2
            x = pal[torch.randint(0, P, (N, H, W), generator=g)].permute(0, 3, 1, 2).contiguous()
        else:
            x = torch.randn(N, Cin, H, W, generator=g) * spread + 0.2
        if src == "raw":
            xs, xh = torch.ones(Cin), torch.zeros(Cin)
        else:
            xs, xh = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.3
        xa = (x.double() * xs.double()[None, :, None, None] + xh.double()[None, :, None, None]).float()      # one fma, one rounding
        if src in ("relu", "relu6"):
            xa = xa.clamp(0.0, 6.0 if src == "relu6" else float("inf"))
        We = torch.randn(Hd, Cin, generator=g) * (2.0 / Cin) ** 0.5
        Wd = torch.randn(Hd, 3, 3, generator=g) * 0.2 + 0.3      # taps of both signs, a sum well away from 0 (see make_gradient)
        gam, bet = torch.rand(Hd, generator=g) + 0.5, torch.randn(Hd, generator=g) * 0.5 + 1.0
        margin = _switch_margin(xa, torch.ones(Cin), torch.zeros(Cin), We, gam, bet)
        if margin > MARGIN:
            break
    else:
        raise AssertionError("no seed with a safe ReLU6 margin")
    t = dict(x=x, xs=xs, xh=xh, xa=xa, We=We, Wd=Wd, gam=gam, bet=bet, margin=margin, seed=seed)
    return t


def make_gradient(case, t, d):
    """the gradient of the depthwise output d (the float64 reference) -> t["R"], as a RAW tensor or as the parts of a BNBWD source.
    It is the gradient of the loss |d|^2 / 2, i.e. d itself (BNBWD: B d + a small A [mask] g + D with B in [0.5, 1.5], d being the
    aux tensor, as in the network): dgamma and dbeta are then sums of mostly one sign.  With a gradient independent of the forward
    pass they are cancelling sums of random signs, and the element-wise relative error of such a sum measures its condition number
    (|sum| against the sum of magnitudes; 200 to 500 for some channel of 192), not the kernel: 4.6e-5 was measured that way."""
    _, N, Cin, Hd, H, W, _ = case
    fl = flags_of(case)
    d32 = d.float()
    if not fl & {"bnb6", "bnbn"}:
        t["R"] = d32.double()
        return
    # dy = A [lo < scale d + shift < hi] g + B d + D on load; the BatchNorm outputs of the aux tensor stay 5e-4 off the thresholds
    g = torch.Generator().manual_seed(t["seed"] + 2)
    gd = torch.randn(d32.shape, generator=g) * 0.2
    cb = torch.zeros(Hd, SC_CST)
    cb[:, 0], cb[:, 1] = torch.rand(Hd, generator=g) * 0.5 + 0.25, torch.randn(Hd, generator=g)
    cb[:, 2], cb[:, 3], cb[:, 4] = torch.rand(Hd, generator=g) + 0.5, torch.rand(Hd, generator=g) + 0.5, torch.randn(Hd, generator=g) * 0.1
    c = [cb[:, k].double()[None, :, None, None] for k in range(5)]
    yh = d32.double() * c[0] + c[1]
    near = (yh.abs() < 1e-3) | ((yh - 6).abs() < 1e-3)
    draw = torch.where(near, ((1.0 - c[1]) / c[0]).float().expand_as(d32), d32)
    yh = draw.double() * c[0] + c[1]
    assert float(torch.minimum(yh.abs(), (yh - 6).abs()).min()) > 5e-4
    passed = ((yh > 0) & (yh < 6)) if "bnb6" in fl else torch.ones_like(yh, dtype=torch.bool)
    t.update(gd=gd, draw=draw, cb=cb, R=torch.where(passed, gd.double(), torch.zeros((), dtype=torch.float64)) * c[2] + draw.double() * c[3] + c[4])


def forward_reference(t, nks):
    """float64 e and the teacher-forced constants; d from those fp32 constants, and the element-wise bound of d"""
    xa, We, Wd = t["xa"].double(), t["We"].double(), t["Wd"].double()
    Hd = We.shape[0]
    e = F.conv2d(xa, We[:, :, None, None])
    mean, var = e.mean((0, 2, 3)), e.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    cst = torch.zeros(Hd, SC_CST, dtype=torch.float64)
    cst[:, 0], cst[:, 1], cst[:, 2], cst[:, 3] = t["gam"].double() * invstd, t["bet"].double() - mean * t["gam"].double() * invstd, mean, invstd
    cst = cst.float()
    sc, sh = cst[:, 0].double()[None, :, None, None], cst[:, 1].double()[None, :, None, None]
    y = sc * e + sh
    eh = y.clamp(0.0, 6.0)
    d = F.conv2d(eh, Wd[:, None], stride=2, padding=1, groups=Hd)
    n = 6 * 16 * nks + 2
    de = (D3 + n * U) * F.conv2d(xa.abs(), We.abs()[:, :, None, None])
    dy = sc.abs() * de + U * y.abs()
    bound = F.conv2d(dy, Wd.abs()[:, None], stride=2, padding=1, groups=Hd) + 10 * U * F.conv2d(eh, Wd.abs()[:, None], stride=2, padding=1, groups=Hd)
    return dict(e=e, cst=cst, d=d, bound=bound)


def per_channel(got, ref, keep):
    """(worst over channels of max |got - ref| / that channel's max |ref|, channels measured against the tensor's maximum, channels);
    keep = the axes that index a channel"""
    ref = ref.detach().double().cpu()
    diff = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    red = [i for i in range(ref.dim()) if i not in keep]
    dmax, rmax = (diff.amax(red), ref.abs().amax(red)) if red else (diff, ref.abs())
    tmax = ref.abs().max()
    low = rmax < 1e-3 * tmax
    return float((dmax / torch.where(low, tmax, rmax)).max()), int(low.sum()), low.numel()


# ---- device side -------------------------------------------------------------------------------------------------------------------
class Guarded:
    """a tensor that is a view inside a NaN-filled allocation with BAND elements either side"""

    def __init__(self, shape, dtype=torch.float32, fill=float("nan")):
        n = 1
        for s in shape:
            n *= int(s)
        self.n = n
        self.buf = torch.full((n + 2 * BAND,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.buf[BAND:BAND + n].view(*shape)
        if fill == fill:
            self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool(torch.isnan(self.buf[:BAND]).all()) and bool(torch.isnan(self.buf[BAND + self.n:]).all())


def run_case(lib, case):
    cls, N, Cin, Hd, H, W, _ = case
    fl, src = flags_of(case), source_of(case)
    S, Ho, Wo = 2, H // 2, W // 2
    geo = _lib.irt_geometry(N, Cin, Hd, H, W, S)
    assert geo is not None and lib.sc_irt_supported(Cin, Hd, H, W, S) == 1
    assert geo_class(geo, Hd) == cls, (geo_class(geo, Hd), cls, geo)
    assert geo["stats_grid"] == lib.sc_irt_rows(0, N, H, W, S) and geo["fwd_tiles"] == lib.sc_irt_rows(1, N, H, W, S)
    assert geo["bwd_rows"] == lib.sc_irt_bwd_rows(N, Hd, H, W)
    t = make_inputs(case)
    fw = forward_reference(t, geo["nks"])
    make_gradient(case, t, fw["d"])
    bw = _reference(t["xa"], torch.ones(Cin), torch.zeros(Cin), t["We"], t["Wd"], t["gam"], t["bet"], t["R"], S)
    tag = f"irt-variant {case_id(case)} class {cls} seed {t['seed']} margin {t['margin']:.1e}:"

    xd, Wed, Wdd, cst_e = dev(t["x"]), dev(t["We"]), dev(t["Wd"]), dev(fw["cst"])
    a = sc_irt_args()
    if src == "raw":
        a.x = make_src(xd, Cin, SRC_RAW)
    else:
        a.x = make_src(xd, Cin, SRC_AFFINE, act={"affine": ACT_NONE, "relu": ACT_RELU, "relu6": ACT_RELU6}[src], cst=cst_affine(t["xs"], t["xh"]))
    a.w_expand, a.w_dw, a.cst_expand = Wed.data_ptr(), Wdd.data_ptr(), cst_e.data_ptr()
    a.N, a.Cin, a.hidden, a.H, a.W, a.stride = N, Cin, Hd, H, W, S
    st = stream()
    guards = {}
    # ---- (A) statistics of e
    stats = guards["stats_e"] = Guarded((geo["stats_grid"], Hd, 2))
    check(lib.sc_irt_expand_stats(C.byref(a), ptr(stats.t), st))
    tot = stats.t.double().sum(0).cpu()
    e_s1, e_s2 = relerr(tot[:, 0], fw["e"].sum((0, 2, 3))), relerr(tot[:, 1], (fw["e"] ** 2).sum((0, 2, 3)))
    # ---- (B) forward
    d_out = guards["d_out"] = Guarded((N, Hd, Ho, Wo))
    stats_d = guards["stats_d"] = Guarded((geo["fwd_tiles"], Hd, 2))
    check(lib.sc_irt_fwd(C.byref(a), ptr(d_out.t), ptr(stats_d.t), st))
    got_d = d_out.t.double().cpu()
    assert bool(torch.isfinite(got_d).all()), tag + " d has unwritten elements"
    err = (got_d - fw["d"]).abs()
    ratio = float(torch.where(fw["bound"] > 0, err / fw["bound"].clamp_min(1e-300), torch.zeros(())).max())
    e_d = relerr(d_out.t, fw["d"])
    totd = stats_d.t.double().sum(0).cpu()
    d_s1, d_s2 = relerr(totd[:, 0], got_d.sum((0, 2, 3))), relerr(totd[:, 1], (got_d ** 2).sum((0, 2, 3)))
    print(tag, f"d error / bound {ratio:.3f} aggregate {e_d:.1e}  statistics e {e_s1:.1e} {e_s2:.1e}  d {d_s1:.1e} {d_s2:.1e}")
    assert bool((err <= fw["bound"]).all()), (tag, ratio)
    assert e_d < 1e-5 and max(e_s1, e_s2, d_s1, d_s2) < 2e-5
    if "nostats" in fl:
        d2 = guards["d_out2"] = Guarded((N, Hd, Ho, Wo))
        before = stats_d.buf.clone()
        check(lib.sc_irt_fwd(C.byref(a), ptr(d2.t), None, st))
        assert torch.equal(d2.t, d_out.t), tag + " the inference forward writes other bits"
        assert torch.equal(stats_d.buf.view(torch.int32), before.view(torch.int32))
    # ---- (C) backward
    if fl & {"bnb6", "bnbn"}:
        dy = make_src(dev(t["gd"]), Hd, SRC_BNBWD, act=ACT_RELU6 if "bnb6" in fl else ACT_NONE, cst=dev(t["cb"]), aux=dev(t["draw"]))
    else:
        dy = make_src(dev(t["R"].float()), Hd, SRC_RAW)
    esums = guards["esums"] = Guarded((geo["bwd_rows"], Hd, 2), dtype=torch.float64)
    dwacc = guards["dw_acc"] = Guarded((Hd, 9), dtype=torch.float64, fill=0.0)
    work = guards["work"] = Guarded((lib.sc_irt_bwd_workspace_floats(N, Cin, Hd, H, W),))
    check(lib.sc_irt_xmoments(C.byref(a), ptr(work.t), st))
    check(lib.sc_irt_bwd(C.byref(a), C.byref(dy), ptr(esums.t), ptr(dwacc.t), ptr(work.t), st))
    cstb = torch.zeros(Hd, SC_CST, device=DEV)
    dgam, dbet = torch.empty(Hd, device=DEV), torch.empty(Hd, device=DEV)
    check(lib.sc_bn_bwd_finalize(ptr(esums.t), geo["bwd_rows"], float(N * H * W), ptr(cst_e), ptr(dgam), ptr(dbet), ptr(cstb), Hd, st))
    dx = guards["dx"] = Guarded((N, Cin, H, W))
    check(lib.sc_irt_bwd_fix(C.byref(a), ptr(cstb), ptr(work.t), ptr(dx.t), None, 0, st))
    agg = dict(dW_dw=relerr(dwacc.t.reshape(Hd, 3, 3), bw["dWd"]), dgamma=relerr(dgam, bw["dgam"]), dbeta=relerr(dbet, bw["dbet"]),
               dx=relerr(dx.t, bw["dx"]))
    if "fix4" in fl:
        g = torch.Generator().manual_seed(t["seed"] + 1)
        add, prev = torch.randn(N, Cin, H, W, generator=g), torch.randn(N, Cin, H, W, generator=g)
        addd = dev(add)
        for name, use_add, accum in (("dx+add", True, 0), ("dx+prev", False, 1), ("dx+add+prev", True, 1)):
            o = guards[name] = Guarded((N, Cin, H, W))
            o.t.copy_(prev if accum else torch.full((), float("nan")))
            check(lib.sc_irt_bwd_fix(C.byref(a), ptr(cstb), ptr(work.t), ptr(o.t), ptr(addd) if use_add else None, accum, st))
            agg[name] = relerr(o.t, bw["dx"] + (add.double() if use_add else 0.0) + (prev.double() if accum else 0.0))
    dWe = guards["dW_e"] = Guarded((Hd, Cin))
    check(lib.sc_irt_wgrad_finalize(C.byref(a), ptr(cstb), ptr(work.t), ptr(dWe.t), st))
    agg["dW_e"] = relerr(dWe.t, bw["dWe"])
    pc = dict(dW_dw=per_channel(dwacc.t.reshape(Hd, 3, 3), bw["dWd"], (0,)), dgamma=per_channel(dgam, bw["dgam"], (0,)),
              dbeta=per_channel(dbet, bw["dbet"], (0,)), dW_e=per_channel(dWe.t, bw["dWe"], (0,)), dx=per_channel(dx.t, bw["dx"], (0, 1)))
    nlow, nchan = sum(v[1] for v in pc.values()), sum(v[2] for v in pc.values())
    print(tag, "aggregate", " ".join(f"{k} {v:.1e}" for k, v in agg.items()), "| per channel", " ".join(f"{k} {v[0]:.1e}" for k, v in pc.items()),
          f"| low {nlow}/{nchan}")
    torch.cuda.synchronize()
    bad = [k for k, gd_ in guards.items() if not gd_.intact()]
    assert not bad, (tag, "guard bands overwritten", bad)
    assert max(agg.values()) < 2e-5, (tag, agg)
    assert nlow < 0.05 * nchan, (tag, nlow, nchan)
    for k, v in pc.items():
        assert v[0] < PER_CHANNEL_GATE[k], (tag, k, v, PER_CHANNEL_GATE[k])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_irt_geometry_class_vs_fp64(hip, case):
    run_case(hip, case)
