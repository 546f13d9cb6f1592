"""Every kernel variant the sub-pixel decoder launchers can reach (conv_sp.hip, conv_spw.hip, conv_sp_pack.h), against float64,
element by element.

sc_conv3x3_sp and sc_conv3x3_sp_dgrad pick among 8 instantiations each of k_conv3_sp / k_conv3_spd<TW, BF, NPP>, the data gradient
with three epilogue paths; sc_conv3x3_sp_wgrad picks k_spw_gemm<1 | 2>.  The host queries sc_sp_variant, sc_spd_variant and
sc_sp_wgrad_variant name the instantiation, and the launchers switch on the same functions.  Here every code they can return under the
default dispatch has a plain case, a ragged case, the features it accepts and exact probes; every case asserts the code it was written
for before it launches.  tests/test_sp_variants_host.py holds the tables below to the swept set of codes on a box without a GPU, which
is why the tables, the argument builders and the code helpers sit at module level and touch no device.

Codes (M = 4: two fp16 terms, 1: one bf16 term; TW = 32 from 32 low-resolution columns, else 16; NPP = pixel groups per wave):
  sp      100 (TW / 16) + 10 NPP + M                      tile = 128 NPP / TW rows x TW columns of the low-resolution plane
  spd     1000 skip_mode + the same                       0: no out1, 1: virtual skip channels (sc_spd_vskip_ok), 2: skip tiles
  spw     CB of k_spw_gemm<CB>                            2 above 64 up-sampled channels
NPP = 2 needs more than 128 work-groups: N x 256-pixel tiles x channel tiles (32 outputs forward; 128 up-sampled channels + 32 skip
channels per skip tile in the data gradient).  Those cases use the smallest planes just past the threshold ("big").

Reference: the same operation in float64 on the CPU from the same fp32 inputs.  The prologue value is formed as the kernels form it
(each fma in float64, rounded to fp32 once), then F.conv2d(cat([nearest_up2, skip])) / conv_transpose2d and the 2x2 sum / autograd.
Inputs that feed a ReLU / ReLU6 mask are moved off the thresholds; no element is excluded from any comparison.

(a) Element-wise bound (u = 2^-24; S = the same operation on the magnitudes, taken on the 3x3 taps: it bounds the phase sums, since
    sum |taps| >= |Wph|):        |out - ref| <= (d + n u) S + floor
  d   M = 4: h0 g0 + h0 g1 + h1 g0 kept, h1 g1 <= 2^-22 dropped (sc_split.h);  M = 1: a0 b0 kept, a0 b1 and a1 b0 dropped: 2^-8.
  n   the fp32 additions an element can see.  Forward: a phase runs 4 slots (a, b) per 16-channel chunk, the skip source has four
      parity chunks per 16 channels: 4 x (padded C0 + 4 x padded C1) x products per pair (3, 1), + 3 for the fp32 sum of up to four
      taps that forms a phase filter (conv_sp_pack.h), + 8 for prologue and epilogue.  Data gradient: 4 parity chunks x 4 slots x padded
      dy channels x products + 3 + 8.  Weight gradient: N Hl Wl x (products + 1) -- the low-resolution pixels, and no more K slices than
      pixels -- + 3 for the 2x2 box sum + 8.
  floor (M = 4), the sub-normal second term of an operand, 2^-25 after its power-of-two scale: activations 2^-25 / h_act_scale, i.e.
      2^-26 by default and 2^-25 in the xbound case (max |x| = 3e4 -> scale 1; the one-bf16-term kernels have no scale and must
      ignore the hint: their xbound case shows only that); filters 2^-25 / 2^6 = 2^-31 (SP_SW = 64: a phase filter
      is a sum of up to four taps, so these kernels scale by 2^6, not 2^8); gradients floor_grad(absmax) = 2^(e-30); the box sums of
      the weight gradient are scaled by h_grad_scale<3>, a quarter of that: 2^(e-28), once per low-resolution pixel.  Each operand's
      floor is convolved with the other operand's magnitudes (weight gradient: floor_x sum |dy[co]| + floor_S sum |x[ci]|, every dy
      pixel being in one box per tap).
  accum0 / accum1 add u (|prev| + |result|).  Statistics rows (summed here in float64): 136 u of the summed magnitudes + the element
  bounds, the row bound of tests/test_gpu_conv3_variants.py -- a row is a tile of at most 256 x 4 outputs per channel, summed as a tree
  of depth 4 + 5 + 8.
(b) The project's aggregate gates, unchanged: relerr < BX3_TOL (M = 4); M = 1: 5e-6 against _sp_phase_reference on bf16-rounded operands
    (forward and, through its autograd, the data gradient) and 2e-2 against the unrounded layer; forward M = 4: error <= 3 x the 3x3
    two-fp16-term kernel's + 1e-7 where sc_conv3x3_bx3 accepts the case (a first source of a multiple of 16 channels, or no skip).
(c) Exact probes, one of each kind per code at its ragged shape.  Unit impulses, one per input channel with disjoint footprints (counted
    in low-resolution cells), on the first and last row and column, on both sides of the tile seams in low-resolution coordinates and,
    for full-resolution tensors (the skip source, dy: 21 channels), in all four parities (qy, qx) on both sides of the doubled ROW
    seam and on both sides of the doubled COLUMN seam (seam_points: 20 wanted pixels, none may be dropped) -- against a
    random filter ("fprobe" / "wprobe"); one-hot power-of-two filters against a random input ("aprobe"); for the weight gradient
    impulses in dy ("wprobe") and in the low-resolution input ("xprobe"), where channels never mix, so positions may repeat.
    What each probe produces (v = the exact value, D = 2^-22 for M = 4, 2^-8 for M = 1):
      forward  fprobe   up-sampled source: PHASE SUMS of up to four taps          D S + 3 u S + 2^-31      (the pack adds the taps in fp32)
                        skip source: single taps                                  D |v| + 2^-31
               aprobe   single products 2^k x (both sources: a phase filter with one non-zero tap is that tap)     D |v| + 2^-26 2^k
      dgrad    fprobe   (impulses in dy)  dprev: phase sums                      D S + 3 u S + 2^-31;    dskip: single taps  D |v| + 2^-31
               aprobe   (one-hot filters) dprev: 2x2 sums of four products       D S + 3 u S + 4 2^-25 2^k;    dskip: single products
      wgrad    wprobe   (impulses in dy)  single products x[ci][q]               D |v| + 2^-26
               xprobe   (impulses in x)   2x2 box sums of four dy values         D S + 3 u S + 2^-23      (h_grad_scale<3> without a hint: 1/4)
    An exact 0 must be 0 (S = 0 there).  The probes run without absmax, so the gradient scale is the fallback.
Every case prints error / bound before it asserts."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import hip_ops  # noqa: E402
from hip_ops import DEV, dev, relerr  # noqa: E402
from starcop_amd import _lib  # noqa: E402
from starcop_amd._lib import TERMS_F16X2, check, ptr, sc_conv_args, sc_wgrad_args, stream  # noqa: E402
from test_gpu_conv3_variants import (D_PROBE, D_SPLIT, FLOOR_GRAD1, PRODUCTS, U, _FAKE, _gscale, _host_src, _onehot_filter, floor_grad,
                                     make_operand, to_src, up2, within)  # noqa: E402
from test_gpu_ops import BX3_TOL, _sp_phase_reference, rnd  # noqa: E402

FLOOR_W_SP = 2.0 ** -31
XB_MAX = 3.0e4                                     # the largest activation of the xbound cases
KNOBS = ("STARCOP_SP_NPP",)
CAPS = dict(N=3, pixels=4096, C=160, wgs_big=160)  # low-resolution pixels N Hl Wl of an ordinary case; work-groups of a big one
OP_SP, OP_SPD, OP_SPW = "sp", "spd", "spw"

# ---- case tables.  Rows: (code, N, channels, Cc, H, W, sources, flags); H x W is the full-resolution size.
#   sp   channels = (C0 up-sampled, C1 skip), Cc = Cout; sources "a+b" = the modes of src[0] (half resolution) and src[1], raw | affine
#   spd  channels = (Cup, Cskip), Cc = the channels of dy (the layer's outputs); sources = the mode of dy: bnbwd | bnbwd6 | ident
#   spw  channels = (Cup, Cin - Cup), Cc = Cout; sources = (mode of dy, mode of the input)
# Flags: ragged, big (NPP = 2), stats, batched (the one-launch pack), xbound, accum, g3e-8 / g2e4 (absmax is always given with M = 4
# outside the probes), fprobe / aprobe / wprobe / xprobe.
#            (tw, npp): plain (N, H, W, Cout), ragged (N, H, W, Cout)
_SP_SHAPES = {(2, 1): ((2, 16, 64, 32), (3, 20, 68, 40)),
              (1, 1): ((2, 16, 32, 32), (3, 20, 36, 40)),
              (2, 2): ((3, 48, 192, 160), (3, 44, 132, 136)),        # 9 tiles x 5 = 135 work-groups
              (1, 2): ((3, 288, 32, 160), (3, 148, 36, 136))}        # 9 x 5 = 135; 10 x 5 = 150
#            (tw, npp, four channel tiles): plain (N, H, W), ragged (N, H, W)
_SPD_SHAPES = {(2, 1, 0): ((2, 16, 64), (3, 20, 68)), (2, 1, 1): ((2, 16, 64), (3, 20, 68)),
               (1, 1, 0): ((2, 16, 32), (3, 20, 36)), (1, 1, 1): ((2, 16, 32), (3, 20, 36)),
               (2, 2, 0): ((3, 176, 256), (3, 172, 196)),            # 44 tiles: 132 work-groups
               (1, 2, 0): ((3, 1408, 32), (3, 692, 36)),             # 44 tiles
               (2, 2, 1): ((3, 176, 64), (3, 88, 68)),               # 11 tiles x 4 = 132; 12 x 4 = 144
               (1, 2, 1): ((3, 352, 32), (3, 180, 36))}
# (Cup, Cskip) per skip mode: plain, ragged (small), plain, ragged (big: ntu + nts = 4 in mode 2)
_SPD_CH = {0: ((128, 0), (40, 0), (32, 0), (40, 0)), 1: ((32, 16), (40, 13), (32, 16), (40, 13)), 2: ((32, 32), (40, 21), (32, 96), (40, 70))}


def _sp_rows(code):
    tw, npp = (code // 100) % 10, (code // 10) % 10
    (n0, h0, w0, c0), (n1, h1, w1, c1) = _SP_SHAPES[(tw, npp)]
    b = "big " if npp == 2 else ""
    return [(code, n0, (16, 16), c0, h0, w0, "affine+raw", b + "stats"),
            (code, n1, (13, 13), c1, h1, w1, "raw+affine", b + "ragged stats batched"),
            (code, n0, (32, 0), c0, h0, w0, "affine", b + "stats batched"),
            (code, n0, (16, 16), c0, h0, w0, "raw+raw", b + "xbound"),
            (code, n0, (32, 0), c0, h0, w0, "raw", b + "stats"),
            (code, n1, (11, 21), c1, h1, w1, "raw+raw", b + "ragged fprobe"),
            (code, n1, (11, 21), c1, h1, w1, "raw+raw", b + "ragged aprobe batched")]


def _spd_rows(code):
    mode, tw, npp, m = code // 1000, (code // 100) % 10, (code // 10) % 10, code % 10
    big = npp == 2
    (n0, h0, w0), (n1, h1, w1) = _SPD_SHAPES[(tw, npp, int(big and mode == 2))]
    chp, chr_ = _SPD_CH[mode][2 * big], _SPD_CH[mode][2 * big + 1]
    b = "big " if big else ""
    rows = [(code, n0, chp, 16, h0, w0, "bnbwd", b.strip()),
            (code, n1, chr_, 13, h1, w1, "bnbwd6", b + "ragged accum batched" + (" g3e-8" if m == 4 else ""))]
    if m == 4:
        rows.append((code, n0, chp, 16, h0, w0, "bnbwd6", b + "g2e4 batched"))
    return rows + [(code, n1, chr_, 21, h1, w1, "ident", b + "ragged fprobe"),      # (21 dy channels: one per wanted pixel of seam_points)
                   (code, n1, chr_, 21, h1, w1, "ident", b + "ragged aprobe batched")]


SP_CODES = [100 * tw + 10 * npp + m for tw in (1, 2) for npp in (1, 2) for m in (1, 4)]
SPD_CODES = [1000 * mode + c for mode in (0, 1, 2) for c in SP_CODES]
SP_CASES = [r for code in SP_CODES for r in _sp_rows(code)]
SPD_CASES = [r for code in SPD_CODES for r in _spd_rows(code)]
# ragged weight gradients: K = 3 x 15 x 50 = 2250 (Kp = 2272: a zero tail of 22; 71 stages in slices of 2, the last one of 1), 9 x 13 = 117
SPW_CASES = [
    (1, 2, (64, 0), 32, 16, 64, ("bnbwd", "affine"), ""),
    (1, 3, (40, 9), 13, 30, 100, ("bnbwd6", "raw"), "ragged g3e-8"),
    (1, 3, (64, 8), 13, 30, 100, ("raw", "affine"), "ragged g2e4"),
    (1, 2, (40, 0), 32, 16, 64, ("affine", "raw"), ""),
    (1, 3, (40, 9), 21, 30, 100, ("ident", "raw"), "ragged wprobe"),
    (1, 3, (40, 9), 13, 30, 100, ("raw", "raw"), "ragged xprobe"),
    (2, 2, (128, 0), 32, 16, 64, ("bnbwd", "affine"), ""),
    (2, 3, (136, 9), 13, 30, 100, ("bnbwd6", "raw"), "ragged g3e-8"),
    (2, 3, (65, 8), 13, 30, 100, ("raw", "affine"), "ragged g2e4"),
    (2, 2, (72, 0), 32, 16, 64, ("affine", "raw"), ""),
    (2, 3, (136, 9), 21, 30, 100, ("ident", "raw"), "ragged wprobe"),
    (2, 3, (136, 9), 13, 30, 100, ("raw", "raw"), "ragged xprobe"),
]
CASES = {OP_SP: SP_CASES, OP_SPD: SPD_CASES, OP_SPW: SPW_CASES}


# ---- code helpers (host only)
def flags_of(case):
    return set(case[7].split())


def terms_of(op, code):
    return 4 if op == OP_SPW else code % 10


def tile_of(code):
    """(rows, columns) of the work-group's low-resolution tile"""
    tw, npp = 16 * ((code // 100) % 10), (code // 10) % 10
    return 128 * npp // tw, tw


def split_srcs(srcs):
    return tuple(srcs.split("+")) if "+" in srcs else (srcs, None)


def sp_args(N, chans, Cout, H, W, srcs, flags, terms):
    """sc_conv_args of a forward case with placeholder pointers: what the host query looks at"""
    m0, m1 = split_srcs(srcs)
    a = sc_conv_args()
    a.nsrc = 2 if m1 else 1
    a.src[0] = _host_src(chans[0], m0, 1)
    if m1:
        a.src[1] = _host_src(chans[1], m1)
    a.wpk, a.out0 = _FAKE, _FAKE
    a.N, a.H, a.W, a.Cout, a.ks, a.co_t, a.csplit = N, H, W, Cout, 3, 32, Cout
    a.terms = TERMS_F16X2 if terms == 4 else terms
    a.stats = _FAKE if "stats" in flags else None
    return a


def spd_args(N, chans, Co, H, W, mode, flags, terms):
    """sc_conv_args of a data-gradient case: dy has Co channels, the outputs are out0 (Cup, half resolution) and out1 (Cskip)"""
    a = sc_conv_args()
    a.nsrc = 1
    a.src[0] = _host_src(Co, mode)
    a.wpk, a.out0 = _FAKE, _FAKE
    a.out1 = _FAKE if chans[1] else None
    a.N, a.H, a.W, a.Cout, a.ks, a.co_t, a.csplit = N, H, W, chans[0] + chans[1], 3, 32, chans[0]
    a.terms = TERMS_F16X2 if terms == 4 else terms
    a.accum0 = 1 if "accum" in flags else 0
    a.accum1 = 1 if "accum" in flags and chans[1] else 0
    return a


def spw_args(N, chans, Cout, H, W, srcs, flags, terms):
    a = sc_wgrad_args()
    a.dy = _host_src(Cout, srcs[0])
    a.nsrc = 1
    a.src[0] = _host_src(chans[0], srcs[1], 1)
    a.N, a.H, a.W, a.Cout, a.Cin, a.ks = N, H, W, Cout, chans[0] + chans[1], 3
    a.terms = TERMS_F16X2 if terms == 4 else terms
    a.dw = _FAKE
    return a


def query(op, a):
    lib = _lib.load()
    return {OP_SP: lib.sc_sp_variant, OP_SPD: lib.sc_spd_variant, OP_SPW: lib.sc_sp_wgrad_variant}[op](C.byref(a))


def case_args(op, case):
    code, N, chans, Cc, H, W, srcs, fl = case
    return {OP_SP: sp_args, OP_SPD: spd_args, OP_SPW: spw_args}[op](N, chans, Cc, H, W, srcs, set(fl.split()), terms_of(op, code))


def case_code(op, case):
    """the code the host query answers for a table row"""
    return query(op, case_args(op, case))


def channel_tiles(op, case):
    """the channel tiles of a launch: 32 outputs (forward); 128 up-sampled channels + 32 skip channels per skip tile (data gradient)"""
    code, _, (ca, cb), Cc = case[:4]
    if op == OP_SP:
        return -(-Cc // 32)
    return -(-ca // 128) + (-(-cb // 32) if code // 1000 == 2 else 0)


def work_groups2(op, case):
    """work-groups of the launch with 256-pixel tiles: what the NPP rule compares with 128"""
    N, H, W = case[1], case[4], case[5]
    Hl, Wl = H // 2, W // 2
    tiles = -(-Wl // 32) * -(-Hl // 8) if Wl >= 32 else -(-Wl // 16) * -(-Hl // 16)
    return N * tiles * channel_tiles(op, case)


def spw_plan(N, H, W, Cout, Cup):
    """(K, Kp, cb, mtiles, ntiles, kstages, nsl) of spw_plan in conv_spw.hip"""
    K = N * (H // 2) * (W // 2)
    Kp = -(-K // 32) * 32
    cb = 2 if Cup > 64 else 1
    mt, nt = -(-9 * Cout // 256), -(-Cup // (64 * cb))
    stages = Kp // 32
    want = max(1, min(-(-768 // (mt * nt)), 64, stages))
    kst = -(-stages // want)
    return K, Kp, cb, mt, nt, kst, -(-stages // kst)


def act_scale(M):
    """h_act_scale of sc_split.h for the bound M"""
    if not M * 2.0 > 32752.0:
        return 2.0
    return 2.0 ** (math.frexp(32752.0 / M)[1] - 1)


# ---- impulse placement
def _cells(kind, y, x):
    """the low-resolution cells (y0, y1, x0, x1) an impulse's 3x3 footprint touches: "lo" = a pixel of the half-resolution source
    (its 2x2 block of copies reaches the full-resolution rows 2y-1 .. 2y+2), "hi" = a full-resolution pixel"""
    if kind == "lo":
        return y - 1, y + 1, x - 1, x + 1
    return (y - 1) // 2, (y + 1) // 2, (x - 1) // 2, (x + 1) // 2


def seam_points(Hl, Wl, th, tw):
    """wanted impulse pixels in priority order -> (lo, hi).  lo: both sides of the tile seam, the corners (6 pixels).  hi: the corners, every parity
    (qy, qx) on both sides of the doubled row seam (low-resolution rows th-1 | th) AND on both sides of the doubled column seam
    (low-resolution columns tw-1 | tw), and the corners: 4 + 8 + 8 = 20 pixels.  Every entry is a list of candidates, the preferred
    one first: a seam pixel may slide ALONG its seam (never off it) to find room."""
    lo = [[p] for p in ((th - 1, tw - 1), (th, tw), (0, 0), (0, Wl - 1), (Hl - 1, 0), (Hl - 1, Wl - 1))]
    hi = [[p] for p in ((0, 0), (0, 2 * Wl - 1), (2 * Hl - 1, 0), (2 * Hl - 1, 2 * Wl - 1))]      # (fixed pixels first)
    for k, (qy, qx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        for row, c0 in ((th - 1, 4 * k), (th, 4 * k + 2)):
            hi.append([(2 * row + qy, 2 * ((c0 + t) % Wl) + qx) for t in range(Wl)])
    for k, (qy, qx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        for col, r0 in ((tw - 1, 2 * k), (tw, 2 * k + 1)):
            hi.append([(2 * ((r0 + t) % Hl) + qy, 2 * col + qx) for t in range(Hl)])
    return lo, hi


def impulse_plan(N, Hl, Wl, th, tw, n_lo, n_hi):
    """one impulse per channel: [(image, y, x)] for n_lo half-resolution and n_hi full-resolution channels, no two footprints of one
    image sharing a low-resolution cell.  The wanted pixels of seam_points come first -- a tensor that gets impulses must have a channel
    for each of them, and each must find room --, then a lattice."""
    lo, hi = seam_points(Hl, Wl, th, tw)
    assert n_lo == 0 or n_lo >= len(lo), (n_lo, len(lo), "fewer channels than wanted pixels")
    assert n_hi == 0 or n_hi >= len(hi), (n_hi, len(hi), "fewer channels than wanted pixels")
    lo, hi = lo[:n_lo], hi[:n_hi]
    used = [[] for _ in range(N)]
    got = {"lo": [], "hi": []}

    def put(kind, y, x, first):
        r = _cells(kind, y, x)
        for t in range(N):
            n = (first + t) % N
            if all(r[1] < q[0] or q[1] < r[0] or r[3] < q[2] or q[3] < r[2] for q in used[n]):
                used[n].append(r)
                got[kind].append((n, y, x))
                return True
        return False

    for k, cands in enumerate(lo):
        assert any(put("lo", y, x, k) for y, x in cands), ("no room for", "lo", cands[0])
    for cands in hi:
        assert any(put("hi", y, x, 0) for y, x in cands), ("no room for", "hi", cands[0])
    lattice = [(y, x) for y in range(1, Hl, 3) for x in range(1, Wl, 3)]
    for kind, want, f in (("lo", n_lo, 1), ("hi", n_hi, 2)):
        for k, (y, x) in enumerate(lattice):
            if len(got[kind]) >= want:
                break
            put(kind, f * y + (k & 1) * (f - 1), f * x + ((k >> 1) & 1) * (f - 1), k)
        assert len(got[kind]) == want, (kind, want, len(got[kind]), "too few impulse positions")
    return got["lo"], got["hi"]


def impulse_tensor(N, C_, H, W, plan):
    x = torch.zeros(N, C_, H, W)
    for c, (n, y_, x_) in enumerate(plan):
        x[n, c, y_, x_] = 1.0
    return x


def cycled_plan(N, C_, points):
    """weight-gradient probes: channels never mix, so channel c takes the c-th wanted pixel (cyclically) in image c % N"""
    assert C_ >= len(points), (C_, len(points), "fewer channels than wanted pixels")
    return [(c % N, *points[c % len(points)]) for c in range(C_)]


def fwd_probe_plans(case):
    code, N, (C0, C1), _, H, W = case[:6]
    th, tw = tile_of(code)
    return impulse_plan(N, H // 2, W // 2, th, tw, C0, C1)


def dgrad_probe_plan(case):
    code, N, _, Co, H, W = case[:6]
    th, tw = tile_of(code)
    return impulse_plan(N, H // 2, W // 2, th, tw, 0, Co)[1]


def wgrad_probe_plans(case):
    """(dy impulses, input impulses): the seams are those of the 8 x 32 tile of k_spw_dysum"""
    _, N, (Cup, _), Cout, H, W = case[:6]
    lo, hi = seam_points(H // 2, W // 2, 8, 32)
    fl = flags_of(case)
    return (cycled_plan(N, Cout, [c[0] for c in hi]) if "wprobe" in fl else None), (cycled_plan(N, Cup, [c[0] for c in lo]) if "xprobe" in fl else None)


def case_id(case):
    code, N, chans, Cc, H, W, srcs, fl = case
    s = srcs if isinstance(srcs, str) else "~".join(srcs)
    return f"{code}-{N}x{chans[0]}+{chans[1]}x{Cc}x{H}x{W}-{s}-{fl.replace(' ', '+')}".rstrip("-")


# ---- the runs
def _check(op, kind, name, got, ref, bound):
    r = within(name, got, ref, bound)
    print(f"SPMAX {op} {kind} {r:.4f}")
    return r


def _pack_written(wpk, m):
    """the pack buffer is prefilled with fp32 NaN, whose upper half is a NaN as fp16 and as bf16 too: every 16-bit term must be finite"""
    return bool(torch.isfinite(wpk.view(torch.float16 if m == 4 else torch.bfloat16).float()).all())


def _pool(t):
    return F.avg_pool2d(t, 2) * 4


def run_sp(lib, case):
    code, N, (C0, C1), Cout, H, W, srcs, flag_s = case
    fl = set(flag_s.split())
    name = f"sp {case_id(case)}"
    m = code % 10
    Hl, Wl, K = H // 2, W // 2, C0 + C1
    m0, m1 = split_srcs(srcs)
    probe = "fprobe" in fl or "aprobe" in fl
    v0 = v1 = None
    if "fprobe" in fl:
        lo, hi = fwd_probe_plans(case)
        v0, v1 = impulse_tensor(N, C0, Hl, Wl, lo), impulse_tensor(N, C1, H, W, hi)
    elif "xbound" in fl:
        v0 = rnd(N, C0, Hl, Wl, seed=1)
        v0 = v0 * (XB_MAX / float(v0.abs().max()))
    s0 = make_operand(m0, N, C0, Hl, Wl, seed=1, values=v0)
    s1 = make_operand(m1, N, C1, H, W, seed=20, values=v1) if m1 else None
    xup = up2(s0["val"]).double()
    xin = torch.cat([xup, s1["val"].double()], 1) if m1 else xup
    w = _onehot_filter(Cout, K, 1) if "aprobe" in fl else rnd(Cout, K, 3, 3, seed=2, scale=0.2)
    wd_ = w.double()
    ref = F.conv2d(xin, wd_, padding=1)
    S = F.conv2d(xin.abs(), wd_.abs(), padding=1)
    # the launch
    a = sp_args(N, (C0, C1), Cout, H, W, srcs, fl, m)
    assert query(OP_SP, a) == code, (query(OP_SP, a), code)
    a.src[0] = to_src(s0, C0, up=1)
    if m1:
        a.src[1] = to_src(s1, C1)
    terms = TERMS_F16X2 if m == 4 else 1
    wpk = hip_ops.pack_sp(dev(w), C0, batched="batched" in fl, terms=terms)
    assert _pack_written(wpk, m)
    a.wpk = wpk.data_ptr()
    out = torch.full((N, Cout, H, W), float("nan"), device=DEV)
    a.out0 = out.data_ptr()
    rows = lib.sc_sp_stat_rows(N, H, W, Cout)
    th, tw = tile_of(code)
    assert rows == N * -(-Hl // th) * -(-Wl // tw), (rows, th, tw)
    stats = torch.full((rows, Cout, 2), float("nan"), device=DEV) if "stats" in fl else None
    a.stats = stats.data_ptr() if stats is not None else None
    hs = 2.0
    if "xbound" in fl:
        xb = [dev(torch.tensor([s0["amax"]])), dev(torch.tensor([s1["amax"]]))]
        a.xbound[0], a.xbound[1] = xb[0].data_ptr(), xb[1].data_ptr()
        if m == 4:      # (the one-bf16-term kernels have fp32's range and no activation scale: they must ignore the hint)
            hs = act_scale(max(s0["amax"], s1["amax"]))
            assert hs != 2.0, "the xbound case must leave the default activation scale"
    check(lib.sc_conv3x3_sp(C.byref(a), stream()))
    torch.cuda.synchronize()
    fa = 2.0 ** -25 / hs
    if probe:
        bound = D_PROBE[m] * S
        if "fprobe" in fl:
            bound = bound + 3 * U * F.conv2d(xup.abs(), wd_[:, :C0].abs(), padding=1)
        if m == 4:
            bound = bound + (S > 0) * (FLOOR_W_SP if "fprobe" in fl else fa * 8.0)      # (8: the largest one-hot tap)
        _check(OP_SP, "fprobe" if "fprobe" in fl else "aprobe", name, out, ref, bound)
        return
    n = 4 * (-(-C0 // 16) * 16 + 4 * -(-C1 // 16) * 16) * PRODUCTS[m] + 3 + 8
    bound = (D_SPLIT[m] + n * U) * S
    if m == 4:
        bound = bound + fa * F.conv2d(torch.ones(1, K, H, W, dtype=torch.float64), wd_.abs(), padding=1) \
            + FLOOR_W_SP * F.conv2d(xin.abs().sum(1, keepdim=True), torch.ones(1, 1, 3, 3, dtype=torch.float64), padding=1)
    _check(OP_SP, "out", name, out, ref, bound)
    dims = (0, 2, 3)
    if stats is not None:
        ns = 32 * 4 + 8
        st = stats.double().sum(0).cpu()
        _check(OP_SP, "stats", name + " sum", st[:, 0], ref.sum(dims), ns * U * (ref.abs() + bound).sum(dims) + bound.sum(dims))
        _check(OP_SP, "stats", name + " sumsq", st[:, 1], (ref ** 2).sum(dims),
               ns * U * ((ref.abs() + bound) ** 2).sum(dims) + (2 * ref.abs() * bound + bound ** 2).sum(dims))
    # (b): the aggregate gates
    e = relerr(out, ref)
    print(f"SPGATE {name} relerr {e:.3e}")
    if m == 1:
        rb = lambda t: t.float().bfloat16().double()
        ref_r = _sp_phase_reference(s0["val"], s1["val"] if m1 else None, w, rb)
        assert relerr(out, ref_r) < 5e-6 and e < 2e-2, (relerr(out, ref_r), e)
        return
    assert e < BX3_TOL
    if C0 % 16 == 0 or not m1:
        co_t = 64 if Cout > 32 else 32
        a3 = sp_args(N, (C0, C1), Cout, H, W, srcs, fl - {"stats"}, 4)
        a3.src[0], a3.src[1], a3.co_t = a.src[0], a.src[1], co_t
        a3.xbound[0], a3.xbound[1] = a.xbound[0], a.xbound[1]
        w3 = hip_ops.pack_bx3(dev(w), co_t, 0, TERMS_F16X2)
        o3 = torch.full((N, Cout, H, W), float("nan"), device=DEV)
        a3.wpk, a3.out0 = w3.data_ptr(), o3.data_ptr()
        check(lib.sc_conv3x3_bx3(C.byref(a3), stream()))
        e3 = relerr(o3, ref)
        print(f"SPGATE {name} 3x3 kernel relerr {e3:.3e}")
        assert e < 3 * e3 + 1e-7, (e, e3)


def run_spd(lib, case):
    code, N, (Cup, Csk), Co, H, W, mode, flag_s = case
    fl = set(flag_s.split())
    name = f"spd {case_id(case)}"
    m, smode = code % 10, code // 1000
    Hl, Wl, K = H // 2, W // 2, Cup + Csk
    gs = _gscale(fl)
    probe = "fprobe" in fl or "aprobe" in fl
    gv = impulse_tensor(N, Co, H, W, dgrad_probe_plan(case)) if "fprobe" in fl else None
    d = make_operand(mode, N, Co, H, W, seed=1, gscale=gs, values=gv)
    w = _onehot_filter(K, Co, 1).transpose(0, 1).contiguous() if "aprobe" in fl else rnd(Co, K, 3, 3, seed=2, scale=0.2)
    wd_, dyv = w.double(), d["val"].double()
    full = F.conv_transpose2d(dyv, wd_, padding=1)
    Sf = F.conv_transpose2d(dyv.abs(), wd_.abs(), padding=1)
    a = spd_args(N, (Cup, Csk), Co, H, W, mode, fl, m)
    assert query(OP_SPD, a) == code, (query(OP_SPD, a), code)
    assert smode == (0 if not Csk else (1 if lib.sc_spd_vskip_ok(Cup, Csk) else 2))
    a.src[0] = to_src(d, Co)
    terms = TERMS_F16X2 if m == 4 else 1
    wpk = hip_ops.pack_spd(dev(w), Cup, batched="batched" in fl, vskip=smode == 1, terms=terms, skip_tiles=smode == 2)
    assert _pack_written(wpk, m)
    a.wpk = wpk.data_ptr()
    prev0 = rnd(N, Cup, Hl, Wl, seed=30) * gs if a.accum0 else None
    prev1 = rnd(N, Csk, H, W, seed=31) * gs if a.accum1 else None
    out0 = dev(prev0).clone() if prev0 is not None else torch.full((N, Cup, Hl, Wl), float("nan"), device=DEV)
    out1 = None
    if Csk:
        out1 = dev(prev1).clone() if prev1 is not None else torch.full((N, Csk, H, W), float("nan"), device=DEV)
    a.out0, a.out1 = out0.data_ptr(), out1.data_ptr() if out1 is not None else None
    amax = None
    if m == 4 and not probe:
        amax = torch.tensor([d["amax"]], device=DEV)
        a.absmax = amax.data_ptr()
    check(lib.sc_conv3x3_sp_dgrad(C.byref(a), stream()))
    torch.cuda.synchronize()
    r0, r1 = _pool(full[:, :Cup]), full[:, Cup:]
    if probe:
        bf_ = D_PROBE[m] * Sf
        if m == 4:
            bf_ = bf_ + (Sf > 0) * (FLOOR_W_SP if "fprobe" in fl else FLOOR_GRAD1 * 8.0)
        b0, b1 = _pool(bf_[:, :Cup]) + 3 * U * _pool(Sf[:, :Cup]), bf_[:, Cup:]
    else:
        n = 16 * -(-Co // 16) * 16 * PRODUCTS[m] + 3 + 8
        bf_ = (D_SPLIT[m] + n * U) * Sf
        if m == 4:
            one = torch.ones(1, 1, 3, 3, dtype=torch.float64)
            bf_ = bf_ + floor_grad(d["amax"]) * F.conv_transpose2d(torch.ones(1, Co, H, W, dtype=torch.float64), wd_.abs(), padding=1) \
                + FLOOR_W_SP * F.conv_transpose2d(dyv.abs().sum(1, keepdim=True), one, padding=1)
        b0, b1 = _pool(bf_[:, :Cup]), bf_[:, Cup:]
    if prev0 is not None:
        b0 = b0 + U * (prev0.double().abs() + r0.abs() + b0)
        r0 = r0 + prev0.double()
    if prev1 is not None:
        b1 = b1 + U * (prev1.double().abs() + r1.abs() + b1)
        r1 = r1 + prev1.double()
    kind = ("fprobe" if "fprobe" in fl else "aprobe") if probe else "out"
    _check(OP_SPD, kind, name + " dprev", out0, r0, b0)
    if Csk:
        _check(OP_SPD, kind, name + " dskip", out1, r1, b1)
    if probe:
        return
    errs = [relerr(out0, r0)] + ([relerr(out1, r1)] if Csk else [])
    print(f"SPGATE {name} relerr {max(errs):.3e}")
    if m == 4:
        assert max(errs) < BX3_TOL
        return
    assert max(errs) < 2e-2
    # the bf16-rounded operands through the same sub-pixel sums (autograd of _sp_phase_reference; linear, so accum adds prev)
    rb = lambda t: t.float().bfloat16().double()
    pv = torch.zeros(N, Cup, Hl, Wl, dtype=torch.float64, requires_grad=True)
    sk = torch.zeros(N, Csk, H, W, dtype=torch.float64, requires_grad=True) if Csk else None
    _sp_phase_reference(pv, sk, w, lambda t: t.double() if t.requires_grad or t.grad_fn is not None else rb(t)).backward(rb(d["val"]))
    e0 = relerr(out0, pv.grad + (prev0.double() if prev0 is not None else 0))
    e1 = relerr(out1, sk.grad + (prev1.double() if prev1 is not None else 0)) if Csk else 0.0
    print(f"SPGATE {name} relerr on bf16-rounded operands {max(e0, e1):.3e}")
    assert e0 < 5e-6 and e1 < 5e-6, (e0, e1)


def run_spw(lib, case):
    code, N, (Cup, Cx), Cout, H, W, (dym, xm), flag_s = case
    fl = set(flag_s.split())
    name = f"spw {case_id(case)}"
    Hl, Wl, Cin = H // 2, W // 2, Cup + Cx
    gs = _gscale(fl)
    probe = "wprobe" in fl or "xprobe" in fl
    plans = wgrad_probe_plans(case)
    dv = impulse_tensor(N, Cout, H, W, plans[0]) if "wprobe" in fl else None
    xv = impulse_tensor(N, Cup, Hl, Wl, plans[1]) if "xprobe" in fl else None
    d = make_operand(dym, N, Cout, H, W, seed=1, gscale=gs, values=dv)
    s0 = make_operand(xm, N, Cup, Hl, Wl, seed=10, values=xv)
    xin, dyv = up2(s0["val"]).double(), d["val"].double()

    def grad(x_, dy_):
        w_ = torch.zeros(Cout, Cup, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(x_, w_, padding=1).backward(dy_)
        return w_.grad
    ref, S = grad(xin, dyv), grad(xin.abs(), dyv.abs())
    a = spw_args(N, (Cup, Cx), Cout, H, W, (dym, xm), fl, 4)
    assert query(OP_SPW, a) == code, (query(OP_SPW, a), code)
    a.dy = to_src(d, Cout)
    a.src[0] = to_src(s0, Cup, up=1)
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
    a.dw = dw.data_ptr()
    if not probe:
        amax = torch.tensor([d["amax"]], device=DEV)
        a.absmax = amax.data_ptr()
    nb = lib.sc_sp_wgrad_workspace_bytes(N, H, W, Cout, Cup)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    check(lib.sc_conv3x3_sp_wgrad(C.byref(a), ptr(ws), nb, stream()))
    torch.cuda.synchronize()
    if Cx:
        assert bool(torch.isnan(dw[:, Cup:]).all()), "the skip channels' columns are not this entry point's"
    if probe:
        bound = D_PROBE[4] * S + (S > 0) * (2.0 ** -26 if "wprobe" in fl else 4 * FLOOR_GRAD1)
        if "xprobe" in fl:
            bound = bound + 3 * U * S
        _check(OP_SPW, "wprobe" if "wprobe" in fl else "xprobe", name, dw[:, :Cup], ref, bound)
        return
    n = N * Hl * Wl * (PRODUCTS[4] + 1) + 3 + 8
    bound = (D_SPLIT[4] + n * U) * S + 2.0 ** -26 * dyv.abs().sum((0, 2, 3))[:, None, None, None] \
        + 4 * floor_grad(d["amax"]) * s0["val"].double().abs().sum((0, 2, 3))[None, :, None, None]
    _check(OP_SPW, "out", name, dw[:, :Cup], ref, bound)
    e = relerr(dw[:, :Cup], ref)
    print(f"SPGATE {name} relerr {e:.3e}")
    assert e < BX3_TOL


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """a failed assertion is one finding; a device error would fail every later case too: end the session there"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, nothing more is launched: {e}", returncode=3)


@pytest.mark.parametrize("case", SP_CASES, ids=case_id)
def test_sp_variant(hip, case):
    run_sp(hip, case)


@pytest.mark.parametrize("case", SPD_CASES, ids=case_id)
def test_spd_variant(hip, case):
    run_spd(hip, case)


@pytest.mark.parametrize("case", SPW_CASES, ids=case_id)
def test_sp_wgrad_variant(hip, case):
    run_spw(hip, case)
