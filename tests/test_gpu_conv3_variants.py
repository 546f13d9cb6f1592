"""Every kernel variant the 3x3 matrix-core launchers of conv_bx3.hip can reach, against float64, element by element.

sc_conv3x3_bx3, sc_conv3x3_thin16, sc_conv3x3_wgrad_bx3 and sc_conv3x3_wgrad_thin16 pick among about fifty template instantiations.
The host queries sc_conv3_variant, sc_thin16_variant, sc_wgrad3_variant and sc_wgrad_thin16_variant name the instantiation, and the
launchers switch on the same functions.  Here every code they can return under the default dispatch has a plain case, a ragged case
and exact probes; every case asserts the code it was written for before it launches.  tests/test_conv3_variants_host.py holds the
tables below to the swept set of codes on a box without a GPU, which is why the tables, the argument builders and the code helpers
sit at module level and touch no device.  (An up-sampled 32-channel RAW / AFFINE source of the thin forward always takes the sub-pixel
kernel 1200; code 200 is the 32-channel source that is not up-sampled.)

Codes (M = 1, 2, 3 bf16 terms per operand, 4 = two fp16 terms):
  conv3   1000 WS + 100 Q + 10 BNB + M          Q = co_t / 32, BNB = BatchNorm-backward source (the data gradient), WS = k_conv3_ws
  thin    100 (C / 16) + 10 BNB (k_conv3_thin_h), 1200 = k_conv3_thin_sp (up-sampled 32 channels), 2110 = k_conv3_thin_spd (down0)
  wgrad3  10000 PIPE + 1000 M + 100 WM + 10 NCI + R      R: the pipelined kernel sums its K parts itself
  wthin   100 (Cin / 16) + 10 BNB

Reference: the same operation in float64 on the CPU from the same fp32 inputs.  The prologue value is formed as sc_pro_affine /
sc_pro_bnbwd form it (each fma evaluated in float64 and rounded to fp32 once), then F.conv2d / conv_transpose2d / autograd in float64.
Inputs that feed a ReLU / ReLU6 mask are moved off the thresholds; no element is excluded from any comparison.

(a) Element-wise bound, from the arithmetic of sc_split.h (u = 2^-24, S = the float64 convolution of the operands' magnitudes):
        |out - ref| <= (d + n u) S + floor
  d, the weight of the products the split drops (p-bit terms: bf16 p = 8, fp16 p = 11; a term t_i of an operand a is <= 2^(-p i) |a|):
      M = 1   a0 b0 kept; a0 b1 and a1 b0 (<= 2^-8 each, 2^-9 on average, independent signs) dropped     d = 2^-8
      M = 2   a0 b0 + a0 b1 + a1 b0 kept; a1 b1 <= 2^-16 dropped                                    d = 2^-16
      M = 3   three 8-bit terms hold an fp32 significand exactly; the six products of weight >= 2^-24 are kept, a1 b2 and a2 b1
              (2^-24 each) and a2 b2 (2^-32) dropped                                                d = 3 u
      M = 4   h0 g0 + h0 g1 + h1 g0 kept; h1 g1 <= 2^-22 dropped                                   d = 2^-22
    The remainder of an operand behind its last term has the same weight as the dropped product; over the >= 72 products of a random
    case these do not add up coherently, so the constants above are kept as they stand (the probes of (c) see single products).
  n, the fp32 additions an element can see: 9 x padded channels x products per pair (1, 3, 6, 3) + 8 for the prologue and epilogue;
      weight gradients: N H W x (products per pair + 1) -- the pixels, and no more K parts and slices than pixels -- + 8.
  floor (M = 4 only), the sub-normal second term of an operand, 2^-25 after its power-of-two scale s: activations s = 2 -> 2^-26,
      filters s = 2^8 -> 2^-33, gradients s = 2^(5-e) with 2^e > absmax >= 2^(e-1) -> 2^(e-30) (s = 1 without the hint: 2^-25).
      Each operand's floor is convolved with the other operand's magnitudes.
  add0 / accum add u |prev|; the 2x2 sums of down0 add their bounds and 3 u of the summed magnitudes.
  Statistics rows (32 x 4 pixels each, summed here in float64) and the bnr rows: 136 u of the summed magnitudes + the element bounds.
(b) The project's aggregate gates, unchanged: relerr < BX3_TOL (M = 3, 4) against float64; error <= 3 x the fp32 MFMA kernel's + 1e-7
    (2e-7 for weight gradients) where that kernel accepts the case; M = 1: 5e-6 against the bf16-rounded operands and 2e-2; M = 2: 2e-5.
(c) Exact probes, one of each kind per code at its ragged shape.  Unit impulses (different channels, footprints disjoint, on the
    first and last row and column and on both sides of the tile seams) against a random filter, one-hot power-of-two filters against a
    random input, and the two mirror images for the weight gradients.  Every output is then a single product v (or exactly 0), and
        |out - v| <= 0 (M = 3: bit for bit),  2^-22 |v| + floor (M = 4),  2^-16 |v| (M = 2),  2^-8 |v| (M = 1)
    -- one operand of the product is a power of two, so only the other's remainder is left.  Where the launch sums up to four such
    products (an up-sampled source, the 2x2 sums of down0) three fp32 additions are allowed for: + 3 u S.
    A power of two has one term, so such a probe never needs a product of two low-order terms.  With three bf16 terms the filter
    probe of sc_conv3x3_bx3 therefore gives the impulses of the odd channels the value 1 + 2^-10 and cuts their filter values to 13
    bits: a 24-bit product, still exact, that needs a1 b1 -- the first product of the chain.  The weight-gradient probes do the same
    with the impulses of image 0.
Every case prints error / bound before it asserts."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import hip_ops  # noqa: E402
from hip_ops import DEV, dev, relerr  # noqa: E402
from starcop_amd import _lib  # noqa: E402
from starcop_amd._lib import (ACT_NONE, ACT_RELU, ACT_RELU6, SC_CST, SRC_AFFINE, SRC_BNBWD, SRC_RAW, STAT_CONV3, TERMS_F16X2, check,
                              make_src, ptr, sc_bnr_args, sc_conv_args, sc_src, sc_wgrad_args, stream)  # noqa: E402
from test_gpu_ops import BX3_TOL, rnd  # noqa: E402

U = 2.0 ** -24
D_SPLIT = {1: 2.0 ** -8, 2: 2.0 ** -16, 3: 3 * U, 4: 2.0 ** -22}      # (a): the dropped-product weight
D_PROBE = {1: 2.0 ** -8, 2: 2.0 ** -16, 3: 0.0, 4: 2.0 ** -22}        # (c): the remainder of the one inexact operand
PRODUCTS = {1: 1, 2: 3, 3: 6, 4: 3}
FLOOR_ACT, FLOOR_W, FLOOR_GRAD1 = 2.0 ** -26, 2.0 ** -33, 2.0 ** -25
KNOBS = ("STARCOP_BX3_WS_MINCHUNKS",)
CAPS = dict(N=3, H=40, W=72, C=96)
WIDE_AREA = 16 * 32

# ---- case tables.  Rows: (code, N, source channels (C0, C1), output channels, H, W, sources, flags).
# conv3 / thin sources: raw | affine (BatchNorm constants + ReLU) | bnbwd (ReLU mask) | bnbwd6 | ident (BNBWD with A = 1, B = D = 0 and
# an open mask: the probes' gradient source); "up:" = src[0] up-sampled 2x; "+raw" = a second, RAW source (C1 channels).  With a BNBWD
# source the launch is a data gradient: the filter is that of a layer with C0 output and `output channels` input channels, packed
# transposed and flipped.  Flags: ragged, wide (above the caps: the wave-specialised kernels), stats, add (add0 + accum0), csplit (two
# outputs), down0, bnr, g3e-8 / g2e4 (gradient magnitude; absmax is always given with M = 4 and a BNBWD source), fprobe (filter probe),
# aprobe (activation probe).


def _fwd_rows(code, wide):
    co_t = 32 * ((code // 100) % 10)
    w = "wide " if wide else ""
    k = 224 if wide else 0
    return [(code, 2 if not wide else 1, (32 + k, 0), co_t, 16, 32 if wide else 64, "affine", w + "stats"),
            (code, 3, (16 + k, 13), co_t + 8, 12, 34, "up:affine+raw", w + "ragged stats"),
            (code, 1, (24 + k, 0), 40, 8, 36, "up:affine", w.strip()),
            (code, 7 if wide else 3, (16 + k, 13), co_t + 8, 12, 34, "raw+raw", w + "ragged fprobe"),
            (code, 3, (16 + k, 13), co_t + 8, 12, 34, "raw+raw", w + "ragged aprobe")]


def _dgrad_rows(code, wide):
    co_t = 32 * ((code // 100) % 10)
    w = "wide " if wide else ""
    k = 220 if wide else 0
    g1, g2 = (" g3e-8", " g2e4") if code % 10 == 4 else ("", "")
    rows = [(code, 2 if not wide else 1, (32 + k + (4 if wide else 0), 0), co_t, 16, 32 if wide else 64, "bnbwd", w.strip()),
            (code, 3, (29 + k, 0), co_t + 8, 12, 34, "bnbwd6", w + "ragged add" + g1),
            (code, 2 if not wide else 1, (24 + k, 0), co_t + 16, 8, 36, "bnbwd", w + "csplit down0" + g2),
            (code, 7 if wide else 3, (29 + k, 0), co_t + 8, 12, 34, "ident", w + "ragged fprobe"),
            (code, 3, (29 + k, 0), co_t + 8, 12, 34, "ident", w + "ragged aprobe")]
    if not wide:      # (the wave-specialised kernels have no bnr epilogue: the dispatcher keeps those launches on k_conv3_bx3)
        rows.insert(3, (code, 2, (40, 0), co_t, 10, 34, "bnbwd6", "bnr"))
    return rows


CONV3_CASES = [r for q in (1, 2) for m in (1, 2, 3, 4) for r in _fwd_rows(100 * q + m, False)] + \
              [r for q in (1, 2) for r in _fwd_rows(1000 + 100 * q + 4, True)] + \
              [r for q in (1, 2) for m in (1, 2, 3, 4) for r in _dgrad_rows(100 * q + 10 + m, False)] + \
              [r for q in (1, 2) for r in _dgrad_rows(1000 + 100 * q + 14, True)]

THIN_CASES = [
    (100, 2, (16, 0), 16, 16, 64, "affine", "stats"), (100, 3, (16, 0), 9, 12, 66, "raw", "ragged stats"),
    (100, 1, (16, 0), 11, 12, 68, "up:affine", "ragged stats"),
    (100, 3, (16, 0), 9, 12, 66, "raw", "ragged fprobe"), (100, 3, (16, 0), 9, 12, 66, "raw", "ragged aprobe"),
    (110, 2, (16, 0), 16, 16, 64, "bnbwd", ""), (110, 3, (16, 0), 9, 12, 66, "bnbwd6", "ragged g3e-8"),
    (110, 1, (16, 0), 16, 12, 68, "bnbwd", "ragged bnr g2e4"),
    (110, 3, (16, 0), 9, 12, 66, "ident", "ragged fprobe"), (110, 3, (16, 0), 9, 12, 66, "ident", "ragged aprobe"),
    (200, 2, (32, 0), 16, 16, 64, "affine", "stats"), (200, 3, (32, 0), 9, 12, 34, "raw", "ragged stats"),
    (200, 3, (32, 0), 9, 12, 34, "raw", "ragged fprobe"), (200, 3, (32, 0), 9, 12, 34, "raw", "ragged aprobe"),
    (210, 2, (32, 0), 16, 16, 64, "bnbwd", ""), (210, 3, (32, 0), 9, 12, 34, "bnbwd6", "ragged g3e-8"),
    (210, 1, (32, 0), 16, 12, 36, "bnbwd", "ragged bnr g2e4"),
    (210, 3, (32, 0), 9, 12, 34, "ident", "ragged fprobe"), (210, 3, (32, 0), 9, 12, 34, "ident", "ragged aprobe"),
    (1200, 2, (32, 0), 16, 16, 64, "up:affine", "stats"), (1200, 3, (32, 0), 9, 12, 66, "up:raw", "ragged stats"),
    (1200, 3, (32, 0), 9, 12, 66, "up:raw", "ragged fprobe"), (1200, 3, (32, 0), 9, 12, 66, "up:raw", "ragged aprobe"),
    (2110, 2, (16, 0), 32, 16, 64, "bnbwd", "down0"), (2110, 3, (16, 0), 32, 12, 66, "bnbwd6", "ragged down0 accum g3e-8"),
    (2110, 1, (16, 0), 32, 12, 68, "bnbwd", "ragged down0 g2e4"),
    (2110, 3, (16, 0), 32, 12, 66, "ident", "ragged down0 fprobe"), (2110, 3, (16, 0), 32, 12, 66, "ident", "ragged down0 aprobe"),
]

# weight gradients.  Rows: (code, N, input channels (C0, C1), Cout, H, W, (dy, input sources), flags).  dy: raw | affine | bnbwd | bnbwd6 |
# ident; inputs: raw | affine | up:affine+raw (the concat of an up-sampled AFFINE source and a RAW one).  Flags: ragged, oddw / offset
# (the two ways a two-fp16-term launch with a BNBWD gradient leaves the pipelined kernel: an odd width; a gradient tensor 4 bytes off an
# 8-byte boundary), g3e-8 / g2e4, wprobe (impulses in dy), xprobe (impulses in the input).
_WG_TILE = {(1, 1): ((32, 32), (20, 19)), (1, 2): ((32, 64), (20, 41)), (2, 1): ((64, 32), (40, 19)), (2, 2): ((64, 64), (40, 41)),
            (1, 3): ((32, 96), (20, 81))}      # (WM, NCI) -> (Cout, Cin) plain, ragged


def _wgrad_rows(code):
    pipe, m, wm, nci = code // 10000, (code // 1000) % 10, (code // 100) % 10, (code // 10) % 10
    (co, ci), (cor, cir) = _WG_TILE[(wm, nci)]
    if pipe:
        return [(code, 2, (ci, 0), co, 8, 64, ("bnbwd", "raw"), ""),
                (code, 3, (cir, 0), cor, 13, 34, ("bnbwd6", "affine"), "ragged g3e-8"),
                (code, 2, (ci - 16, 16), co, 8, 36, ("bnbwd", "up:affine+raw"), "g2e4"),
                (code, 3, (cir, 0), cor, 13, 34, ("ident", "raw"), "ragged wprobe"),
                (code, 3, (cir, 0), cor, 13, 34, ("ident", "raw"), "ragged xprobe")]
    hf = m == 4      # a BNBWD gradient reaches the non-pipelined two-fp16-term kernels only past one of the pipeline's conditions
    return [(code, 2, (ci, 0), co, 8, 64, ("raw", "raw"), ""),
            (code, 3, (cir, 0), cor, 13, 35 if hf else 34, ("bnbwd6", "affine"), "ragged oddw g3e-8" if hf else "ragged"),
            (code, 3, (cir, 0), cor, 13, 34, ("bnbwd", "affine"), "ragged offset g2e4" if hf else "ragged"),
            (code, 2, (ci, 0), co, 8, 36, ("affine", "raw"), ""),
            (code, 2, (ci - 16, 16), co, 8, 36, ("bnbwd6" if not hf else "raw", "up:affine+raw"), ""),
            (code, 3, (cir, 0), cor, 13, 34, ("raw", "raw"), "ragged wprobe"),
            (code, 3, (cir, 0), cor, 13, 34, ("raw", "raw"), "ragged xprobe")]


WGRAD3_CODES = [1000 * m + 100 * wm + 10 * nci for m in (1, 2, 3, 4) for wm in (1, 2) for nci in (1, 2)] + [14111, 14121, 14210, 14221, 14131]
WGRAD3_CASES = [r for code in WGRAD3_CODES for r in _wgrad_rows(code)]


def _wthin_rows(code):
    cin, bnb = 16 * (code // 100), (code // 10) % 10
    d0, d1, dp = ("bnbwd", "bnbwd6", "ident") if bnb else ("raw", "affine", "raw")
    return [(code, 2, (cin, 0), 16, 16, 64, (d0, "raw"), ""),
            (code, 3, (cin, 0), 9, 10, 34, (d1, "affine"), "ragged g3e-8"),
            (code, 2, (cin, 0), 11, 12, 36, (d0 if bnb else d1, "up:affine"), "g2e4"),
            (code, 3, (cin, 0), 9, 10, 34, (dp, "raw"), "ragged wprobe"),
            (code, 3, (cin, 0), 9, 10, 34, (dp, "raw"), "ragged xprobe")]


WTHIN_CASES = [r for code in (100, 110, 200, 210) for r in _wthin_rows(code)]

OP_CONV3, OP_THIN, OP_WGRAD3, OP_WTHIN = "conv3", "thin", "wgrad3", "wthin"
CASES = {OP_CONV3: CONV3_CASES, OP_THIN: THIN_CASES, OP_WGRAD3: WGRAD3_CASES, OP_WTHIN: WTHIN_CASES}


# ---- code helpers (host only)
def flags_of(case):
    return set(case[7].split())


def terms_of(op, code):
    return (code // 1000) % 10 if op == OP_WGRAD3 else (code % 10 if op == OP_CONV3 else 4)


def co_t_of(op, code):
    return 32 * ((code // 100) % 10) if op == OP_CONV3 else 16


def tile_w(op, code):
    """columns of the work-group's pixel tile"""
    if op == OP_CONV3:
        return 32
    if op == OP_THIN:
        return 64 if code in (100, 110, 1200, 2110) else 32
    return 32


def tile_h(op):
    return {OP_CONV3: 8, OP_THIN: 8, OP_WGRAD3: 2, OP_WTHIN: 4}[op]


def parse_src(s):
    """'up:affine+raw' -> (up, mode of src[0], has a second RAW source)"""
    up = s.startswith("up:")
    s = s[3:] if up else s
    two = s.endswith("+raw")
    return up, (s[:-4] if two else s), two


_MODE = {"raw": SRC_RAW, "affine": SRC_AFFINE, "bnbwd": SRC_BNBWD, "bnbwd6": SRC_BNBWD, "ident": SRC_BNBWD}
_FAKE = 0x10000      # a non-NULL, 16-byte aligned address for the host queries (never dereferenced)


def _host_src(C_, mode, up=0, at=_FAKE):
    s = sc_src()
    s.x, s.C, s.mode, s.up = at, C_, _MODE[mode], int(up)
    s.cst = _FAKE if mode != "raw" else None
    s.aux = at if _MODE[mode] == SRC_BNBWD else None
    s.act = {"affine": ACT_RELU, "bnbwd": ACT_RELU, "bnbwd6": ACT_RELU6}.get(mode, ACT_NONE)
    return s


_HOST_KEEP = []


def conv_args(op, N, chans, Cout, H, W, srcs, flags, co_t, terms):
    """sc_conv_args of a conv3 / thin case with placeholder pointers: what the host queries look at"""
    up, mode, two = parse_src(srcs)
    a = sc_conv_args()
    a.nsrc = 2 if two else 1
    a.src[0] = _host_src(chans[0], mode, up)
    if two:
        a.src[1] = _host_src(chans[1], "raw")
    a.wpk, a.out0 = _FAKE, _FAKE
    a.N, a.H, a.W, a.Cout, a.ks, a.co_t = N, H, W, Cout, 3, co_t
    a.terms = TERMS_F16X2 if terms == 4 else terms
    a.csplit = csplit_of(Cout) if "csplit" in flags else Cout
    a.out1 = _FAKE if "csplit" in flags else None
    a.down0 = 1 if "down0" in flags else 0
    a.accum0 = 1 if ("add" in flags or "accum" in flags) else 0
    a.add0 = _FAKE if "add" in flags else None
    a.stats = _FAKE if "stats" in flags else None
    if "bnr" in flags:
        b = sc_bnr_args()
        b.y = b.cst = b.rows = b.absmax = _FAKE
        b.act = ACT_RELU
        _HOST_KEEP.append(b)
        a.bnr = C.addressof(b)
    return a


def wgrad_args(N, chans, Cout, H, W, srcs, flags, terms):
    """sc_wgrad_args of a weight-gradient case with placeholder pointers"""
    dym, xs = srcs
    up, mode, two = parse_src(xs)
    a = sc_wgrad_args()
    a.dy = _host_src(Cout, dym, at=_FAKE + (4 if "offset" in flags else 0))
    a.nsrc = 2 if two else 1
    a.src[0] = _host_src(chans[0], mode, up)
    if two:
        a.src[1] = _host_src(chans[1], "raw")
    a.N, a.H, a.W, a.Cout, a.Cin, a.ks = N, H, W, Cout, chans[0] + chans[1], 3
    a.terms = TERMS_F16X2 if terms == 4 else terms
    a.part, a.dw, a.part_floats = _FAKE, _FAKE, 1 << 40
    return a


def csplit_of(Cout):
    return max(8, Cout // 2 // 8 * 8)


def query(op, a):
    lib = _lib.load()
    fn = {OP_CONV3: lib.sc_conv3_variant, OP_THIN: lib.sc_thin16_variant, OP_WGRAD3: lib.sc_wgrad3_variant, OP_WTHIN: lib.sc_wgrad_thin16_variant}[op]
    return fn(C.byref(a))


def case_code(op, case):
    """the code the host query answers for a table row"""
    code, N, chans, Cout, H, W, srcs, fl = case
    fl = set(fl.split())
    if op in (OP_CONV3, OP_THIN):
        return query(op, conv_args(op, N, chans, Cout, H, W, srcs, fl, co_t_of(op, code), terms_of(op, code)))
    return query(op, wgrad_args(N, chans, Cout, H, W, srcs, fl, terms_of(op, code)))


def wgrad3_plan(N, H, W, Cout, Cin, allow96):
    """(wm, nci, kp, nsl) of plan_wgrad_bx3, for the ragged condition 'the slice count does not divide the tile count'"""
    wm = 2 if Cout > 32 else 1
    nci = 1 if Cin <= 32 else 2
    if allow96 and wm == 1 and 64 < Cin <= 96:
        nci = 3
    kp = 1 if nci * wm == 3 else 4 // (nci * wm)
    tiles = -(-Cout // (32 * wm)) * -(-Cin // (32 * nci))
    T = N * -(-W // 32) * -(-H // 2)
    nmax = min(max(T // 4, 1), 512)
    cost = [(-(-(tiles * k) // 256)) * (-(-T // k) + 6.0) for k in range(1, nmax + 1)]
    nsl = next(k for k in range(1, nmax + 1) if cost[k - 1] <= 1.03 * min(cost))
    return wm, nci, kp, nsl, T


def positions(H, W, tw, image=0, th=8):
    """impulse pixels with disjoint 3 x 3 footprints: a tile seam (rows th-1 | th, columns tw-1 | tw), the corners, then a lattice.  The
    two sides of the seams are neighbours, so they go to different images; every third image has the corners only (in a small plane
    the seam pixel displaces the last corner)."""
    seam = [[(th - 1, tw - 1)], [(th, tw)], []][image % 3]
    want = seam + [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    want += [(y, x) for y in range(1, H, 3) for x in range(1, W, 3)] + [(y, x) for y in range(0, H, 3) for x in range(0, W, 3)]
    got = []
    for y, x in want:
        if 0 <= y < H and 0 <= x < W and all(max(abs(y - q), abs(x - r)) >= 3 for q, r in got):
            got.append((y, x))
    return got


# ---- inputs and float64 references
def _bc(v):
    return v[None, :, None, None]


def _fma32(a, b, c):
    """fmaf(a, b, c) of fp32 tensors: the product is exact in float64, one rounding of the sum to float64 and one to fp32"""
    return (a.double() * b.double() + c.double()).float()


def _off_threshold(t, scale, shift, hi6):
    """move the elements of t whose scale * t + shift lies within 1e-3 of 0 (or 6) by 0.01 / scale; none may remain"""
    def near(v):
        p = v.double() * _bc(scale.double()) + _bc(shift.double())
        return (p.abs() < 1e-3) | (((p - 6).abs() < 1e-3) if hi6 else torch.zeros_like(p, dtype=torch.bool))
    t = torch.where(near(t), t + 0.01 / _bc(scale), t)
    assert not bool(near(t).any())
    return t


def make_operand(mode, N, C_, H, W, seed, gscale=1.0, values=None):
    """one source tensor -> dict(x, y, cst, mode, act, val = the fp32 value the prologue forms, amax = max |A g| under the mask).
    values: the raw tensor to use instead of a random one (the probes)."""
    x = values if values is not None else rnd(N, C_, H, W, seed=seed) * gscale
    if mode == "raw":
        return dict(x=x, y=None, cst=None, mode=SRC_RAW, act=ACT_NONE, val=x.clone(), amax=float(x.abs().max()))
    cst = torch.zeros(C_, SC_CST)
    if mode == "affine":
        sc, sh = rnd(C_, seed=seed + 1) * 0.3 + 1.0, rnd(C_, seed=seed + 2) * 0.3 * gscale
        x = _off_threshold(x, sc, sh, False)
        cst[:, 0], cst[:, 1] = sc, sh
        val = _fma32(x, _bc(sc), _bc(sh)).clamp_min(0)
        return dict(x=x, y=None, cst=cst, mode=SRC_AFFINE, act=ACT_RELU, val=val, amax=float(val.abs().max()))
    if mode == "ident":
        cst[:, 0], cst[:, 2] = 1.0, 1.0
        y = rnd(N, C_, H, W, seed=seed + 6)
        return dict(x=x, y=y, cst=cst, mode=SRC_BNBWD, act=ACT_NONE, val=x.clone(), amax=float(x.abs().max()))
    a, b = rnd(C_, seed=seed + 1) * 0.2 + 1.0, rnd(C_, seed=seed + 2) * 0.2
    A, B, D = rnd(C_, seed=seed + 3) * 0.5 + 1.0, rnd(C_, seed=seed + 4) * 0.1 * gscale, rnd(C_, seed=seed + 5) * 0.1 * gscale
    cst[:, 0], cst[:, 1], cst[:, 2], cst[:, 3], cst[:, 4] = a, b, A, B, D
    six = mode == "bnbwd6"
    y = _off_threshold(rnd(N, C_, H, W, seed=seed + 6, scale=2.0) + 1.5, a, b, six)
    yh = _fma32(y, _bc(a), _bc(b))
    mask = (yh > 0) & (yh < 6) if six else yh > 0
    gm = torch.where(mask, x, torch.zeros(()))
    val = _fma32(gm, _bc(A), _fma32(y, _bc(B), _bc(D)))
    return dict(x=x, y=y, cst=cst, mode=SRC_BNBWD, act=ACT_RELU6 if six else ACT_RELU, val=val, amax=float((gm * _bc(A)).abs().max()))


def to_src(d, C_, up=0, offset=False):
    def put(t):
        if not offset:
            return dev(t)
        buf = torch.empty(t.numel() + 4, device=DEV)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        hip_ops._KEEP.append(v)
        assert v.data_ptr() % 8 == 4
        return v
    return make_src(put(d["x"]), C_, d["mode"], act=d["act"], up=up, cst=dev(d["cst"]) if d["cst"] is not None else None,
                    aux=put(d["y"]) if d["y"] is not None else None)


def up2(t):
    return F.interpolate(t, scale_factor=2, mode="nearest")


def within(name, got, ref, bound):
    """element-wise |got - ref| <= bound with no NaN left; prints and returns the largest error-to-bound ratio"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
    err = (got - ref).abs()
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    print(f"C3RATIO {name} {ratio:.4f} maxerr {float(err.max()):.3e}")
    bad = err > bound
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements outside the bound, worst ratio {ratio:.3f}, first at {bad.nonzero()[0].tolist()}, " \
                                f"got {got[bad][0]:.9g} want {ref[bad][0]:.9g}"
    return ratio


def case_id(case):
    code, N, chans, Cout, H, W, srcs, fl = case
    s = srcs if isinstance(srcs, str) else "~".join(srcs)
    return f"{code}-{N}x{chans[0]}+{chans[1]}x{Cout}x{H}x{W}-{s}-{fl.replace(' ', '+')}".rstrip("-")


def _gscale(fl):
    return 3e-8 if "g3e-8" in fl else (2e4 if "g2e4" in fl else 1.0)


def _impulses(N, C_, H, W, tw, th=8):
    """one unit impulse per channel, channel c in image c % N at that image's (c // N)-th position"""
    pos = [positions(H, W, tw, n, th) for n in range(N)]
    x = torch.zeros(N, C_, H, W)
    for c in range(C_):
        assert c // N < len(pos[c % N]), (N, H, W, C_, "too few impulse positions")
        y_, x_ = pos[c % N][c // N]
        x[c % N, c, y_, x_] = 1.0
    return x


def floor_grad(amax):
    """the sub-normal floor of a gradient operand scaled by h_grad_scale(absmax): 2^-25 / 2^(5-e), amax = m 2^e with m in [0.5, 1)"""
    import math
    return 2.0 ** (math.frexp(amax)[1] - 30) if 0.0 < amax < 3.0e38 else FLOOR_GRAD1


def _cut13(t):
    """t rounded to 13 significant bits: two bf16 terms hold it, and its product with 1 + 2^-10 has 24 bits"""
    mant, expo = torch.frexp(t)
    return torch.ldexp(torch.round(mant * 8192.0) / 8192.0, expo)


def _onehot_filter(Co, Ci, seed):
    """one tap 2^k per output channel: (ci, ky, kx) and k vary with the channel"""
    w = torch.zeros(Co, Ci, 3, 3)
    for co in range(Co):
        w[co, (5 * co + seed) % Ci, (co // 3) % 3, co % 3] = 2.0 ** ((co % 7) - 3)
    return w


# ---- forward and data gradient: sc_conv3x3_bx3 and sc_conv3x3_thin16
def _pack(lib, op, w, co_t, tflip, terms):
    if op == OP_CONV3:
        return hip_ops.pack_bx3(dev(w), co_t, tflip, TERMS_F16X2 if terms == 4 else terms)
    co, ci = w.shape[:2]
    out = torch.empty(lib.sc_packed_weight_floats_thin16(co, ci, tflip), device=DEV)
    check(lib.sc_pack_weights_thin16(ptr(dev(w)), ptr(out), co, ci, tflip, stream()))
    return out


def run_conv(lib, op, case):
    code, N, (C0, C1), Cout, H, W, srcs, flag_s = case
    fl = set(flag_s.split())
    name = f"{op} {case_id(case)}"
    m, co_t = terms_of(op, code), co_t_of(op, code)
    up, mode, two = parse_src(srcs)
    bnb = _MODE[mode] == SRC_BNBWD
    probe = "fprobe" in fl or "aprobe" in fl
    K = C0 + C1
    gs = _gscale(fl)
    Hs, Ws = (H // 2, W // 2) if up else (H, W)
    tw = tile_w(op, code)
    # operands
    v0 = v1 = None
    if "fprobe" in fl:      # one impulse per input channel, over both sources
        assert not (up and two)
        imp = _impulses(N, K, Hs, Ws, tw // 2 if up else tw, 4 if up else 8)
        if m == 3:      # odd channels: a second term in BOTH operands (see the filter below)
            imp[:, 1::2] *= 1.0 + 2.0 ** -10
        v0, v1 = imp[:, :C0].contiguous(), imp[:, C0:].contiguous()
    s0 = make_operand(mode, N, C0, Hs, Ws, seed=1, gscale=gs, values=v0)
    vals = [up2(s0["val"]) if up else s0["val"]]
    if two:
        s1 = make_operand("raw", N, C1, H, W, seed=20, values=v1)
        vals.append(s1["val"])
    xin = torch.cat(vals, 1).double()
    wshape = (K, Cout, 3, 3) if bnb else (Cout, K, 3, 3)
    w = _onehot_filter(Cout, K, 1).transpose(0, 1).contiguous() if ("aprobe" in fl and bnb) else \
        (_onehot_filter(Cout, K, 1) if "aprobe" in fl else rnd(*wshape, seed=2, scale=0.2))
    assert tuple(w.shape) == wshape
    if "fprobe" in fl and m == 3:
        # The impulses of the odd input channels are 1 + 2^-10 (bf16 terms 1 and 2^-10) and their filter values are cut to 13
        # significant bits (two terms): the product has 24 bits, so it is still exact -- and it needs a1 b1, the first product of
        # the chain, which a unit impulse never exercises.  The even channels keep all 24 bits of the filter (a2 b0).
        if bnb:
            w[1::2] = _cut13(w[1::2])
        else:
            w[:, 1::2] = _cut13(w[:, 1::2])
    conv = (lambda x_, w_: F.conv_transpose2d(x_, w_, padding=1)) if bnb else (lambda x_, w_: F.conv2d(x_, w_, padding=1))
    ref = conv(xin, w.double())
    S = conv(xin.abs(), w.double().abs())
    # the launch
    a = conv_args(op, N, (C0, C1), Cout, H, W, srcs, fl, co_t, m)
    assert query(op, a) == code, (query(op, a), code)
    a.src[0] = to_src(s0, C0, up=int(up))
    if two:
        a.src[1] = to_src(s1, C1)
    wpk = _pack(lib, op, w, co_t, 1 if bnb else 0, m)
    a.wpk = wpk.data_ptr()
    cs = a.csplit
    down0 = "down0" in fl
    prev = rnd(N, cs, H // 2 if down0 else H, W // 2 if down0 else W, seed=30) * gs if a.accum0 else None
    add0 = rnd(N, Cout, H, W, seed=31) * gs if "add" in fl else None
    out0 = dev(prev).clone() if prev is not None else torch.full((N, cs, H // 2 if down0 else H, W // 2 if down0 else W), float("nan"), device=DEV)
    out1 = torch.full((N, Cout - cs, H, W), float("nan"), device=DEV) if cs < Cout else None
    a.out0, a.out1 = out0.data_ptr(), out1.data_ptr() if out1 is not None else None
    a.add0 = dev(add0).data_ptr() if add0 is not None else None
    rows = lib.sc_stat_rows(STAT_CONV3, N, H, W)
    stats = torch.full((rows, Cout, 2), float("nan"), device=DEV) if "stats" in fl else None
    a.stats = stats.data_ptr() if stats is not None else None
    amax = None
    if m == 4 and bnb and not probe:
        amax = torch.tensor([s0["amax"]], device=DEV)
        a.absmax = amax.data_ptr()
    if "bnr" in fl:
        y_in = rnd(N, cs, H, W, seed=40)
        cst_in = torch.zeros(cs, SC_CST)
        cst_in[:, 0], cst_in[:, 1] = rnd(cs, seed=41) * 0.3 + 1, rnd(cs, seed=42) * 0.3
        cst_in[:, 2], cst_in[:, 3] = rnd(cs, seed=43) * 0.2, rnd(cs, seed=44).abs() + 0.5
        y_in = _off_threshold(y_in, cst_in[:, 0], cst_in[:, 1], False)
        a.bnr = C.addressof(hip_ops.make_bnr((dev(y_in), dev(cst_in), ACT_RELU), rows, cs))
    fn = lib.sc_conv3x3_bx3 if op == OP_CONV3 else lib.sc_conv3x3_thin16
    check(fn(C.byref(a), stream()))
    torch.cuda.synchronize()
    # (a) / (c): the element-wise bound
    Kpad = -(-K // 16) * 16
    if probe:
        bound = D_PROBE[m] * S
        if m == 4:
            bound = bound + (S > 0) * (FLOOR_W if "fprobe" in fl else (FLOOR_GRAD1 if bnb else FLOOR_ACT) * 8.0)      # (8: the largest one-hot tap)
        if up or down0:
            bound = bound + 3 * U * S
    else:
        bound = (D_SPLIT[m] + (9 * Kpad * PRODUCTS[m] + 8) * U) * S
        if m == 4:
            fa = floor_grad(s0["amax"]) if bnb else FLOOR_ACT
            bound = bound + conv(torch.full_like(xin, fa), w.double().abs()) + conv(xin.abs(), torch.full_like(w.double(), FLOOR_W))
    full_ref, full_bound = ref, bound
    if add0 is not None:
        full_ref = full_ref + add0.double()
        full_bound = full_bound + U * (add0.double().abs() + ref.abs())
    r0, b0 = full_ref[:, :cs], full_bound[:, :cs]
    if down0:
        pool = lambda t: F.avg_pool2d(t, 2) * 4
        b0 = pool(b0) + 3 * U * pool(r0.abs() + b0)
        r0 = pool(r0)
    if prev is not None:
        b0 = b0 + U * (prev.double().abs() + r0.abs() + b0)
        r0 = r0 + prev.double()
    within(name + " out0", out0, r0, b0)
    if out1 is not None:
        within(name + " out1", out1, full_ref[:, cs:], full_bound[:, cs:])
    if probe:
        return
    dims = (0, 2, 3)
    if stats is not None:
        n = 32 * 4 + 8
        st = stats.double().sum(0).cpu()
        within(name + " sum", st[:, 0], ref.sum(dims), n * U * (ref.abs() + bound).sum(dims) + bound.sum(dims))
        within(name + " sumsq", st[:, 1], (ref ** 2).sum(dims), n * U * ((ref.abs() + bound) ** 2).sum(dims) + (2 * ref.abs() * bound + bound ** 2).sum(dims))
    if "bnr" in fl:
        brows, bmax = hip_ops.LAST_BNR
        sc, sh, mu, isd = (_bc(cst_in[:, k].double()) for k in range(4))
        live = (y_in.double() * sc + sh) > 0
        xhat = (y_in.double() - mu) * isd
        gp, gb = torch.where(live, r0, torch.zeros_like(r0)), torch.where(live, b0, torch.zeros_like(b0))
        n = 32 * 4 + 8
        got = brows.double().sum(0).cpu()
        within(name + " bnr sum", got[:, 0], gp.sum(dims), n * U * (gp.abs() + gb).sum(dims) + gb.sum(dims))
        within(name + " bnr sumxhat", got[:, 1], (gp * xhat).sum(dims), (n + 3) * U * ((gp.abs() + gb) * xhat.abs()).sum(dims) + (gb * xhat.abs()).sum(dims))
        want_mx = float((gp * sc).abs().max())
        slack = float((gb * sc.abs()).max()) + 2 * U * want_mx
        print(f"C3RATIO {name} bnr absmax {abs(float(bmax) - want_mx) / slack:.4f}")
        assert abs(float(bmax) - want_mx) <= slack
    # (b): the aggregate gates
    outs = [(out0, r0)] + ([(out1, full_ref[:, cs:])] if out1 is not None else [])
    errs = [relerr(o, r) for o, r in outs]
    print(f"C3GATE {name} relerr {max(errs):.3e}")
    if m >= 3:
        assert max(errs) < BX3_TOL
    elif m == 2:
        assert max(errs) < 2e-5
    else:
        rb = lambda t: t.float().bfloat16().double()
        ref_r = conv(rb(xin), rb(w))
        if fl <= {"ragged", "stats", "wide"}:
            assert relerr(out0, ref_r) < 5e-6
        assert max(errs) < 2e-2
    if op == OP_CONV3 and m >= 3 and fl <= {"ragged", "stats", "wide"} and C0 % 8 == 0 and C1 % 8 == 0:
        a32 = conv_args(op, N, (C0, C1), Cout, H, W, srcs, fl - {"stats"}, co_t, 0)
        a32.src[0] = a.src[0]
        if two:
            a32.src[1] = a.src[1]
        w32 = hip_ops.pack(dev(w), co_t, 1 if bnb else 0)
        o32 = torch.full((N, Cout, H, W), float("nan"), device=DEV)
        a32.wpk, a32.out0 = w32.data_ptr(), o32.data_ptr()
        check(lib.sc_conv2d_mfma(C.byref(a32), stream()))
        e32 = relerr(o32, ref)
        print(f"C3GATE {name} fp32 kernel relerr {e32:.3e}")
        assert errs[0] < 3 * e32 + 1e-7, (errs[0], e32)


# ---- weight gradients: sc_conv3x3_wgrad_bx3 and sc_conv3x3_wgrad_thin16
def run_wgrad(lib, op, case):
    code, N, (C0, C1), Cout, H, W, (dym, xs), flag_s = case
    fl = set(flag_s.split())
    name = f"{op} {case_id(case)}"
    m = terms_of(op, code)
    up, mode, two = parse_src(xs)
    Cin = C0 + C1
    gs = _gscale(fl)
    probe = "wprobe" in fl or "xprobe" in fl
    Hs, Ws = (H // 2, W // 2) if up else (H, W)
    dyv = _impulses(N, Cout, H, W, 32) if "wprobe" in fl else None
    xv = _impulses(N, C0, Hs, Ws, 32) if "xprobe" in fl else None
    if probe and m == 3:
        # image 0 (the channels c with c % N == 0 have their impulse there): impulses of 1 + 2^-10 against values cut to 13 bits -- a
        # 24-bit product, still exact, that needs a1 b1; the other images keep unit impulses against all 24 bits
        assert not up and not two
        imp, other = (dyv, rnd(N, C0, H, W, seed=10)) if "wprobe" in fl else (xv, rnd(N, Cout, H, W, seed=1))
        imp[0] *= 1.0 + 2.0 ** -10
        other[0] = _cut13(other[0])
        dyv, xv = (imp, other) if "wprobe" in fl else (other, imp)
    d = make_operand(dym, N, Cout, H, W, seed=1, gscale=gs, values=dyv)
    s0 = make_operand(mode, N, C0, Hs, Ws, seed=10, values=xv)
    vals = [up2(s0["val"]) if up else s0["val"]]
    if two:
        s1 = make_operand("raw", N, C1, H, W, seed=20)
        vals.append(s1["val"])
    xin = torch.cat(vals, 1).double()

    def grad(x_, dy_):
        w_ = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(x_, w_, padding=1).backward(dy_)
        return w_.grad
    ref, S = grad(xin, d["val"].double()), grad(xin.abs(), d["val"].double().abs())
    a = wgrad_args(N, (C0, C1), Cout, H, W, (dym, xs), fl, m)
    assert query(op, a) == code, (query(op, a), code)
    a.dy = to_src(d, Cout, offset="offset" in fl)
    a.src[0] = to_src(s0, C0, up=int(up))
    if two:
        a.src[1] = to_src(s1, C1)
    nws = (lib.sc_wgrad_bx3_workspace_floats if op == OP_WGRAD3 else lib.sc_wgrad_thin16_workspace_floats)(N, H, W, Cout, Cin)
    ws = torch.empty(nws, device=DEV)
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
    a.part, a.part_floats, a.dw = ws.data_ptr(), nws, dw.data_ptr()
    amax = None
    if m == 4 and not probe:
        amax = torch.tensor([d["amax"]], device=DEV)
        a.absmax = amax.data_ptr()
    fn = lib.sc_conv3x3_wgrad_bx3 if op == OP_WGRAD3 else lib.sc_conv3x3_wgrad_thin16
    check(fn(C.byref(a), stream()))
    torch.cuda.synchronize()
    if probe:
        bound = D_PROBE[m] * S
        if m == 4:
            bound = bound + (S > 0) * (FLOOR_GRAD1 if "xprobe" in fl else FLOOR_ACT)
        if up:
            bound = bound + 3 * U * S
        within(name + " dw", dw, ref, bound)
        return
    bound = (D_SPLIT[m] + (N * H * W * (PRODUCTS[m] + 1) + 8) * U) * S
    if m == 4:
        bound = bound + grad(xin.abs(), torch.full_like(d["val"], floor_grad(d["amax"])).double()) + grad(torch.full_like(xin, FLOOR_ACT), d["val"].double().abs())
    within(name + " dw", dw, ref, bound)
    e = relerr(dw, ref)
    print(f"C3GATE {name} relerr {e:.3e}")
    if op == OP_WTHIN:
        assert e < 2e-5      # (the gate of test_wgrad_thin16_split)
        return
    if m >= 3:
        assert e < BX3_TOL
    elif m == 2:
        assert e < 2e-5
    else:
        rb = lambda t: t.float().bfloat16().double()
        assert relerr(dw, grad(rb(xin), rb(d["val"]))) < 5e-6 and e < 2e-2
    if m >= 3 and "offset" not in fl and C0 % 8 == 0 and C1 % 8 == 0 and Cout % 8 == 0:
        a32 = wgrad_args(N, (C0, C1), Cout, H, W, (dym, xs), fl, 0)
        a32.dy, a32.src[0] = a.dy, a.src[0]
        if two:
            a32.src[1] = a.src[1]
        n32 = lib.sc_wgrad_workspace_floats(N, H, W, Cout, Cin, 3)
        ws32 = torch.empty(n32, device=DEV)
        dw32 = torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
        a32.part, a32.part_floats, a32.dw = ws32.data_ptr(), n32, dw32.data_ptr()
        check(lib.sc_conv2d_wgrad_mfma(C.byref(a32), stream()))
        e32 = relerr(dw32, ref)
        print(f"C3GATE {name} fp32 kernel relerr {e32:.3e}")
        assert e < 3 * e32 + 2e-7, (e, e32)


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """a failed assertion is one finding; a device error would fail every later case too: end the session there"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, nothing more is launched: {e}", returncode=3)


@pytest.mark.parametrize("case", CONV3_CASES, ids=case_id)
def test_conv3_variant(hip, case):
    run_conv(hip, OP_CONV3, case)


@pytest.mark.parametrize("case", THIN_CASES, ids=case_id)
def test_thin16_variant(hip, case):
    run_conv(hip, OP_THIN, case)


@pytest.mark.parametrize("case", WGRAD3_CASES, ids=case_id)
def test_wgrad3_variant(hip, case):
    run_wgrad(hip, OP_WGRAD3, case)


@pytest.mark.parametrize("case", WTHIN_CASES, ids=case_id)
def test_wgrad_thin16_variant(hip, case):
    run_wgrad(hip, OP_WTHIN, case)
