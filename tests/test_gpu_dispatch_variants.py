"""Every kernel variant the pointwise dispatchers can reach, at kernel tolerance.

sc_conv1x1_pw3, sc_conv1x1_wgrad_pw3, sc_irb_eval and the streaming kernel inside sc_conv2d_mfma pick a template instantiation from
the shape.  The per-op tests next door (test_gpu_ops.py, test_gpu_irb.py) use the network's small test shapes, which select a few of
those instantiations; the rest -- among them what the batch-16 / batch-64 step runs -- only ran inside whole-network tests with gates
of 1e-4 and looser.  Here every variant code the host queries (sc_conv1x1_pw3_variant, sc_wgrad_pw3_variant, sc_irb_variant,
sc_pw_stream_variant -- the dispatchers call them themselves) can return has a plain case and a ragged one; every case asserts the
code it was written for before it launches.  tests/test_dispatch_variants_host.py holds the tables below to the full set of codes on a
box without a GPU, which is why the tables and the *_code helpers sit at module level and touch no device.

References, helpers and bounds are the neighbours': float64 conv2d / conv_transpose2d / the same op sequence, `_run` of
test_gpu_irb.py, hip_ops; 2e-6 (forward) and 1e-5 (gradients: dy is formed in fp32) for the split-bf16 pointwise kernels -- the bounds
of the PW3 tests of test_gpu_ops.py, both inside its TOL --, TOL for the streaming kernel, 3e-6 for sc_irb_eval, 1e-5 for a statistics
row against the sums of the launch's own output."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import test_gpu_irb  # noqa: E402
import test_gpu_ops  # noqa: E402
from hip_ops import DEV, dev, relerr  # noqa: E402
from starcop_amd import _lib  # noqa: E402
from starcop_amd._lib import (ACT_NONE, ACT_RELU, ACT_RELU6, SC_CST, SRC_AFFINE, SRC_BNBWD, SRC_RAW, make_src, sc_conv_args)  # noqa: E402
from test_gpu_ops import TOL, act_ref, rnd  # noqa: E402

assert TOL == 1e-4
PW3_FWD_TOL, PW3_BWD_TOL, IRB_TOL, STATS_TOL = 2e-6, 1e-5, 3e-6, 1e-5


# ---- sc_conv1x1_pw3: (ncb, K, M, N, H, W).  Forward: the layer K -> M.  Data gradient: of the layer M -> K (the launch writes M channels
# from a BNBWD source of K channels).  npb = ceil(N H W / 32), MB = ceil(M / 32); ncb = 4 needs MB >= 3 and npb * ceil(MB / 4) >= 1536,
# ncb = 2 needs MB >= 2 and npb * ceil(MB / 2) >= 1536.
PW3_VARIANT_CASES = [
    (4, 64, 384, 1, 128, 128),     # npb 512, MB 12: 512 * 3 = 1536, exactly the threshold
    (2, 64, 384, 1, 128, 127),     # npb 508: 1524 < 1536, then 508 * 6
    (4, 16, 96, 3, 128, 128),      # MB 3 in a group of 4: one padding block
    (4, 24, 136, 3, 91, 90),       # npb 768, N H W % 32 = 26, H W % 4 = 2 (scalar stores), MB 5: the second group has one valid block; K 24 -> 32
    (2, 16, 40, 3, 128, 128),      # MB 2, M % 64 != 0
    (2, 32, 160, 1, 128, 128),     # npb 512: 512 * 2 fails for 4, 512 * 3 passes for 2; MB 5: the last group has one valid block
    (2, 24, 40, 3, 127, 129),      # npb 1536 (49149 pixels: % 32 = 29), H W % 4 = 3, K 24 -> 32
    (1, 32, 64, 2, 16, 16),
    (1, 24, 40, 1, 10, 13),        # N H W = 130, H W % 4 = 2
]

# ---- sc_conv1x1_wgrad_pw3: (10 tm + tn, layer Cin, layer Cout, N, H, W); H W % 8 == 0.  11 = k_pw3_wgrad<1, 1, 4> (both <= 32 channels)
PW3_WGRAD_VARIANT_CASES = [
    (11, 32, 16, 2, 8, 12),
    (11, 24, 24, 1, 4, 6),         # 24 pixels: one whole and one half K step
    (12, 40, 24, 1, 4, 6),
    (21, 24, 40, 2, 8, 12),
    (22, 40, 72, 1, 4, 6),
]

# ---- sc_irb_eval: (code, N, Cin, hidden, Cout, H, W, residual, source[, stride]); code = 10000 tiling (0 A, 1 B, 3 stride-2 A)
# + 1000 pairs per wave + 10 NKE + work-groups per CU.  Tiling A: hidden % 64 == 0, pairs = ceil(ceil(Cout / 32) / 4), two work-groups
# per CU while Cin <= 96 and Cout <= 128; B: hidden % 64 != 0, pairs = ceil(ceil(Cout / 32) / 2); NKE = ceil(Cin / 16) rounded up to
# 2, 4, 6, 10.  Channel counts off the multiples of 16 / 32 and the 13 x 11 planes (H, W off the tile, W % 4 != 0) are the edges.
IRB_VARIANT_CASES = [
    (1022, 2, 32, 128, 32, 16, 16, True, "raw"),
    (1022, 1, 24, 64, 24, 13, 11, True, "affine"),
    (1042, 1, 40, 128, 72, 8, 16, False, "affine"),
    (1062, 1, 96, 192, 128, 8, 8, False, "raw"),
    (1101, 1, 128, 128, 96, 8, 8, False, "raw"),
    (1101, 1, 104, 128, 104, 13, 11, True, "affine"),      # Cin % 16 != 0 at NKE 10: 7 of the 10 K steps, the last one half full
    (2021, 1, 32, 128, 160, 8, 8, False, "raw"),
    (2041, 1, 64, 128, 136, 8, 8, False, "affine"),
    (2061, 1, 96, 128, 256, 8, 8, False, "raw"),
    (2101, 1, 152, 128, 152, 8, 8, True, "affine"),
    (3021, 1, 16, 64, 264, 8, 8, False, "raw"),
    (3041, 1, 48, 128, 384, 8, 8, False, "affine"),
    (3061, 1, 96, 128, 320, 8, 8, False, "raw"),
    (3061, 2, 88, 64, 264, 13, 11, False, "affine"),
    (3101, 1, 160, 128, 328, 4, 8, False, "affine"),
    (11021, 1, 32, 96, 32, 16, 16, True, "raw"),
    (11041, 1, 56, 96, 64, 8, 8, False, "affine"),
    (11061, 1, 96, 96, 40, 8, 8, False, "raw"),
    (11101, 1, 160, 96, 24, 8, 8, False, "affine"),
    (12021, 1, 24, 96, 96, 8, 8, False, "raw"),
    (12041, 1, 64, 160, 128, 8, 8, False, "affine"),
    (12061, 1, 88, 96, 88, 8, 8, True, "raw"),
    (12101, 1, 136, 96, 72, 8, 8, False, "raw"),
    (13021, 1, 32, 96, 192, 8, 8, False, "affine"),
    (13041, 1, 64, 96, 136, 8, 8, False, "raw"),
    (13041, 2, 40, 96, 136, 13, 11, False, "raw"),
    (13061, 1, 96, 96, 160, 8, 8, False, "affine"),
    (13101, 1, 144, 96, 144, 8, 8, True, "affine"),
    (31021, 1, 32, 128, 64, 16, 16, False, "raw", 2),
    (31041, 1, 56, 128, 128, 16, 16, False, "affine", 2),
    (31061, 1, 96, 128, 96, 13, 11, False, "raw", 2),
    (32021, 1, 24, 64, 136, 16, 16, False, "raw", 2),
    (32041, 1, 64, 128, 256, 16, 16, False, "affine", 2),
    (32061, 1, 80, 128, 160, 9, 13, False, "raw", 2),
]

# the residual sum of a block whose AFFINE input carries an activation: (code, N, C, hidden, H, W, act).  W % 4 == 0 takes the 16-byte
# store path of the epilogue, W % 4 != 0 the scalar one; one case on tiling B.
IRB_RESIDUAL_ACT_CASES = [
    (1022, 1, 32, 128, 16, 16, ACT_RELU6),
    (1022, 1, 32, 128, 13, 11, ACT_RELU6),
    (1022, 2, 24, 64, 8, 12, ACT_RELU),
    (11041, 1, 64, 96, 8, 10, ACT_RELU),
]

# ---- the streaming kernel of sc_conv2d_mfma, forward: (code, N, Cin, Cout, H, W, source); code = 10 NCB + NKS, NKS = Cin / 4;
# NCB 1: Cout <= 16, 2: <= 32, 5: <= 160, 6: <= 192.  Cout = 8 / 40 / 168: most of the wave's 16-channel output blocks are padding.
PWS_VARIANT_CASES = [
    (16, 1, 24, 16, 64, 64, "affine6"), (16, 1, 24, 8, 64, 64, "raw"), (18, 1, 32, 16, 64, 64, "raw"), (18, 2, 32, 8, 64, 64, "affine6"),
    (26, 1, 24, 24, 64, 64, "affine"), (28, 1, 32, 32, 64, 64, "affine6"),
    (56, 1, 24, 144, 64, 64, "raw"), (56, 1, 24, 40, 64, 64, "affine6"), (58, 1, 32, 160, 64, 64, "affine"), (58, 1, 32, 40, 64, 64, "raw"),
    (66, 1, 24, 176, 64, 64, "affine"), (66, 1, 24, 168, 64, 64, "affine6"), (68, 1, 32, 192, 64, 64, "raw"), (68, 1, 32, 168, 64, 64, "affine"),
]
# ... and with a BatchNorm-backward source: (code, N, layer Cin = M, layer Cout = K, H, W, act); code = 100 + 10 NCB + NKS, NKS = K / 4;
# NCB 2: M <= 32, 3: <= 96, 5: <= 160, 6: <= 192.  M = 33: two of the three blocks of NCB 3 are padding but for one channel.
PWS_DGRAD_VARIANT_CASES = [
    (124, 1, 32, 16, 64, 64, ACT_NONE), (126, 1, 24, 24, 64, 64, ACT_RELU6), (128, 1, 32, 32, 64, 64, ACT_RELU), (128, 1, 8, 32, 64, 64, ACT_NONE),
    (134, 1, 33, 16, 64, 64, ACT_RELU6), (134, 1, 96, 16, 64, 64, ACT_NONE), (136, 1, 96, 24, 64, 64, ACT_RELU), (138, 1, 88, 32, 64, 64, ACT_NONE),
    (138, 1, 33, 32, 64, 64, ACT_RELU6),
    (154, 1, 104, 16, 64, 64, ACT_RELU), (156, 1, 144, 24, 64, 64, ACT_NONE), (158, 1, 160, 32, 64, 64, ACT_RELU6), (158, 1, 100, 32, 64, 64, ACT_NONE),
    (164, 1, 168, 16, 64, 64, ACT_NONE), (164, 1, 161, 16, 64, 64, ACT_RELU6), (166, 1, 184, 24, 64, 64, ACT_RELU6), (168, 1, 192, 32, 64, 64, ACT_RELU),
]


# ---- host side: the variant code of a table entry (no device)
def pw3_code(N, H, W, M):
    return _lib.load().sc_conv1x1_pw3_variant(N, H, W, M)


def pw3_wgrad_code(N, H, W, cout, cin):
    return _lib.load().sc_wgrad_pw3_variant(N, H, W, cout, cin)


def irb_code(cin, hidden, cout, stride=1):
    return _lib.load().sc_irb_variant(cin, hidden, cout, stride)


def pws_code(N, K, M, H, W, bnb, stats=False, base=1 << 20):
    """sc_pw_stream_variant for the launch the streaming tests make: one K-channel source (16-byte aligned at `base`), M outputs, the
    co_t they pack with; the pointers are never dereferenced"""
    a = sc_conv_args()
    a.nsrc = 1
    a.src[0] = sc_src_stub(base, K, SRC_BNBWD if bnb else SRC_AFFINE)
    a.wpk, a.out0, a.csplit = 1 << 22, 1 << 23, M
    a.N, a.H, a.W, a.Cout, a.ks, a.co_t = N, H, W, M, 1, (32 if M <= 32 else 64)
    a.stats = (1 << 24) if stats else None
    return _lib.load().sc_pw_stream_variant(C.byref(a))


def sc_src_stub(base, K, mode):
    s = _lib.sc_src()
    s.x, s.aux, s.cst = base, (base + (1 << 19) if mode == SRC_BNBWD else None), 1 << 21
    s.C, s.mode, s.act, s.up = K, mode, ACT_NONE, 0
    return s


def _ids(case):
    return "x".join(str(v) for v in case)


# ---- sc_conv1x1_pw3
@pytest.mark.parametrize("case", PW3_VARIANT_CASES, ids=_ids)
def test_pw3_forward_every_variant(hip, case):
    """forward through ReLU6(affine) with statistics rows, then the same launch with add0 and accumulation into an existing tensor"""
    from hip_ops import conv_pw3, pack_pw3
    ncb, K, M, N, H, W = case
    assert hip.sc_conv1x1_pw3_variant(N, H, W, M) == ncb
    x, w = rnd(N, K, H, W, seed=1, scale=3.0), rnd(M, K, 1, 1, seed=2, scale=0.3)
    cst = torch.rand(K, SC_CST, generator=torch.Generator().manual_seed(3)) + 0.5
    xin = act_ref(x.double() * cst[:, 0].double()[None, :, None, None] + cst[:, 1].double()[None, :, None, None], ACT_RELU6)
    ref = F.conv2d(xin, w.double())
    src = make_src(dev(x), K, SRC_AFFINE, act=ACT_RELU6, cst=dev(cst))
    wpk = pack_pw3(dev(w), 0)
    out, st = conv_pw3(src, wpk, N, H, W, M, want_stats=True)
    own = out.double()
    e = (relerr(out, ref), relerr(st.double().sum(0)[:, 0], own.sum((0, 2, 3))), relerr(st.double().sum(0)[:, 1], (own * own).sum((0, 2, 3))))
    res, old = rnd(N, M, H, W, seed=9), rnd(N, M, H, W, seed=10)
    out2, _ = conv_pw3(src, wpk, N, H, W, M, add0=dev(res), accum_into=dev(old.clone()))
    e2 = relerr(out2, ref + res.double() + old.double())
    print(f"pw3 forward {_ids(case)}: out {e[0]:.2e} stats {e[1]:.2e} {e[2]:.2e} add0+accum {e2:.2e}")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(st).all())
    assert e[0] < PW3_FWD_TOL and e[1] < STATS_TOL and e[2] < STATS_TOL and e2 < PW3_FWD_TOL, (e, e2)


@pytest.mark.parametrize("case", PW3_VARIANT_CASES, ids=_ids)
def test_pw3_data_gradient_every_variant(hip, case):
    """the data gradient of the layer M -> K: BNBWD source, the plain launch, add0 + accumulation, and sc_bnr_args (the gradient
    bit-identical, the rows against float64 sums of the launch's own output: the check of
    test_conv_pw3_dgrad_leaves_batchnorm_backward_sums)"""
    import hip_ops
    from hip_ops import conv_pw3, pack_pw3
    ncb, K, M, N, H, W = case
    assert hip.sc_conv1x1_pw3_variant(N, H, W, M) == ncb
    w = rnd(K, M, 1, 1, seed=2, scale=0.3)
    g, y = rnd(N, K, H, W, seed=3) * 1e-3, rnd(N, K, H, W, seed=4)
    a, b = rnd(K, seed=4) * 0.2 + 1, rnd(K, seed=5) * 0.2
    A, B, D = rnd(K, seed=6) * 0.3 + 1, rnd(K, seed=7) * 1e-4, rnd(K, seed=8) * 1e-4
    yh = y * a[None, :, None, None] + b[None, :, None, None]
    gm = torch.where((yh > 0) & (yh < 6), g, torch.zeros(()))
    dy = gm.double() * A.double()[None, :, None, None] + B.double()[None, :, None, None] * y.double() + D.double()[None, :, None, None]
    cstb = torch.zeros(K, SC_CST); cstb[:, 0], cstb[:, 1], cstb[:, 2], cstb[:, 3], cstb[:, 4] = a, b, A, B, D
    dsrc = make_src(dev(g), K, SRC_BNBWD, act=ACT_RELU6, cst=dev(cstb), aux=dev(y))
    ref = F.conv_transpose2d(dy, w.double())
    wpk = pack_pw3(dev(w), 1)
    dx, _ = conv_pw3(dsrc, wpk, N, H, W, M)
    res, old = rnd(N, M, H, W, seed=9) * 1e-3, rnd(N, M, H, W, seed=10) * 1e-3
    dx2, _ = conv_pw3(dsrc, wpk, N, H, W, M, add0=dev(res), accum_into=dev(old.clone()))
    y_in = rnd(N, M, H, W, seed=11) * 2
    cst_in = torch.zeros(M, SC_CST)
    cst_in[:, 0], cst_in[:, 1], cst_in[:, 2], cst_in[:, 3] = rnd(M, seed=12) * 0.2 + 1, rnd(M, seed=13) * 0.5 + 1.5, rnd(M, seed=14) * 0.1, rnd(M, seed=15).abs() * 0.2 + 0.8
    dx1, _ = conv_pw3(dsrc, wpk, N, H, W, M, bnr=(dev(y_in), dev(cst_in), ACT_RELU6))
    rows, _ = hip_ops.LAST_BNR
    sc, sh, mu, isd = (cst_in[:, k].double()[None, :, None, None] for k in range(4))
    yhi = y_in.double() * sc + sh
    gp = torch.where((yhi > 0) & (yhi < 6), dx1.double().cpu(), torch.zeros((), dtype=torch.float64))
    s1, s2 = gp.sum((0, 2, 3)), (gp * (y_in.double() - mu) * isd).sum((0, 2, 3))
    got = rows.double().sum(0).cpu()
    scale = max(float(s1.abs().max()), float(s2.abs().max()), 1e-6)
    e = (relerr(dx, ref), relerr(dx2, ref + res.double() + old.double()), float((got[:, 0] - s1).abs().max()) / scale, float((got[:, 1] - s2).abs().max()) / scale)
    print(f"pw3 data gradient {_ids(case)}: dx {e[0]:.2e} add0+accum {e[1]:.2e} bnr rows {e[2]:.2e} {e[3]:.2e}")
    assert e[0] < PW3_BWD_TOL and e[1] < PW3_BWD_TOL, e
    assert torch.equal(dx, dx1) and bool(torch.isfinite(rows).all())
    assert e[2] < 2e-5 and e[3] < 2e-5, e


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("case", PW3_WGRAD_VARIANT_CASES, ids=_ids)
def test_pw3_weight_gradient_every_variant(hip, case, deferred):
    code, cin, cout, N, H, W = case
    assert hip.sc_wgrad_pw3_variant(N, H, W, cout, cin) == code
    test_gpu_ops.test_conv_pw3_wgrad(hip, cin, cout, N, H, W, deferred)      # float64 autograd reference, 1e-5


# ---- sc_irb_eval
@pytest.mark.parametrize("case", IRB_VARIANT_CASES, ids=_ids)
def test_irb_every_variant(hip, case):
    code, shape = case[0], case[1:]
    stride = shape[8] if len(shape) > 8 else 1
    assert hip.sc_irb_variant(shape[1], shape[2], shape[3], stride) == code
    out, want, zmax = test_gpu_irb._run(shape, seed=300 + IRB_VARIANT_CASES.index(case))
    e = relerr(out, want)
    print(f"irb {_ids(case)}: {e:.2e}")
    assert bool(torch.isfinite(out).all())
    assert e < IRB_TOL, e
    if shape[6]:
        assert abs(float(zmax) - float(out.abs().max())) <= 1e-6 * float(out.abs().max())


@pytest.mark.parametrize("case", IRB_RESIDUAL_ACT_CASES, ids=_ids)
def test_irb_residual_adds_the_activated_input(hip, case):
    """z = act(scale x + shift) + BN_p(p): the residual term is the block input as the expansion saw it.  The input spreads over about
    +-16, so a residual term that skips the clamp is wrong by up to the whole excess over [0, 6]"""
    code, N, C_, hid, H, W, act = case
    assert hip.sc_irb_variant(C_, hid, C_, 1) == code
    shape = (N, C_, hid, C_, H, W, True, "affine")
    out, want, zmax = test_gpu_irb._run(shape, seed=400 + IRB_RESIDUAL_ACT_CASES.index(case), act=act, xscale=4.0)
    e = relerr(out, want)
    print(f"irb residual act {_ids(case)}: {e:.2e}, max |z| {float(zmax):.6f} vs {float(out.abs().max()):.6f} (reference {float(want.abs().max()):.6f})")
    assert bool(torch.isfinite(out).all())
    assert e < IRB_TOL, e
    assert abs(float(zmax) - float(out.abs().max())) <= 1e-6 * float(out.abs().max())
    assert abs(float(zmax) - float(want.abs().max())) <= IRB_TOL * float(want.abs().max())


# ---- the streaming kernel of sc_conv2d_mfma (bodies: test_gpu_ops.py -- float64 reference at TOL, statistics rows against the sums
# of the launch's own output at 1e-5, and the LDS-staged kernel through a source offset by one float)
@pytest.mark.parametrize("case", PWS_VARIANT_CASES, ids=_ids)
def test_pointwise_streaming_forward_every_variant(hip, case):
    code, N, cin, cout, H, W, mode = case
    assert pws_code(N, cin, cout, H, W, False, stats=True) == code and pws_code(N, cin, cout, H, W, False) == code
    assert pws_code(N, cin, cout, H, W, False, base=(1 << 20) + 4) == -1      # one float off: the LDS-staged kernel
    test_gpu_ops.test_pointwise_streaming_forward(hip, case[1:])


@pytest.mark.parametrize("case", PWS_DGRAD_VARIANT_CASES, ids=_ids)
def test_pointwise_streaming_dgrad_every_variant(hip, case):
    code, N, cin, cout, H, W, act = case
    assert pws_code(N, cout, cin, H, W, True) == code
    assert pws_code(N, cout, cin, H, W, True, base=(1 << 20) + 4) == -1
    test_gpu_ops.test_pointwise_streaming_dgrad(hip, case[1:])
