"""Multi-class U-Net inference on the GPU: the 9..16-channel stem (sc_stem_conv_fwd), the K-class head with its fused argmax
(sc_head_conv_fwd_k), HyperStarcopUNet(13, 4) / predict_classes and the Sentinel-2 cloud detector (sentinel2.CDModel) against
plain torch CPU ops in float64 and the CPU oracle network.  Tolerance of the operators: the 1e-4 (relative to the largest
reference magnitude) that tests/test_gpu_ops.py applies to the existing stem and head."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hip_ops import DEV, cst_affine, dev, relerr  # noqa: E402
from oracle.unet_ref import UnetMobileNetV2  # noqa: E402
from starcop_amd import sentinel2  # noqa: E402
from starcop_amd._lib import ACT_RELU, SC_CST, SRC_AFFINE, SRC_NORM, SRC_RAW, STAT_STEM, check, make_src, ptr, stream  # noqa: E402
from starcop_amd.network import HyperStarcopUNet  # noqa: E402

TOL = 1e-4
K_MFMA4, K_VALU4, K_VALU8, K_VALU16 = 0, 1, 2, 3        # enum sc_stem_kernel


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------ stem
def _stem_case(Cin, H, W, mode):
    N = 2
    x, w = rnd(N, Cin, H, W, seed=41) * 2.0, rnd(32, Cin, 3, 3, seed=42, scale=0.3)
    if mode == "norm":
        cst = torch.zeros(Cin, SC_CST)
        cst[:, 0], cst[:, 1], cst[:, 2], cst[:, 3] = 0.1, rnd(Cin, seed=43).abs() + 0.5, -1.0, 1.5
        xa = torch.clamp((x.double() - 0.1) / cst[:, 1].double()[None, :, None, None], -1.0, 1.5)
        src = make_src(dev(x), Cin, SRC_NORM, cst=dev(cst))
    else:
        xa = x.double()
        src = make_src(dev(x), Cin, SRC_RAW)
    ref = F.conv2d(xa, w.double(), stride=2, padding=1)
    return N, src, dev(w), ref


@pytest.mark.parametrize("case", [(Cin, H, W, "raw") for Cin in (9, 13, 16) for H, W in ((38, 70), (64, 96))] + [(13, 38, 70, "norm")],
                         ids=lambda c: "x".join(map(str, c)))
def test_wide_stem(hip, case):
    """9 <= Cin <= 16: the two-chunk kernel, ragged (19 x 35 outputs, more than one tile) and whole tiles, through an aligned and an
    unaligned output; statistics rows are refused above 8 channels"""
    Cin, H, W, mode = case
    N, src, wd, ref = _stem_case(Cin, H, W, mode)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert hip.sc_stem_fwd_kernel(Cin, W, 1) == K_VALU16 and hip.sc_stem_fwd_kernel(Cin, W, 0) == K_VALU16
    obuf = torch.zeros(N * 32 * Ho * Wo + 4, device=DEV)
    outs = []
    for off in (0, 1):
        out = obuf[off:off + N * 32 * Ho * Wo].view(N, 32, Ho, Wo)
        out.fill_(float("nan"))
        check(hip.sc_stem_conv_fwd(C.byref(src), ptr(wd), ptr(out), N, Cin, H, W, None, stream()))
        e = relerr(out, ref)
        print(f"wide stem {case}: rel err {e:.3g}")
        assert e < TOL, e
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])
    stats = torch.zeros(hip.sc_stat_rows(STAT_STEM, N, Ho, Wo), 32, 2, device=DEV)
    with pytest.raises(ValueError, match="statistics"):
        check(hip.sc_stem_conv_fwd(C.byref(src), ptr(wd), ptr(outs[0]), N, Cin, H, W, ptr(stats), stream()))
    with pytest.raises(ValueError):
        check(hip.sc_stem_conv_fwd(C.byref(make_src(outs[0], 17, SRC_RAW)), ptr(wd), ptr(outs[0]), N, 17, H, W, None, stream()))


def test_stem_eight_channels_keep_their_kernel(hip):
    """Cin <= 8 keeps its launches: the dispatch rule names the unchanged kernels (k_stem_fwd4m / k_stem_fwd<4> / k_stem_fwd<8>) for
    them and the new one only above 8; the 8-channel result is the float64 convolution at the existing tolerance"""
    for W in (70, 96):
        assert hip.sc_stem_fwd_kernel(8, W, 1) == K_VALU8 and hip.sc_stem_fwd_kernel(5, W, 0) == K_VALU8
        assert hip.sc_stem_fwd_kernel(9, W, 1) == K_VALU16 and hip.sc_stem_fwd_kernel(16, W, 1) == K_VALU16
        assert hip.sc_stem_fwd_kernel(4, W, 0) == K_VALU4 and hip.sc_stem_fwd_kernel(1, W, 0) == K_VALU4
    assert hip.sc_stem_fwd_kernel(4, 96, 1) == K_MFMA4 and hip.sc_stem_fwd_kernel(4, 70, 1) == K_VALU4       # Wout = 48 / 35
    assert hip.sc_stem_fwd_kernel(0, 96, 1) < 0 and hip.sc_stem_fwd_kernel(17, 96, 1) < 0
    for H, W in ((38, 70), (64, 96)):
        N, src, wd, ref = _stem_case(8, H, W, "raw")
        out = torch.full((N, 32, (H - 1) // 2 + 1, (W - 1) // 2 + 1), float("nan"), device=DEV)
        check(hip.sc_stem_conv_fwd(C.byref(src), ptr(wd), ptr(out), N, 8, H, W, None, stream()))
        assert relerr(out, ref) < TOL


# ------------------------------------------------------------------------------------------------ head
def _head_inputs(N, Cin, K, H, W, mode):
    x, w, b = rnd(N, Cin, H, W, seed=11), rnd(K, Cin, 3, 3, seed=12, scale=0.3), rnd(K, seed=13, scale=0.5)
    if mode == "affine":
        sc, sh = rnd(Cin, seed=14) * 0.3 + 1, rnd(Cin, seed=15) * 0.2
        xa = F.relu(x.double() * sc.double()[None, :, None, None] + sh.double()[None, :, None, None])
        src_of = lambda t: make_src(t, Cin, SRC_AFFINE, act=ACT_RELU, cst=cst_affine(sc, sh))     # noqa: E731
    else:
        xa = x.double()
        src_of = lambda t: make_src(t, Cin, SRC_RAW)     # noqa: E731
    return x, w, b, src_of, F.conv2d(xa, w.double(), b.double(), padding=1)


def _run_head(hip, src, wd, bd, N, Cin, K, H, W, want_logits, want_classes, off=0):
    """outputs start as NaN / 255 so that an unwritten element shows; off: element offset of both outputs (unaligned bases)"""
    lbuf = torch.full((N * K * H * W + 4,), float("nan"), device=DEV)
    cbuf = torch.full((N * H * W + 4,), 255, dtype=torch.uint8, device=DEV)
    logits = lbuf[off:off + N * K * H * W].view(N, K, H, W)
    classes = cbuf[off:off + N * H * W].view(N, H, W)
    check(hip.sc_head_conv_fwd_k(C.byref(src), ptr(wd), ptr(bd), ptr(logits) if want_logits else None,
                                 ptr(classes) if want_classes else None, N, Cin, K, H, W, stream()))
    torch.cuda.synchronize()
    if not want_logits:
        assert torch.isnan(lbuf).all()
    if not want_classes:
        assert bool((cbuf == 255).all())
    assert torch.isnan(lbuf[:off]).all() and torch.isnan(lbuf[off + N * K * H * W:]).all()
    assert bool((cbuf[:off] == 255).all()) and bool((cbuf[off + N * H * W:] == 255).all())
    return logits, classes


@pytest.mark.parametrize("mode", ["raw", "affine"])
@pytest.mark.parametrize("plane", [(19, 37), (32, 64)], ids=lambda p: "x".join(map(str, p)))
@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_head_k(hip, K, plane, mode):
    """Cin = 16: logits only, classes only, both; the ragged plane (W % 4 != 0: 4-byte staging and stores, two row tiles) and the
    16-byte path; the same call through unaligned input / output bases"""
    N, Cin = 2, 16
    H, W = plane
    x, w, b, src_of, ref = _head_inputs(N, Cin, K, H, W, mode)
    xd, wd, bd = dev(x), dev(w), dev(b)
    src = src_of(xd)
    both_l, both_c = _run_head(hip, src, wd, bd, N, Cin, K, H, W, True, True)
    e = relerr(both_l, ref)
    print(f"head K={K} {plane} {mode}: rel err {e:.3g}")
    assert e < TOL, e
    assert torch.equal(both_c, torch.argmax(both_l, dim=1).to(torch.uint8))
    only_l, _ = _run_head(hip, src, wd, bd, N, Cin, K, H, W, True, False)
    assert torch.equal(only_l, both_l)
    _, only_c = _run_head(hip, src, wd, bd, N, Cin, K, H, W, False, True)
    assert torch.equal(only_c, both_c)
    if K == 1:
        one = torch.full((N, 1, H, W), float("nan"), device=DEV)
        check(hip.sc_head_conv_fwd(C.byref(src), ptr(wd), ptr(bd), ptr(one), N, Cin, H, W, stream()))
        assert torch.equal(one, both_l) and int(both_c.max()) == 0
    # unaligned bases: the input one float, the outputs one element past an aligned address
    xo = torch.zeros(x.numel() + 4, device=DEV)
    xv = xo[1:1 + x.numel()].view(N, Cin, H, W)
    xv.copy_(xd)
    un_l, un_c = _run_head(hip, src_of(xv), wd, bd, N, Cin, K, H, W, True, True, off=1)
    assert relerr(un_l, ref) < TOL
    assert torch.equal(un_c, torch.argmax(un_l, dim=1).to(torch.uint8))
    if K > 1:
        assert torch.equal(un_l, both_l)        # one stencil, two staging forms: the same FMA sequence


@pytest.mark.parametrize("Cin,K", [(8, 4), (32, 3), (5, 8)])
def test_head_k_other_channel_counts(hip, Cin, K):
    """Cin != 16: the one-pixel-per-thread kernel, ragged 19 x 37 plane (two row tiles, two column tiles)"""
    N, H, W = 2, 19, 37
    x, w, b, src_of, ref = _head_inputs(N, Cin, K, H, W, "affine")
    src, wd, bd = src_of(dev(x)), dev(w), dev(b)
    both_l, both_c = _run_head(hip, src, wd, bd, N, Cin, K, H, W, True, True)
    assert relerr(both_l, ref) < TOL
    assert torch.equal(both_c, torch.argmax(both_l, dim=1).to(torch.uint8))
    _, only_c = _run_head(hip, src, wd, bd, N, Cin, K, H, W, False, True)
    assert torch.equal(only_c, both_c)


@pytest.mark.parametrize("Cin", [16, 8])
@pytest.mark.parametrize("bias,want", [((0.5, 0.5, 0.5, 0.5), 0), ((0.0, 1.0, 1.0, 0.0), 1), ((1.0, float("nan"), 0.0, float("nan")), 1)],
                         ids=["all-equal", "tie", "nan"])
def test_argmax_rules(hip, Cin, bias, want):
    """zero weights: the logits are the bias.  torch.argmax: first maximal index; NaN counts as maximal, the first NaN wins"""
    N, K = 2, 4
    b = torch.tensor(bias)
    assert int(torch.argmax(b)) == want
    for H, W in ((19, 37), (32, 64)):
        src = make_src(dev(rnd(N, Cin, H, W, seed=5)), Cin, SRC_RAW)
        wd, bd = dev(torch.zeros(K, Cin, 3, 3)), dev(b)
        logits, classes = _run_head(hip, src, wd, bd, N, Cin, K, H, W, True, True)
        assert torch.equal(torch.nan_to_num(logits.cpu(), nan=-7.0), torch.nan_to_num(b, nan=-7.0)[None, :, None, None].expand(N, K, H, W))
        assert bool((classes == want).all())
        _, only_c = _run_head(hip, src, wd, bd, N, Cin, K, H, W, False, True)
        assert bool((only_c == want).all())


def test_head_k_argument_checks(hip):
    N, Cin, H, W = 1, 16, 8, 8
    src = make_src(dev(rnd(N, Cin, H, W)), Cin, SRC_RAW)
    wd, bd = dev(torch.zeros(9, Cin, 3, 3)), dev(torch.zeros(9))
    out = torch.zeros(N * 9 * H * W, device=DEV)
    for K in (0, 9):
        with pytest.raises(ValueError, match="K must be"):
            check(hip.sc_head_conv_fwd_k(C.byref(src), ptr(wd), ptr(bd), ptr(out), None, N, Cin, K, H, W, stream()))
    with pytest.raises(ValueError, match="at least one"):
        check(hip.sc_head_conv_fwd_k(C.byref(src), ptr(wd), ptr(bd), None, None, N, Cin, 4, H, W, stream()))


# ------------------------------------------------------------------------------------------------ whole network
NEAR_TIE = 1e-4         # classes are compared where the float64 top-two gap is at least this fraction of max |logit| (the fp32 contract)


@functools.lru_cache(maxsize=None)
def _oracle_case():
    """the 13-band / 4-class oracle with seeded weights and non-trivial BatchNorm statistics, its input and float64 logits; the head
    bias is minus each class's mean logit so that every class wins somewhere (with the zero bias of the initialisation class 2 never
    does on this input).  Computed once, never modified."""
    torch.manual_seed(0)
    ref = UnetMobileNetV2(13, 4).eval()
    g = torch.Generator().manual_seed(1)
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    x = torch.randn(2, 13, 64, 96, generator=torch.Generator().manual_seed(2))
    ref64 = copy.deepcopy(ref).double()
    with torch.no_grad():
        bias = -ref64(x.double()).mean((0, 2, 3)).float()
        ref.segmentation_head[0].bias.copy_(bias)
        ref64.segmentation_head[0].bias.copy_(bias.double())
        logits64 = ref64(x.double())
    return ref.state_dict(), ref64, x, logits64


def _check_classes(got, logits64, what):
    """got: uint8 classes; logits64: (.., K, H, W) float64 with the class axis at -3"""
    top = logits64.topk(2, dim=-3).values
    sure = (top.select(-3, 0) - top.select(-3, 1)) >= NEAR_TIE * float(logits64.abs().max())
    left_out = 1.0 - float(sure.double().mean())
    want = logits64.argmax(-3)
    wrong = int((got.cpu().long() != want)[sure].sum())
    print(f"{what}: {100 * left_out:.3f} % of the pixels are near ties and left out; {wrong} of the others differ")
    assert left_out <= 0.01, left_out
    assert wrong == 0, wrong


def test_network_13_4_against_the_oracle(hip):
    sd, _, x, logits64 = _oracle_case()
    counts = torch.bincount(logits64.argmax(1).flatten(), minlength=4).double()
    assert bool((counts / counts.sum() >= 0.05).all()), counts.tolist()
    net = HyperStarcopUNet(13, 4)
    net.load_state_dict(sd)
    net = net.to(DEV).eval()
    with torch.no_grad():
        logits = net(x.to(DEV))
    assert logits.shape == (2, 4, 64, 96) and logits.dtype == torch.float32
    e = float((logits.double().cpu() - logits64).abs().max() / logits64.abs().max())
    print(f"HyperStarcopUNet(13, 4) eval logits: rel err {e:.3g} of the oracle's float64 logits")
    assert e < 1e-4, e
    # a fresh network, so that predict_classes alone builds the plan: no logits buffer exists for it
    net2 = HyperStarcopUNet(13, 4)
    net2.load_state_dict(sd)
    net2 = net2.to(DEV).eval()
    classes = net2.predict_classes(x.to(DEV))
    assert classes.shape == (2, 64, 96) and classes.dtype == torch.uint8
    assert "logits" not in net2._plans[(2, 64, 96)].buf
    _check_classes(classes, logits64, "predict_classes")
    assert torch.equal(classes, torch.argmax(logits, dim=1).to(torch.uint8))
    with torch.no_grad():
        again = net2(x.to(DEV))         # the same plan now serves a logits call
    assert torch.equal(again, logits)
    with pytest.raises(RuntimeError, match="eval mode"):
        net2.train().predict_classes(x.to(DEV))


def test_cdmodel_predict(hip):
    sd, ref64, _, _ = _oracle_case()
    model = sentinel2.CDModel(device=DEV)
    model.load_state_dict({"model." + k: v for k, v in sd.items()}, strict=True)
    bands = np.random.default_rng(3).standard_normal((13, 50, 77)).astype(np.float32)
    got = model.predict(bands)
    assert isinstance(got, np.ndarray) and got.shape == (50, 77) and got.dtype == np.uint8
    # the reference procedure (starcop/sentinel2/models.py:27-52) with the oracle network
    pad_r, pad_c = (7, 7), (9, 10)
    assert sentinel2.find_padding(50, 32) == pad_r and sentinel2.find_padding(77, 32) == pad_c
    padded = np.pad(bands, ((0, 0), pad_r, pad_c), "reflect")
    assert padded.shape == (13, 64, 96)
    with torch.no_grad():
        logits64 = ref64(torch.from_numpy(padded).double()[None])[0][:, pad_r[0]:-pad_r[1], pad_c[0]:-pad_c[1]]
    _check_classes(torch.from_numpy(got), logits64, "CDModel.predict")
    out = model(torch.from_numpy(padded)[None].to(DEV))
    assert out.shape == (1, 64, 96) and out.dtype == torch.uint8
    with pytest.raises(AssertionError, match="Expected 13 channels found 12"):
        model.predict(bands[:12])


def test_train_mode_is_refused(hip):
    net = HyperStarcopUNet(13, 4).to(DEV).train()
    x = rnd(2, 13, 64, 96, seed=2).to(DEV)
    with pytest.raises(NotImplementedError, match="stem weight gradient.*K-class head"):
        net(x)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        net(x)


def test_default_network_is_unchanged_beside_a_multiclass_one(hip):
    """plans and caches do not leak between shapes: the 4-channel / 1-class logits before and after a 13 / 4 model was built and run"""
    torch.manual_seed(3)
    net = HyperStarcopUNet(4, 1).to(DEV).eval()
    x = rnd(2, 4, 64, 96, seed=4).to(DEV)
    with torch.no_grad():
        first = net(x)
    assert first.shape == (2, 1, 64, 96)
    other = HyperStarcopUNet(13, 4).to(DEV).eval()
    x13 = rnd(2, 13, 64, 96, seed=5).to(DEV)
    with torch.no_grad():
        l13 = other(x13)
    c13 = other.predict_classes(x13)
    assert torch.equal(c13, torch.argmax(l13, dim=1).to(torch.uint8))
    with torch.no_grad():
        second = net(x)
    assert torch.equal(first, second)
    assert torch.equal(net.predict_classes(x), torch.zeros(2, 64, 96, dtype=torch.uint8, device=DEV))
