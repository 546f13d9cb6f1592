"""HyperSTARCOP network: the MobileNetV2-encoder U-Net of ``smp.Unet('mobilenet_v2')`` executed
by hand-written HIP kernels (libstarcop_hip.so) -- forward, backward, eval and train mode.

Reference: ``configure_architecture`` builds ``smp.Unet(encoder_name='mobilenet_v2',
encoder_weights=None, in_channels=C, classes=1, activation=None)``
(/root/reference/starcop/models/model_module.py:224-256).  This module keeps

  * the ``state_dict`` key names/shapes of that network (``encoder.features.N...``,
    ``decoder.blocks.N.convK.M``, ``segmentation_head.0``) so reference checkpoints load,
  * ordinary ``nn.Parameter`` tensors so ``torch.optim.Adam(network.parameters())`` works
    (model_module.py:174), ``.train()/.eval()`` BatchNorm semantics, ``.to(device)``.

The ``torch.nn`` sub-modules are parameter containers only: no torch op computes anything on the
path.  Execution model ("normalise on load"): every convolution stores its RAW output and
accumulates per-channel sum / sum-of-squares in its epilogue; BatchNorm + ReLU/ReLU6 of a producer
are applied by the consumer while it stages tiles into LDS, nearest x2 upsampling and the skip
concat are address arithmetic in the consumer, and the backward pass applies the BatchNorm /
activation backward the same way (g, y -> dy on load).
"""
import collections
import ctypes as C
import math
import os

import torch
import torch.nn as nn

from . import _lib, scene
from ._lib import (ACT_NONE, ACT_RELU, ACT_RELU6, SC_CST, sc_irb_args, sc_irt_args, SRC_AFFINE, SRC_BNBWD, SRC_NORM, SRC_RAW, STAT_BNBWD, sc_wgrad_pending,
                   PACK_PW3, PACK_SP, PACK_SPD, PACK_THIN16, STAT_PW3, STAT_CONV1, STAT_CONV1K, STAT_CONV3, STAT_DW, STAT_STEM, TERMS_F16X2, check, make_src, ptr,
                   sc_conv_args, sc_wgrad_args, stream)

MBV2_SETTINGS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2),
                 (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
DECODER_CHANNELS = (256, 128, 64, 32, 16)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
# where the head of a scene batch writes its cores (_forward_impl(head="mosaic" | "probmosaic")): win / win_host = scene.table_rows of the
# batch; classes: the uint8 mosaic of "mosaic"; prob / mask (either may be None) / valid / fill_bits / nodata: those of "probmosaic"
HeadMosaic = collections.namedtuple("HeadMosaic", "win win_host classes prob mask valid fill_bits nodata", defaults=(None,) * 4 + (0, 0.0))


# ----------------------------------------------------------------------------------------------
# parameter containers (names == smp / torchvision names)
def _conv_bn_act(cin, cout, k, stride=1, groups=1, act="relu6"):
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False),
                         nn.BatchNorm2d(cout, eps=BN_EPS, momentum=BN_MOMENTUM),
                         nn.ReLU6() if act == "relu6" else nn.ReLU())


class _InvertedResidual(nn.Module):
    def __init__(self, cin, cout, stride, t):
        super().__init__()
        hid = cin * t
        self.use_res_connect = stride == 1 and cin == cout
        self.stride, self.expand = stride, t != 1
        layers = []
        if t != 1:
            layers.append(_conv_bn_act(cin, hid, 1))
        layers += [_conv_bn_act(hid, hid, 3, stride, groups=hid),
                   nn.Conv2d(hid, cout, 1, bias=False),
                   nn.BatchNorm2d(cout, eps=BN_EPS, momentum=BN_MOMENTUM)]
        self.conv = nn.Sequential(*layers)


class _Encoder(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        feats = [_conv_bn_act(in_channels, 32, 3, 2)]
        cin = 32
        for t, c, n, s in MBV2_SETTINGS:
            for i in range(n):
                feats.append(_InvertedResidual(cin, c, s if i == 0 else 1, t))
                cin = c
        feats.append(_conv_bn_act(cin, 1280, 1))
        self.features = nn.Sequential(*feats)


class _DecoderBlock(nn.Module):
    def __init__(self, cin, cskip, cout):
        super().__init__()
        self.conv1 = _conv_bn_act(cin + cskip, cout, 3, act="relu")
        self.conv2 = _conv_bn_act(cout, cout, 3, act="relu")


class _Decoder(nn.Module):
    def __init__(self):
        super().__init__()
        cins = (1280,) + DECODER_CHANNELS[:-1]
        cskips = (96, 32, 24, 16, 0)
        self.blocks = nn.ModuleList(_DecoderBlock(i, s, o) for i, s, o in zip(cins, cskips, DECODER_CHANNELS))


# ----------------------------------------------------------------------------------------------
# An activation of the plan.  kind: 'input' | 'raw' (conv output, BN+act applied by readers) | 'fin'.
_T = collections.namedtuple("_T", "name C shift kind bn act")


_COT_RATIO = 1.15      # 64-wide cout tiles when they pad the channel count by less than this factor (measured per layer)
_COT_RATIO3 = 1.15     # the same choice for the 3x3 layers


def _pick_cot(M, ks=1):
    if M <= 16 and ks == 3:
        return 16            # thin layers: v_mfma_f32_16x16x4_f32 kernel, no wasted MFMA rows
    if M <= 32:
        return 32
    p32, p64 = -(-M // 32) * 32, -(-M // 64) * 64
    return 64 if p64 <= p32 * (_COT_RATIO3 if ks == 3 else _COT_RATIO) else 32


# Pointwise convolutions on sc_conv1x1_pw3 / sc_conv1x1_wgrad_pw3 (conv_pw3.hip: split-bf16 MFMA, register-only, no LDS staging)
# or on k_conv_mfma<1> / k_conv1_ksplit / k_wgrad_mfma<1> (fp32 MFMA, LDS staging, K split over the waves of a work-group).
# Measured per layer and pass at batch 4, 16 and 64 (tools/bench_layers.py with STARCOP_PW3=all against =0: profiles/r03a/b_layers_*,
# profiles/r04_layers_b{4,64}_pw3_{all,0}.txt).  What decides is the plane (H*W), the contraction length K and -- new in round 4 --
# how many waves the launch has: the register-only family does not split K, so a long contraction only pays once
# (32-pixel blocks of the batch) x (32-channel output blocks) fills the machine:
#   forward        planes up to 64^2; K <= 320 always, longer K from 1024 (pixel block, output block) pairs
#                  (batch 4: the 32^2 / 16^2 projections stay on the K-splitting kernel, 15-21 vs 23-43 us; batch 64: every one moves
#                  over, 72 vs 103 us on features.15-17)
#   backward-data  K <= 192 (the projections' gradients) on planes up to 64^2 while the batch has <= 131072 pixels of that plane size;
#                  longer K (the expansions' gradients) at <= 32^2 from 2048 pairs (batch 64: 48 vs 73, 83 vs 130, 148 vs 222 us;
#                  batch 16 and 4: the other family, 27 vs 32, 38 vs 68)
#   backward-weight  planes up to 32^2 of at most 32768 batch pixels, small filters (K*M bounds as measured at batch 16)
# "1" = these rules, "all" = every pointwise launch (the tests run both), "0" = off.
_PW3 = os.environ.get("STARCOP_PW3", "1")


def _use_pw3(which, N, HW, Cin, Cout):
    """which: 0 forward, 1 backward-data, 2 backward-weight (reads 8-pixel groups: H*W % 8 == 0) of a Cin -> Cout pointwise layer on
    N planes of HW pixels"""
    if _PW3 == "0" or (which == 2 and HW % 8):
        return False
    if _PW3 == "all":
        return True
    NP = N * HW
    npb = -(-NP // 32)
    if HW == 4096 and which in (0, 1):
        # 64 x 64 planes with a short contraction on the streaming kernel inside sc_conv2d_mfma (k_pw_stream) instead of sc_conv1x1_pw3:
        # the features.5-.7 expansions forward 25-27 -> 21-22 us, the features.4-.6 projections' data gradients 23-30 -> 19-25 us at
        # batch 16 (tools/bench_layers.py, same box); step level to +0.6 % (four alternating pairs)
        K_, M_ = (Cin, Cout) if which == 0 else (Cout, Cin)
        if K_ in (16, 24, 32) and M_ <= 192 and (which == 1 or K_ in (24, 32)):
            return False
    if which == 0:
        return HW <= 4096 and (Cin <= 320 or npb * (-(-Cout // 32)) >= 1024)
    if which == 1:
        K, MB = Cout, -(-Cin // 32)
        return (K <= 192 and HW <= 4096 and NP <= 131072) or (K > 192 and HW <= 1024 and npb * MB >= 2048)
    KM = Cin * Cout
    return HW <= 1024 and NP <= 32768 and KM <= 300000 and (HW <= 256 or KM <= 32768)


# Fused TRAINING execution of the expansion + depthwise pair of a stride-2 inverted-residual block (conv_irt.hip: the 6x-expanded
# tensor and its gradient are never stored, every sweep recomputes it from the block input).  Measured per block (tools/bench_irt.py
# against the launches it replaces, tools/bench_layers.py) and on the whole step (bench.py with STARCOP_IRT=1 / 0, same box):
#   batch 16: features.2 (16 -> 96 channels at 256^2: e = 403 MB) 610 vs 835 us, step +1.3-1.5 %; features.4 (128^2, 151 MB) 414 vs
#             341, features.7 (64^2) 244 vs 143
#   batch 64: features.2 (1.6 GB) step +2.5 % (1555 vs 1517 tiles/s); features.4 (604 MB) 1292 vs 1278: a tie; features.7 loses
#   batch  4: features.2 (101 MB -- the tensor lives in the 256 MB Infinity Cache, the separate kernels' passes over it are cache
#             hits) step -4..6 % (641 vs 674 tiles/s)
# so the recomputation pays where the expanded tensor is large against the cache AND the plane is large: planes >= 256^2 whose e is
# >= 256 MB.  "1" = that rule, "all" = every supported block (tests), "0" = off.
_IRT = os.environ.get("STARCOP_IRT", "1")


def _use_irt(N, Cin, Hd, Hin, Win, stride):
    if _IRT == "0" or not _lib.load().sc_irt_supported(Cin, Hd, Hin, Win, stride):
        return False
    return _IRT == "all" or (Hin * Win >= 65536 and 4 * N * Hd * Hin * Win >= (256 << 20))


# INFERENCE: a stride-1 inverted-residual block (expansion -> depthwise -> projection [-> residual add]) as ONE launch (conv_irb.hip:
# the expanded tensors never leave the CU).  Eval-mode BatchNorm is a per-channel affine, so nothing batch-wide separates the three
# convolutions; at 32 x 32 / 16 x 16 planes the separate launches are 10-35 us each for 3-8 us of work (per block, batch 16, us,
# tools/bench_eval_layers.py, separate -> fused: see DESIGN 16).  "1" = the measured rule, "all" = every supported block (tests),
# "0" = off.
_IRB = os.environ.get("STARCOP_IRB", "1")


def _use_irb(N, Cin, hidden, Cout, H, W, stride):
    """The rule: blocks whose patch fits two work-groups per CU (Cin <= 96, hidden % 64 == 0, Cout <= 128: features.5 / .6 / .8-.13) on
    planes up to 80 x 80, and the stride-2 blocks features.7 / .14 (H, W: the INPUT plane).  features.15-.17 (Cin = 160 at 16 x 16) are NOT taken: every work-group streams the block's whole filter set
    (1.8 MB as three bf16 terms) for a 4 x 8 pixel tile, 128 work-groups of them -- 80-98 us against 74-86 us for the three launches
    (tools/bench_irb.py); splitting the hidden channels over work-groups instead of the pixels is what that shape needs."""
    if _IRB == "0" or not _lib.load().sc_irb_supported(Cin, hidden, Cout, H, W, stride):
        return False
    if _IRB == "all":
        return True
    if stride == 2:       # features.7 (32 -> 192 -> 64 from 64 x 64): 41 vs 54 us; features.14 (96 -> 576 -> 160 from 32 x 32): 74 vs 75 -- not taken
        return Cin <= 64 and hidden % 64 == 0 and H * W <= 25600
    return Cin <= 96 and hidden % 64 == 0 and Cout <= 128 and H * W <= 6400


# Decoder conv1 = conv3x3(cat([nearest_up2(prev), skip])) as a SUB-PIXEL convolution (conv_sp.hip: four phase-specific 2x2
# convolutions on the low-resolution prev, the skip channels as low-resolution parity planes: 2.25x fewer MFMAs for the up-sampled
# channels, every low-resolution value staged once instead of once per high-resolution copy).  Measured against sc_conv3x3_bx3 with
# an up-sampled source (tools/bench_sp.py, us per launch, batch 16): decoder.blocks.0 311 -> 288 (16 x 16 low-resolution planes: 128
# work-groups of 8 waves for 256 CUs; 1131 -> 778 at batch 64), blocks.1 125 -> 79, blocks.2 147 -> 104, blocks.3 178 -> 122; blocks.4
# (16 output channels: half-empty MFMA rows) 196-213, level with sc_conv3x3_thin16's 202, stays there.  "1" = that rule, "all" =
# every decoder conv1 (tests), "0" = off.
_SP = os.environ.get("STARCOP_SP", "1")
_SP_TERMS = (TERMS_F16X2, 1)      # arithmetic modes of the sub-pixel forward / data-gradient kernels (conv_sp.hip)


def _use_sp(N, Ho, Wo, Cout):
    """forward of a decoder conv1 with an Ho x Wo output on sc_conv3x3_sp?"""
    if _SP == "0" or Ho % 2 or Wo % 2:
        return False
    if _SP == "all":
        return True
    Hl, Wl = Ho // 2, Wo // 2
    tw = 32 if Wl >= 32 else 16
    wgs = N * (-(-Wl // tw)) * (-(-Hl // (256 // tw))) * (-(-Cout // 32))
    return Cout >= 32 and wgs >= 128


def _use_spd(N, Ho, Wo, Cup, Csk=0):
    """data gradient of a decoder conv1's up-sampled channels on sc_conv3x3_sp_dgrad?  (tools/bench_sp.py, us, batch 16, against
    sc_conv3x3_bx3(down0) on the same channels: decoder.blocks.0 336 -> 250, blocks.1 140 -> 129, blocks.2 148 -> 83; blocks.3 / .4 have
    64 / 32 such channels for the kernel's 128-channel tiles: 176 -> 190, 285 -> 500 -- they keep the 3x3 form)"""
    if _SP == "0" or Ho % 2 or Wo % 2:
        return False
    return _SP == "all" or Cup >= 128 or (Csk and _lib.load().sc_spd_vskip_ok(Cup, Csk))       # (.. or ONE launch for both gradients)


def _use_spd_skip_tiles(Cup, Csk):
    """the skip channels' gradient of a decoder conv1 as additional channel tiles of its sub-pixel data-gradient launch (instead of a
    3x3 launch of its own on 32-wide tiles, which stages dy again)?  Each skip tile costs what a tile of 128 up-sampled channels costs,
    so it pays where the skip channels are few tiles beside many: decoder.blocks.0 (10 + 3 tiles; the 3x3 launch it replaces: 54 us at
    batch 16).  decoder.blocks.1 (2 + 1): level; blocks.2 (1 + 1: twice the launch for a 50 us one): no."""
    if _SP == "all":
        return True
    return _SP != "0" and Cup >= 1024 and -(-Csk // 32) * 3 <= -(-Cup // 128)


def _use_spw(N, Ho, Wo, Cout, Cup):
    """weight gradient of a decoder conv1's up-sampled channels as the box-sum GEMM of conv_spw.hip?  up(x) is constant over 2x2 output
    blocks, so dW[kh][kw] = sum_q x[q] S_(kh,kw)[q] with S tap-aligned 2x2 box sums of dy: nine plain GEMMs over the low-resolution
    pixels, a quarter of the multiply-adds -- but the nine box-sum planes (2.25x the size of dy, as two fp16 terms) are written and
    read once, which only pays where the layer is matrix-bound (tools/bench_sp.py, us at batch 16, up-sampled channels alone, 3x3 form
    -> box-sum GEMM: decoder.blocks.0 338 -> 222, blocks.1 143 -> 147, blocks.2 148 -> 228, blocks.3 186 -> 482)"""
    if _SP == "0" or Ho % 2 or Wo % 2:
        return False
    return _SP == "all" or Cup >= 512


def _use_ksplit(N, HW, K, M, ks=1):
    """1x1 layers with few pixels and long K: the split-K kernel (sc_conv1x1_ksplit) beats the 128-pixel tiles when
    those leave most CUs idle (measured crossover, tools/bench_pw.py)."""
    if ks != 1:
        return False
    wgs = N * (-(-HW // 128)) * (-(-M // _pick_cot(M, 1)))
    return wgs <= 512 and (K >= 384 or (K >= 192 and wgs <= 256))


# ----------------------------------------------------------------------------------------------
# Which kernel runs a pass of a pointwise / 3x3 layer at a shape and precision: ONE answer per pass (_fwd_route, _dgrad_route,
# _wgrad_route) and one for the filter layouts a layer can be sent to (_layouts), built from the measured rules above.  Everything
# else reads these: the statistics rows and workspaces of a plan (_get_plan), the packed layouts (_pack_all), both walks, the profile
# families and kernel_table().  They need no device.
# static facts of a layer; Cup / Csk: the up-sampled / skip channels of a decoder conv1 (0 elsewhere)
_Layer = collections.namedtuple("_Layer", "type Cout Cin ks up Cup Csk nsrc")
# A route names everything its launch needs: the entry point, the filter layout, the cout tile, the profile family.
# _Fwd.rows: per-work-group partial rows of the BatchNorm statistics.  _Dgrad.launches: (entry, layout, cout tile, down0, sources whose
# gradient the launch writes), down0 = 1: the kernel stores the 2x2 sums itself, 2: full resolution into up_tmp, then sc_downsum2x2;
# _Dgrad.fallback: the route the walk takes where the preferred kernel's plain epilogue does not do.  _Wgrad.skip: the route of the skip
# channels' columns beside the box-sum GEMM.
_Fwd = collections.namedtuple("_Fwd", "kernel entry layout cot rows family")
_Dgrad = collections.namedtuple("_Dgrad", "kernel launches family fallback", defaults=(None,))
_Wgrad = collections.namedtuple("_Wgrad", "kernel entry family skip", defaults=(None,))
_Routes = collections.namedtuple("_Routes", "fwd dgrad wgrad")
_PACK_ORDER = ("f", "b", "bA", "bB", "spd", "sp", "tf", "tb", "tsd", "pf", "pb", "pfi")      # rows of the pack table, per layer
_BWD_LAYOUTS = frozenset(("b", "bA", "bB", "spd", "tb", "tsd", "pb"))                        # ... of which a forward-only pack leaves out


def _tiles(L, split):
    """(forward, backward) cout-tile widths of a layer's packed filters, and whether each direction runs split (bx3): 3x3 layers with
    >= 32 output channels run on the 16-bit matrix cores with exactly-split operands (fp32-level accuracy, conv_bx3.hip; `precision`
    picks the split); thin ones stay on the fp32 MFMA kernels"""
    cf, cb = _pick_cot(L.Cout, L.ks), _pick_cot(L.Cin, L.ks)
    if L.ks == 3 and L.Cout <= 16 and L.Cin >= 32 and split:
        cf = 32       # decoder.blocks.4.conv1 (32 -> 16): the split kernel with half-empty cout blocks still beats
                      # the fp32-MFMA thin kernel (0.36 vs 0.50 ms); 16 -> 16 layers do not (tools/bench_thin_bx3.py)
    return cf, cb, bool(split and L.ks == 3 and cf >= 32), bool(split and L.ks == 3 and cb >= 32)


def _family(kind, ks, terms, which):
    """profile family of a forward (which = "fwd") or data-gradient ("dgrad") launch.  The split-bf16 3x3 kernel: forward and dgrad
    launches are one family unless they run with a different number of terms (then their MFMA ceilings differ)"""
    if kind == "bx3":
        return "k_conv3_bx3 (fwd+dgrad)" if terms[0] == terms[1] else f"k_conv3_bx3 ({which})"
    return "k_conv3_thin_h (fwd+dgrad)" if kind == "thin" else f"k_conv_mfma<{ks}> (fwd+dgrad)"


def _spd_skip(L):
    """how the skip channels' gradient of a decoder conv1 rides with its sub-pixel data gradient: "vskip" (decoder.blocks.3: in the
    same launch), "stiles" (additional channel tiles of that launch, where measured faster than a 3x3 launch of its own), "bx3" (a
    3x3 launch on a 32-wide pack) or None (no skip source)"""
    if not L.Csk:
        return None
    if _lib.load().sc_spd_vskip_ok(L.Cup, L.Csk):
        return "vskip"
    return "stiles" if _use_spd_skip_tiles(L.Cup, L.Csk) else "bx3"


def _layouts(L, split, terms):
    """{layout: (floats, co_t, tflip, bx3 code of its sc_pack_desc)}: the filter layouts a layer's routes can name at this precision
    (split: split_bf16; terms: (forward, backward)).  Which of a pointwise layer's two families are packed follows the shapes in use
    (HyperStarcopUNet._pw_need)."""
    lib = _lib.load()
    co, ci, ks, (tf_, tb_) = L.Cout, L.Cin, L.ks, terms
    cf, cb, xf, xb = _tiles(L, split)
    lay = {"f": (lib.sc_packed_weight_floats_bx3(co, ci, cf, 0, tf_) if xf else lib.sc_packed_weight_floats(co, ci, ks, cf, 0), cf, 0, tf_ if xf else 0),
           "b": (lib.sc_packed_weight_floats_bx3(co, ci, cb, 1, tb_) if xb else lib.sc_packed_weight_floats(co, ci, ks, cb, 1), cb, 1, tb_ if xb else 0)}
    if L.type == "pw":
        for flip, name in enumerate(("pf", "pb")):
            lay[name] = (lib.sc_packed_weight_floats_pw3(co, ci, flip), 0, flip, PACK_PW3)
        lay["pfi"] = lay["pf"]      # a fused inference block's own copy of "pf" (HyperStarcopUNet._wanted_layouts)
        return lay
    # decoder.blocks.4 (<= 16 output channels at full resolution) under the two-fp16-term split: filters in registers
    # (sc_conv3x3_thin16; 0.20-0.28 vs 0.31-0.51 ms per launch).  The backward-data kernel only takes the plain
    # epilogue, so the regular pack is kept beside it.
    thin = {"tf": split and tf_ == TERMS_F16X2 and co <= 16 and ci in (16, 32), "tb": split and tb_ == TERMS_F16X2 and ci <= 16 and co in (16, 32),
            # decoder.blocks.4.conv1: the half-resolution data gradient in its sub-pixel form (sc_conv3x3_thin16 with down0)
            "tsd": split and tb_ == TERMS_F16X2 and L.up and co == 16 and ci == 32}
    for flip, name in ((0, "tf"), (1, "tb"), (1, "tsd")):
        if ks == 3 and L.nsrc == 1 and thin[name]:
            lay[name] = (lib.sc_packed_weight_floats_thin16(co, ci, flip), 16, flip, PACK_THIN16)
    sk = _spd_skip(L)
    spd = L.up and xb and tb_ in _SP_TERMS and _SP != "0" and L.Cup % 32 == 0
    # decoder conv1 data gradient (up-sampled channels + skip channels): the two outputs as TWO launches with their own
    # cout tiles -- 64-wide for the up-sampled part (a multiple of 64), one 32-wide tile for the <= 32 skip channels --
    # instead of one launch of 32-wide tiles (80 = 64 + 16: 3 x 32; 152 = 128 + 24: 5 x 32): every cout tile stages (loads,
    # BatchNorm-backward prologue, split) the whole gradient patch again.  Measured at 16 x 512^2: decoder.blocks.2.conv1
    # 212 -> 197 us (5 -> 3 passes), decoder.blocks.3.conv1 293 -> 288 us (a 64-wide pass costs two 32-wide ones there: the
    # operand reads and MFMAs, not the staging, are what its work-groups wait for); 288 = 256 + 32, which already runs on
    # 64-wide tiles, loses 5 us to the second launch and stays as it was.  Step +0.6 % (same-box pairs).
    split2 = xb and cb == 32 and L.up and L.nsrc == 2 and L.Cup % 64 == 0 and L.Csk <= 32
    for cot, name in ((64, "bA"), (32, "bB")):
        if split2 or (name == "bB" and spd and sk == "bx3"):
            lay[name] = (lib.sc_packed_weight_floats_bx3(co, ci, cot, 1, tb_), cot, 1, tb_)
    # decoder conv1 forward as a sub-pixel convolution (the two-fp16-term arithmetic or, "bf16", one bf16 term): phase /
    # parity filters (tflip | 4: the one-bf16-term layout)
    if L.up and xf and tf_ in _SP_TERMS and _SP != "0":
        lay["sp"] = (lib.sc_packed_weight_floats_sp(co, L.Cup, L.Csk), L.Cup, 4 if tf_ == 1 else 0, PACK_SP)
    # ... and the data gradient of its up-sampled channels (the skip channels' gradient: see _spd_skip)
    if spd:
        lay["spd"] = (lib.sc_packed_weight_floats_spd(co, L.Cup, L.Csk if sk == "stiles" else 0), L.Cup,
                      {"stiles": 3, "vskip": 2}.get(sk, 1) | (4 if tb_ == 1 else 0), PACK_SPD)
    return lay


def _fwd_route(L, N, Ho, Wo, split, terms):
    """forward kernel of a pointwise / 3x3 layer with an Ho x Wo output plane"""
    lib = _lib.load()
    cf, _, xf, _ = _tiles(L, split)
    mfma = _family("mfma", L.ks, terms, "fwd")
    if L.type == "pw":
        if _use_pw3(0, N, Ho * Wo, L.Cin, L.Cout):
            return _Fwd("pw3", "sc_conv1x1_pw3", "pf", cf, lib.sc_stat_rows(STAT_PW3, N, Ho, Wo), mfma)
        if _use_ksplit(N, Ho * Wo, L.Cin, L.Cout):
            return _Fwd("ksplit", "sc_conv1x1_ksplit", "f", cf, lib.sc_stat_rows(STAT_CONV1K, N, Ho, Wo), mfma)
        return _Fwd("mfma", "sc_conv2d_mfma", "f", cf, lib.sc_stat_rows(STAT_CONV1, N, Ho, Wo), mfma)
    lay, bx3 = _layouts(L, split, terms), _family("bx3", 3, terms, "fwd")
    if "sp" in lay and _use_sp(N, Ho, Wo, L.Cout):       # one partial row per work-group tile
        return _Fwd("sp", "sc_conv3x3_sp", "sp", cf, lib.sc_sp_stat_rows(N, Ho, Wo, L.Cout), bx3)
    rows = lib.sc_stat_rows(STAT_CONV3, N, Ho, Wo)
    if "tf" in lay:
        return _Fwd("thin16", "sc_conv3x3_thin16", "tf", cf, rows, _family("thin", 3, terms, "fwd"))
    # (a 3x3 layer never takes the K-split kernel: _use_ksplit)
    return _Fwd("bx3", "sc_conv3x3_bx3", "f", cf, rows, bx3) if xf else _Fwd("mfma", "sc_conv2d_mfma", "f", cf, rows, mfma)


def _dgrad_route(L, N, Ho, Wo, split, terms):
    """data-gradient kernel(s) of a layer"""
    cb, xb = _tiles(L, split)[1::2]
    lay, every = _layouts(L, split, terms), tuple(range(L.nsrc))
    bx3, thin = _family("bx3", 3, terms, "dgrad"), _family("thin", 3, terms, "dgrad")
    if "spd" in lay and _use_spd(N, Ho, Wo, L.Cup, L.Csk):
        # sub-pixel form: the up-sampled channels' gradient at half resolution from the four parity planes of dy (2.25x fewer MFMAs,
        # 128 output channels per staged patch), the skip channels' by the 3x3 kernel on their own 32-wide tiles ("bx3") -- or in the SAME
        # launch, dy (g, y) staged ONCE for both gradients: <= 64 up-sampled + <= 16 skip channels (decoder.blocks.3, "vskip") as virtual
        # channels of the 128-channel tile's second half (289 us in two 3x3 launches before); "stiles": as additional channel tiles of
        # the launch (32 skip channels x 4 output parities each)
        sk = _spd_skip(L)
        if sk == "bx3":
            return _Dgrad("spd+bx3", (("sc_conv3x3_sp_dgrad", "spd", cb, 0, (0,)), ("sc_conv3x3_bx3", "bB", 32, 0, (1,))), bx3)
        return _Dgrad("spd+" + sk if sk else "spd", (("sc_conv3x3_sp_dgrad", "spd", cb, 0, every),), bx3)
    # decoder.blocks.4.conv1: 16 gradient channels -> 32 channels at half resolution, the sub-pixel form on the thin layer's MFMA
    # (sc_conv3x3_thin16 with down0: 251 -> see DESIGN 16; otherwise sc_conv3x3_bx3 with its summing store)
    if "tsd" in lay and Ho % 2 == 0 and Wo % 2 == 0:
        return _Dgrad("thin16_down", (("sc_conv3x3_thin16", "tsd", 16, 1, (0,)),), thin)
    if L.up and xb and "bA" in lay:
        return _Dgrad("bx3_split", (("sc_conv3x3_bx3", "bA", 64, 1, (0,)), ("sc_conv3x3_bx3", "bB", 32, 0, (1,))), bx3)
    # ONE ordinary convolution with the flipped filter; a decoder conv1's up-sampled source gets the 2x2 sums (down0)
    down = (1 if xb else 2) if L.up else 0
    if xb:
        plain = _Dgrad("bx3", (("sc_conv3x3_bx3", "b", cb, down, every),), bx3)
    elif L.type == "pw" and _use_pw3(1, N, Ho * Wo, L.Cin, L.Cout):
        plain = _Dgrad("pw3", (("sc_conv1x1_pw3", "pb", cb, 0, every),), _family("mfma", 1, terms, "dgrad"))
    else:
        ksplit = _use_ksplit(N, Ho * Wo, L.Cout, L.Cin, L.ks)
        plain = _Dgrad(("ksplit" if ksplit else "mfma") + ("+downsum" if L.up else ""),
                       (("sc_conv1x1_ksplit" if ksplit else "sc_conv2d_mfma", "b", cb, down, every),), _family("mfma", L.ks, terms, "dgrad"))
    if "tb" in lay and not L.up:      # (the thin kernel only takes the plain epilogue: no accumulation, no residual target)
        return _Dgrad("thin16", (("sc_conv3x3_thin16", "tb", cb, 0, every),), thin, plain)
    return plain


def _wgrad_route(L, N, Ho, Wo, split, terms):
    """weight-gradient kernel of a layer"""
    f16 = split and terms[1] == TERMS_F16X2
    mfma = _Wgrad("mfma", "sc_conv2d_wgrad_mfma", f"k_wgrad_mfma<{L.ks}> (+reduce)")
    bx3 = _Wgrad("bx3", "sc_conv3x3_wgrad_bx3", "k_wgrad3_bx3 (+reduce)")
    if L.up and f16 and _use_spw(N, Ho, Wo, L.Cout, L.Cup):
        # decoder conv1 with many up-sampled channels: their filter gradient as nine plain GEMMs between the low-resolution source
        # and tap-aligned 2x2 box sums of dy (conv_spw.hip); the skip channels' columns from the 3x3 kernel on the skip source alone
        return _Wgrad("spw", "sc_conv3x3_sp_wgrad", bx3.family, None if L.nsrc == 1 else bx3 if (L.Cout >= 32 and L.Csk >= 32) else mfma)
    if L.type == "pw":      # K-slice partials kept until the batched reduction (HyperStarcopUNet._size_backward)
        return (_Wgrad("pw3", "sc_conv1x1_wgrad_pw3", mfma.family) if _use_pw3(2, N, Ho * Wo, L.Cin, L.Cout)
                else mfma._replace(entry="sc_conv2d_wgrad_mfma_deferred"))
    if f16 and L.ks == 3 and L.nsrc == 1 and L.Cout <= 16 and L.Cin in (16, 32) and Wo % 2 == 0:
        # decoder.blocks.4: two fp16 terms on the 16x16x32 MFMA (was MFMA-bound in fp32)
        return _Wgrad("thin16", "sc_conv3x3_wgrad_thin16", "k_wgrad_thin_h (+reduce)")
    # 16-channel layers outside the cases above stay on the fp32 MFMA
    return bx3 if (split and L.ks == 3 and L.Cout >= 32 and L.Cin >= 32) else mfma


def _wgrad_floats(kernel, N, Ho, Wo, Cout, Cin, ks):
    """K-slice partials (floats) a weight-gradient kernel needs"""
    if kernel == "mfma":
        return _lib.load().sc_wgrad_workspace_floats(N, Ho, Wo, Cout, Cin, ks)
    return getattr(_lib.load(), f"sc_wgrad_{kernel}_workspace_floats")(N, Ho, Wo, Cout, Cin)


def _block_table(raw, totals, dev):
    """device table of a batched launch whose descriptors share 256-item blocks: (descriptor bytes, first block of each, count, blocks)"""
    import numpy as np
    starts = np.cumsum([0] + [-(-int(t) // 256) for t in totals]).tolist()
    return (torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dev), torch.tensor(starts[:-1], dtype=torch.int32).to(dev),
            len(totals), starts[-1])


class _BwdWalk:
    """state of one backward walk (HyperStarcopUNet._backward_impl)"""
    def __init__(self, plan, st, dlogits, half_bwd):
        self.plan, self.st, self.dlogits, self.half_bwd = plan, st, dlogits, half_bwd      # st: handle of the main stream
        self.side = self.sd = None         # the weight-gradient stream and its handle (overlap_wgrad)
        self.last_pw = min(plan.pw_part, default=-1)      # the pointwise layer the walk reaches last
        self.written = set()       # tensors whose gradient buffer holds a contribution (the next writer accumulates)
        self.reduced = set()       # tensors whose BatchNorm-backward sums were produced by the launch that wrote their gradient
        self.pw_pending = []       # pointwise weight gradients whose K-slice partials await the batched reduction
        self.dw_casts = []         # (fp64 accumulator, flat fp32 gradient view, n) of the fused depthwise backward launches walked so far
        self.gmax_slot = {}        # tensor -> its slot of plan.gmax (the range hint of the fp16-split kernels)
        self.irt_done = set()      # expand ops a fused block's backward has covered


class HyperStarcopUNet(nn.Module):
    """Drop-in for ``ModelModule.network`` (smp.Unet mobilenet_v2), running on libstarcop_hip.so."""

    def __init__(self, in_channels=4, classes=1):
        super().__init__()
        # inference runs for every pair below; training needs classes == 1 (starcop/config.yaml:40 num_classes: 1) and
        # in_channels <= 8 -- refused at the first training forward (_forward_impl), so that such a model still loads and predicts
        if not (1 <= classes <= self.MAX_CLASSES):
            raise ValueError(f"HyperStarcopUNet: classes must be in [1, {self.MAX_CLASSES}] (sc_head_conv_fwd_k)")
        if not (1 <= in_channels <= self.MAX_IN_CHANNELS):
            raise ValueError(f"HyperStarcopUNet: in_channels must be in [1, {self.MAX_IN_CHANNELS}] (sc_stem_conv_fwd)")
        self.in_channels, self.classes = in_channels, classes
        self.encoder = _Encoder(in_channels)
        self.decoder = _Decoder()
        self.segmentation_head = nn.Sequential(nn.Conv2d(DECODER_CHANNELS[-1], classes, 3, padding=1))
        self.reset_parameters()
        self._ops, self._tensors = self._build_ops()
        self._plans = {}
        self._pflat = self._gflat = None
        self._pack_version = None
        self._wpk, self._pack_tables = {}, {}      # layer -> packed filter layouts (_pack_all); its device-side descriptor tables
        self._pw_need = {}                         # pointwise layer -> the layouts some plan's routes name (sticky over all plans)
        self._irb_layers = set()                   # pointwise layers inside a fused inference block of some plan
        self._nbt = None                           # the BatchNorm step counters (_nbt_list)
        self.register_load_state_dict_post_hook(HyperStarcopUNet._after_load)

    MAX_IN_CHANNELS, MAX_CLASSES = 16, 8                 # forward kernels: the stem's channels, the head's classes
    MAX_TRAIN_IN_CHANNELS, MAX_TRAIN_CLASSES = 8, 1      # ... of which sc_stem_conv_wgrad / sc_head_conv_bwd cover these

    @staticmethod
    def _after_load(module, incompatible_keys):
        module.check_split_range()          # (a post hook must return None)

    # -- range of the default (two-fp16-term) split: filters are scaled by 2^8 and activations by 2 before the fp16 conversion
    FP16_MAX_WEIGHT, FP16_MAX_ACT = 255.0, 32752.0
    range_check_every = 200     # optimiser steps between two check_split_range() calls during training (0: never)

    def _split_feeders(self):
        """inputs of the split 3x3 convolutions: (BatchNorm'd tensors whose activation is not bounded by ReLU6, residual sums)"""
        raw, fin = [], []
        for op in self._ops:
            if op["type"] == "conv3":        # every decoder convolution stages fp16 terms (k_conv3_bx3 / _ws / k_conv3_thin_h)
                for t in op["ins"]:
                    if t.kind == "fin" and t.name not in fin:
                        fin.append(t.name)
                    elif t.kind == "raw" and t.act != ACT_RELU6 and t.name not in raw:
                        raw.append(t.name)
        return raw, fin

    def split_range_report(self, sync_ranks=False):
        """The operands of the split 3x3 convolutions against the limits of the two-fp16-term kernels:

        * largest |filter| (limit 255: filters are scaled by 2^8 before the fp16 conversion);
        * ``activation_observed``: the largest |activation| that has reached one of them so far, from DEVICE-SIDE STICKY RECORDS --
          for BatchNorm-fed inputs ``sc_bn_bwd_reduce / sc_bn_bwd_small`` leave max |BN(y)| of every training step (they stream y
          anyway), in inference ``sc_add_srcs_absmax(out=NULL)`` records it at the ``range_check_every`` cadence; residual sums
          (no BatchNorm bounds them) are recorded by ``sc_add_srcs_absmax`` in every forward.  The records are never lowered, so a
          check at any later time sees every step since the last one: there is no window in which a clamp goes unnoticed;
        * ``activation_bound``: the static bound max_c(64 |gamma_c| + |beta_c|) (|x_hat| <= 64 covers every realistic tile) --
          what can be said about a checkpoint before any data has flowed (``load_state_dict``).

        Synchronises the device.  ``sync_ranks``: MAX over the ranks of an initialised process group, so that every replica of a
        data-parallel job takes the same decision (FusedAdam passes it; all ranks step together there).  The all-reduce also
        carries ``switched`` -- 1 if ANY rank has already left the two-fp16-term mode on its own (an inference forward on
        rank-local data may do that, ``_forward_impl``) -- and is issued by every rank whatever its own precision, so the
        collective sequence of the replicas never diverges."""
        wmax = amax = rmax = omax = 0.0
        raw_feed, fin_feed = self._split_feeders()
        for plan in self._plans.values():
            for n, i in plan.fin_slot.items():
                if n in fin_feed:
                    rmax = max(rmax, float(plan.fin_amax[i]))
            if plan.act_slot:
                omax = max(omax, float(plan.act_amax.max()))
        for op in self._ops:
            if op["type"] != "conv3":
                continue
            wmax = max(wmax, float(op["conv"].weight.detach().abs().max()))
            for t in op["ins"]:
                bn = getattr(t, "bn", None)
                if bn is not None and t.act != ACT_RELU6:
                    amax = max(amax, float((64.0 * bn.weight.detach().abs() + bn.bias.detach().abs()).max()))
        switched = float(self._range_switched)
        if sync_ranks and torch.distributed.is_available() and torch.distributed.is_initialized() and self._pflat is not None:
            v = torch.tensor([wmax, amax, rmax, omax, switched], dtype=torch.float32, device=self._pflat.device)
            torch.distributed.all_reduce(v, op=torch.distributed.ReduceOp.MAX)
            wmax, amax, rmax, omax, switched = (float(x) for x in v.tolist())
        # Round 5: activations can no longer leave the range -- every split convolution scales its fp16 operand from a device-side
        # bound of its sources (h_act_scale in sc_split.h: |gamma| sqrt(n - 1) + |beta| from sc_bn_finalize in training, the
        # recorded maxima for residual sums / in inference), so only the FILTERS (scaled by a fixed 2^8 at pack time) decide `ok`;
        # the activation figures stay in the report (activation_default_scale: the fixed x2 of rounds 1-4 still applies to all).
        #  Inference has no by-construction bound: BatchNorm runs on running statistics and the scales follow the sticky
        # records, which are refreshed at the range_check_every cadence only.  With the cadence OFF (0) nothing would ever notice a
        # clamp, so the observed / residual maxima stay part of `ok` there; `inference_clamped` counts the forwards whose recheck found
        # a tensor beyond the scale that was in force (each of them warned; the last one of a redo chain is NOT repaired).
        act_ok = bool(self.range_check_every) or max(omax, rmax) * 2.0 <= self.FP16_MAX_ACT
        return dict(max_abs_filter=wmax, filter_limit=self.FP16_MAX_WEIGHT, activation_bound=amax, activation_observed=omax,
                    activation_limit=self.FP16_MAX_ACT, residual_absmax=rmax, switched=bool(switched),
                    activation_default_scale=bool(max(omax, rmax) < self.FP16_MAX_ACT / 2),
                    inference_clamped=int(self._inference_clamped), inference_unrepaired=int(self._inference_unrepaired),
                    ok=bool(wmax < self.FP16_MAX_WEIGHT and not switched and act_ok and not self._inference_unrepaired))

    _range_switched = False      # this replica left precision "fp32" because of a range check (reported to the other ranks)
    _inference_clamped = 0       # inference forwards whose range recheck found a clamped operand (each was redone with adapted scales)
    _inference_unrepaired = 0    # ... of which the redo chain gave up (6 re-runs): the returned logits carry clamped operands

    def check_split_range(self, sync_ranks=False):
        """A checkpoint (or a training run) whose filters or activations leave the fp16 range of the default split continues with
        the three-term bf16 split (fp32's exponent range); the warning says how long operands may have been clamped.

        With ``sync_ranks`` the report's all-reduce runs on EVERY rank, also on one that has already switched (or was configured
        with another precision): a rank that skipped it would leave the others waiting in the collective."""
        multi = (sync_ranks and torch.distributed.is_available() and torch.distributed.is_initialized()
                 and torch.distributed.get_world_size() > 1)
        if self.precision != "fp32" and not multi:
            return True          # (the report synchronises the device: only taken where its collective is owed to the other ranks)
        rep = self.split_range_report(sync_ranks)
        if self.precision != "fp32":
            return True
        if not rep["ok"]:
            import warnings
            warnings.warn(f"HyperStarcopUNet: filters outside the range of the two-fp16-term kernels ({rep}); "
                          f"switching to precision='fp32-x3' (three bf16 terms, no range limits)"
                          + ("; another rank of the process group had already switched" if rep["switched"] else ""))
            self.precision = "fp32-x3"
            self._range_switched = True
        return rep["ok"]

    def _record_activation_range(self, plan):
        """inference: one streaming pass per BatchNorm-fed input of a split convolution, raising its sticky record (training steps
        get the same record for free from the BatchNorm-backward reductions)"""
        lib = _lib.load()
        st = stream()
        for name, slot in plan.act_slot.items():
            t = self._tensors[name]
            s = self._src_of(plan, t)
            check(lib.sc_add_srcs_absmax(C.byref(s), None, None, plan.N, t.C, (plan.H >> t.shift) * (plan.W >> t.shift),
                                         plan.act_amax.data_ptr() + 4 * slot, st))

    # -- init conventions of torchvision MobileNetV2 / smp initialize_decoder / initialize_head
    def reset_parameters(self):
        for m in self.encoder.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight); nn.init.zeros_(m.bias)
        if self.in_channels != 3:
            self.encoder.features[0][0].reset_parameters()
        for m in self.decoder.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, mode="fan_in", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight); nn.init.zeros_(m.bias)
        head = self.segmentation_head[0]
        nn.init.xavier_uniform_(head.weight); nn.init.zeros_(head.bias)

    # ------------------------------------------------------------------------------------------
    def _build_ops(self):
        ops, tensors = [], {}
        ir_blocks = self._ir_blocks = {}

        def T(name, Cn, shift, kind, bn=None, act=ACT_NONE):
            t = _T(name, Cn, shift, kind, bn, act)
            tensors[name] = t
            return t

        x = T("x", self.in_channels, 0, "input")
        f = self.encoder.features
        cur = T("f0", 32, 1, "raw", f[0][1], ACT_RELU6)
        ops.append(dict(type="stem", conv=f[0][0], ins=[x], out=cur))
        skips = {}
        for idx in range(1, 18):
            blk = f[idx]
            cin_t = cur
            seq = blk.conv
            j = 0
            h = cur
            if blk.expand:
                e = T(f"f{idx}e", seq[0][0].out_channels, cur.shift, "raw", seq[0][1], ACT_RELU6)
                ops.append(dict(type="pw", conv=seq[0][0], ins=[h], out=e))
                h, j = e, 1
            sh = h.shift + (1 if blk.stride == 2 else 0)
            d = T(f"f{idx}d", seq[j][0].out_channels, sh, "raw", seq[j][1], ACT_RELU6)
            ops.append(dict(type="dw", conv=seq[j][0], stride=blk.stride, ins=[h], out=d))
            p = T(f"f{idx}p", seq[j + 1].out_channels, sh, "raw", seq[j + 2], ACT_NONE)
            ops.append(dict(type="pw", conv=seq[j + 1], ins=[d], out=p))
            if blk.expand:
                ir_blocks[len(ops) - 3] = (len(ops) - 2, len(ops) - 1, blk.stride)      # expand op -> (depthwise op, project op, stride)
            if blk.use_res_connect:
                z = T(f"f{idx}", p.C, sh, "fin")
                ops.append(dict(type="add", ins=[cin_t, p], out=z))
                cur = z
            else:
                cur = p
            if idx in (1, 3, 6, 13):
                skips[idx] = cur
        last = T("f18", 1280, cur.shift, "raw", f[18][1], ACT_RELU6)
        ops.append(dict(type="pw", conv=f[18][0], ins=[cur], out=last))
        cur = last
        skip_list = [skips[13], skips[6], skips[3], skips[1], None]
        for b, blk in enumerate(self.decoder.blocks):
            sh = cur.shift - 1
            ins = [cur] + ([skip_list[b]] if skip_list[b] is not None else [])
            o1 = T(f"d{b}a", blk.conv1[0].out_channels, sh, "raw", blk.conv1[1], ACT_RELU)
            ops.append(dict(type="conv3", conv=blk.conv1[0], ins=ins, up=True, out=o1))
            o2 = T(f"d{b}b", blk.conv2[0].out_channels, sh, "raw", blk.conv2[1], ACT_RELU)
            ops.append(dict(type="conv3", conv=blk.conv2[0], ins=[o1], up=False, out=o2))
            cur = o2
        logits = T("logits", self.classes, 0, "fin")
        ops.append(dict(type="head", conv=self.segmentation_head[0], ins=[cur], out=logits))
        # tables of the backward walk (_backward_impl)
        self._res_of = {op["ins"][0].name: op["out"].name for op in ops if op["type"] == "add"}      # tensor -> the residual sum z = t + ...
        # consumers per tensor: a gradient is complete after ONE launch only for single-consumer tensors
        self._n_cons = collections.Counter(t.name for op in ops for t in op["ins"])
        self._prod_idx = {op["out"].name: k for k, op in enumerate(ops)}      # producer op of every tensor (its range-hint slot)
        self._dw_offs, off = {}, 0      # depthwise op -> offset of its filter gradient in plan.dw_acc
        for i, op in enumerate(ops):
            if op["type"] == "dw":
                self._dw_offs[i] = off
                off += op["conv"].out_channels * 9
        self._last_dw = min(self._dw_offs, default=-1)      # the depthwise op the backward walk reaches last
        self._tail_lo = sum(p.numel() for p in self.encoder.parameters())      # flat offset of the decoder's / head's parameters
        self._layers = {}       # pointwise / 3x3 op -> its static facts, what the routes (_fwd_route ...) decide from
        for i, op in enumerate(ops):
            if op["type"] in ("pw", "conv3"):
                cv, cup = op["conv"], op["ins"][0].C if op.get("up") else 0
                self._layers[i] = _Layer(op["type"], cv.out_channels, cv.in_channels, cv.kernel_size[0], bool(op.get("up")), cup,
                                         cv.in_channels - cup if cup else 0, len(op["ins"]))
        return ops, tensors

    # ------------------------------------------------------------------------------------------
    # flat parameter / gradient storage (one fused Adam pass, one RCCL all-reduce)
    def _ensure_flat(self):
        params = list(self.parameters())
        dev = params[0].device
        ok = self._pflat is not None and self._pflat.device == dev
        if ok:
            off = 0
            base = self._pflat.data_ptr()
            for p in params:
                if p.data_ptr() != base + 4 * off or p.dtype != torch.float32:
                    ok = False
                    break
                off += p.numel()
        if not ok:
            total = sum(p.numel() for p in params)
            flat = torch.empty(total, dtype=torch.float32, device=dev)
            off = 0
            for p in params:
                n = p.numel()
                flat[off:off + n].copy_(p.data.reshape(-1).float())
                p.data = flat[off:off + n].view(p.shape)
                off += n
            self._pflat = flat
            self._gflat = torch.zeros(total, dtype=torch.float32, device=dev)
            self._pack_version = None
            self._plans = {}
        return params

    # -- optional per-kernel-family timing (bench.py roofline): events on the launch stream
    profile = None

    profile_detail = False
    _cur_op = ""

    def _pb(self, fam, flop=0.0, nbytes=0.0, flop_exec=None):
        """flop: ALGORITHMIC flops of the launch(es) (the reference's 3x3 convolution); flop_exec: the multiply-adds the kernels
        actually execute when that differs (sub-pixel decoder conv1: 16 instead of 36 taps per low-resolution pixel and up-sampled
        channel), both before the split's products-per-multiply factor"""
        if self.profile is None:
            return None
        if self.profile_detail:
            fam = f"{self._cur_op}|{fam}"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        return (fam, flop, e0, e1, nbytes, flop if flop_exec is None else flop_exec)

    def _pe(self, tok):
        if tok is not None:
            tok[3].record()
            self.profile.setdefault(tok[0], []).append(tok)

    def collect_profile(self):
        torch.cuda.synchronize()
        out = {}
        for fam, toks in (self.profile or {}).items():
            out[fam] = {"ms": sum(t[2].elapsed_time(t[3]) for t in toks), "flop": sum(t[1] for t in toks), "n": len(toks),
                        "bytes": sum(t[4] for t in toks), "flop_exec": sum(t[5] for t in toks)}
        return out

    _stat_epoch = 0      # bumped whenever parameters / running statistics change through raw pointers (torch's _version does not see those)

    def mark_parameters_changed(self):
        """Call after modifying parameters through raw pointers (fused Adam): packed filters and cached inference constants are stale."""
        self._pack_version = None
        self._stat_epoch += 1

    def flat_parameters(self):
        self._ensure_flat()
        return self._pflat

    def flat_grads(self):
        self._ensure_flat()
        return self._gflat

    def _grad_view(self, p):
        off = (p.data_ptr() - self._pflat.data_ptr()) // 4
        return self._gflat[off:off + p.numel()].view(p.shape)

    # ------------------------------------------------------------------------------------------
    class _Plan:
        """buffers and kernel routes of one input shape (callers may hang scratch of their own on it: loss_acc, reg_work)"""

        def __init__(self, N, H, W, route_key):
            self.N, self.H, self.W, self.route_key = N, H, W, route_key
            self.routes, self.irt, self.irt_of_dw, self.irb = {}, {}, {}, {}      # _route_table; irt_of_dw: depthwise op -> expand op
            self.buf, self.grad, self.cst, self.cstb = {}, {}, {}, {}
            self.stats_v, self.bsums_v, self.srows, self.brows, self.irt_rows = {}, {}, {}, {}, {}
            self.bn_scratch = self.fin_amax = self.act_amax = self.classes = self.x_cst = self.head = None
            self.fin_slot, self.act_slot = {}, {}
            self.n_eval = self.generation = 0
            self.training, self.eval_cst_key = False, None
            # backward (need_grad)
            self.has_grad = False
            self.irt_esums, self.irt_work, self.pw_part, self.dwrows, self.dwsums = {}, {}, {}, {}, {}
            self.ws = self.spw_ws = self.spw_skip = self.up_tmp = self.dw_acc = self.gmax = self.dlogits = None
            self.pw_table, self.dw_cast_table = {}, {}      # device descriptor tables of the batched reduction / cast launches

    def _route_key(self):
        """everything a plan's routes are derived from besides its shape.  _get_plan rebuilds a plan whose key differs and _pack_all repacks
        on the same change: a precision switch (check_split_range) never meets rows, workspaces or layouts sized for other kernels."""
        return (self.split_bf16, self._terms, self.fuse_irt, _PW3, _IRT, _IRB, _SP)

    def _route_table(self, N, H, W):
        """The kernel choices at one input shape and the current precision, no device needed: (routes {pointwise / 3x3 op: _Routes},
        irt {expand op: depthwise op} -- inverted-residual blocks whose expansion + depthwise pair runs fused in TRAINING --,
        irb {expand op: (depthwise op, project op, add op or None)} -- blocks that run as one launch in INFERENCE)"""
        split, terms = self.split_bf16, self._terms
        routes, irt, irb = {}, {}, {}
        for i, L in self._layers.items():
            o = self._ops[i]["out"]
            a = (L, N, H >> o.shift, W >> o.shift, split, terms)
            routes[i] = _Routes(_fwd_route(*a), _dgrad_route(*a), _wgrad_route(*a))
        for i_e, (i_dw, i_pr, stride) in self._ir_blocks.items():
            cv_e, cv_p, tin = self._ops[i_e]["conv"], self._ops[i_pr]["conv"], self._ops[i_e]["ins"][0]
            if tin.kind == "input":
                continue
            Hi, Wi = H >> tin.shift, W >> tin.shift
            if self.fuse_irt and _use_irt(N, cv_e.in_channels, cv_e.out_channels, Hi, Wi, stride):
                irt[i_e] = i_dw
            if _use_irb(N, cv_e.in_channels, cv_e.out_channels, cv_p.out_channels, Hi, Wi, stride):
                i_add = i_pr + 1 if (i_pr + 1 < len(self._ops) and self._ops[i_pr + 1]["type"] == "add"
                                     and self._ops[i_pr + 1]["ins"][1] is self._ops[i_pr]["out"]) else None
                irb[i_e] = (i_dw, i_pr, i_add)
        return routes, irt, irb

    def kernel_table(self, N, H, W, training=True):
        """Which kernel runs each op's passes at this shape and the current precision, in walk order: a list of {"op": output tensor,
        "type", "fwd"} plus, for training, "dgrad" and "wgrad" (None: the op has no such pass).  Pointwise and 3x3 layers carry the
        names of their routes (_fwd_route, _dgrad_route, _wgrad_route), ops inside a fused block "irt" (training block; its forward
        also serves inference) or "irb" (inference block), every other op its type.  Needs no device."""
        routes, irt, irb = self._route_table(N, H, W)
        fused = {}
        if not training:
            fused.update((k, "irb") for i_e, members in irb.items() if i_e not in irt for k in (i_e,) + members if k is not None)
        for i_e, i_dw in irt.items():
            fused[i_e] = fused[i_dw] = "irt"
        table = []
        for i, op in enumerate(self._ops):
            r, ty = routes.get(i), op["type"]
            row = {"op": op["out"].name, "type": ty, "fwd": fused.get(i) or (r.fwd.kernel if r else ty)}
            if training:
                row["dgrad"] = fused.get(i) or (r.dgrad.kernel if r else None if ty == "stem" else ty)
                row["wgrad"] = fused.get(i) or (r.wgrad.kernel + ("+" + r.wgrad.skip.kernel if r.wgrad.skip else "") if r else None if ty == "add" else ty)
            table.append(row)
        return table

    def _get_plan(self, N, H, W, need_grad, want_logits=True, want_classes=None):
        """want_logits=False (predict_classes): a plan created by this call gets no logits buffer; the first call that wants one adds it.
        want_classes (default: not want_logits) likewise for the (N, H, W) class buffer, which predict_classes_into does without."""
        want_classes = (not want_logits) if want_classes is None else want_classes
        key = (N, H, W)
        plan, carry = self._plans.get(key), None
        dev = self._pflat.device
        f32 = dict(dtype=torch.float32, device=dev)
        lib = _lib.load()
        if plan is not None and plan.route_key != self._route_key():
            # other kernels, other buffer sizes: a new plan; the old one's buffers go first, its sticky range records move over
            plan, carry = None, (plan.fin_amax, plan.act_amax, plan.n_eval, plan.generation)
            del self._plans[key]
        if plan is None:
            plan = HyperStarcopUNet._Plan(N, H, W, self._route_key())
            plan.routes, plan.irt, plan.irb = self._route_table(N, H, W)
            plan.irt_of_dw = {i_dw: i_e for i_e, i_dw in plan.irt.items()}
            for i_e, i_dw in plan.irt.items():
                tin, stride = self._ops[i_e]["ins"][0], self._ir_blocks[i_e][2]
                for which, t in enumerate((self._ops[i_e]["out"], self._ops[i_dw]["out"])):
                    plan.irt_rows[t.name] = lib.sc_irt_rows(which, N, H >> tin.shift, W >> tin.shift, stride)
            irt_e = {self._ops[i]["out"].name for i in plan.irt}
            for i, op in enumerate(self._ops):
                t = op["out"]
                if t.kind != "input" and t.name not in plan.buf and t.name not in irt_e and t.name != "logits":      # (a fused block's expanded tensor exists
                    plan.buf[t.name] = torch.empty((N, t.C, H >> t.shift, W >> t.shift), **f32)     #  only in inference: _forward_impl)
                if t.bn is not None:
                    Ho, Wo = H >> t.shift, W >> t.shift
                    # per-work-group partial rows [rows][C][2] (plain stores; summed in fp64 by the finalize kernels)
                    rows = plan.routes[i].fwd.rows if i in plan.routes else lib.sc_stat_rows({"stem": STAT_STEM, "dw": STAT_DW}[op["type"]], N, Ho, Wo)
                    plan.srows[t.name] = max(rows, plan.irt_rows.get(t.name, 0))
                    plan.brows[t.name] = lib.sc_stat_rows(STAT_BNBWD, N, Ho, Wo)
                    plan.stats_v[t.name] = torch.empty(plan.srows[t.name] * t.C * 2, **f32)
                    plan.cst[t.name] = torch.zeros((t.C, SC_CST), **f32)
                    plan.cstb[t.name] = torch.zeros((t.C, SC_CST), **f32)
            # the filter layouts the routes of this plan name (sticky over all plans of the network).  The two 1x1 filters of a fused
            # inference block are read in the PW3 layout whatever their own routes are ("pfi", packed for inference forwards only)
            for i, r in plan.routes.items():
                named = {r.fwd.layout, r.dgrad.launches[0][1]}
                if self._layers[i].type == "pw" and not named <= self._pw_need.setdefault(i, set()):
                    self._pw_need[i] |= named
                    self._pack_version, self._pack_tables = None, {}
            for i_e, (i_dw, i_pr, i_add) in plan.irb.items():
                if not {i_e, i_pr} <= self._irb_layers:
                    self._irb_layers.update((i_e, i_pr))
                    self._pack_version, self._pack_tables = None, {}
            fins = [t.name for t in self._tensors.values() if t.kind == "fin" and t.name != "logits"]
            plan.bn_scratch = torch.empty(64 * 2 * max(t.C for t in self._tensors.values()), dtype=torch.float64, device=dev)   # sc_bn_finalize: coalesced pre-reduction of many-row statistics
            plan.fin_slot = {n: i for i, n in enumerate(fins)}
            plan.fin_amax = torch.zeros(len(fins), **f32)        # running max |value| of each residual sum (never lowered)
            raw_feed = self._split_feeders()[0]
            plan.act_slot = {n: i for i, n in enumerate(raw_feed)}
            plan.act_amax = torch.zeros(max(len(raw_feed), 1), **f32)   # sticky max |BN output| of the split kernels' BatchNorm-fed inputs
            if carry is not None:
                plan.fin_amax, plan.act_amax, plan.n_eval, plan.generation = carry
            self._plans[key] = plan
        if want_logits and "logits" not in plan.buf:
            plan.buf["logits"] = torch.empty((N, self.classes, H, W), dtype=torch.float32, device=dev)
        if want_classes and plan.classes is None:
            plan.classes = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
        if need_grad and not plan.has_grad:
            self._size_backward(plan)
        return plan

    def _size_backward(self, plan):
        """gradient buffers and the workspaces of the backward kernels the plan's routes name"""
        lib = _lib.load()
        N, H, W = plan.N, plan.H, plan.W
        dev = self._pflat.device
        f32 = dict(dtype=torch.float32, device=dev)
        irt_e = {self._ops[i]["out"].name for i in plan.irt}
        for i_e in plan.irt:
            cv, tin, te = self._ops[i_e]["conv"], self._ops[i_e]["ins"][0], self._ops[i_e]["out"]
            Hi, Wi = H >> tin.shift, W >> tin.shift
            plan.irt_esums[te.name] = torch.empty(lib.sc_irt_bwd_rows(N, cv.out_channels, Hi, Wi) * cv.out_channels * 2, dtype=torch.float64, device=dev)
            plan.irt_work[te.name] = torch.empty(lib.sc_irt_bwd_workspace_floats(N, cv.in_channels, cv.out_channels, Hi, Wi), **f32)
        # ws: K-slice partials of the weight gradients that reduce in their own launch.  Pointwise weight gradients keep theirs in
        # buffers of their own (pw_part) until ONE batched reduction at the end of the backward pass (sc_wgrad_reduce_batch) instead of
        # 2-3 dependent few-microsecond launches per layer.  Decoder conv1 weight gradients as box-sum GEMMs (conv_spw.hip): box-sum
        # planes, split source, K-slice partials (spw_b); the skip channels' dense gradient before it is scattered into its columns (spw_sk)
        ws = up = n_dw = spw_b = spw_sk = 0
        for i, op in enumerate(self._ops):
            o, conv, ty = op["out"], op.get("conv"), op["type"]
            Ho, Wo = H >> o.shift, W >> o.shift
            if ty != "head" and o.kind != "fin" and o.name not in irt_e:
                plan.grad[o.name] = torch.empty((N, o.C, Ho, Wo), **f32)
            if ty == "add":
                plan.grad[o.name] = torch.empty((N, o.C, Ho, Wo), **f32)
            if i in plan.routes:
                L, r = self._layers[i], plan.routes[i]
                # ws holds the fp32-MFMA and split kernels' partials of every layer whatever the precision routes it to (so that a
                # precision switch finds the capacity it had), and the routed kernel's
                ws = max(ws, _wgrad_floats("mfma", N, Ho, Wo, L.Cout, L.Cin, L.ks), _wgrad_floats("bx3", N, Ho, Wo, L.Cout, L.Cin, 3) if L.ks == 3 else 0)
                if r.wgrad.kernel == "spw":
                    spw_b = max(spw_b, lib.sc_sp_wgrad_workspace_bytes(N, Ho, Wo, L.Cout, L.Cup))
                    if r.wgrad.skip:
                        spw_sk = max(spw_sk, L.Cout * L.Csk * 9)
                        ws = max(ws, _wgrad_floats(r.wgrad.skip.kernel, N, Ho, Wo, L.Cout, L.Csk, 3))
                elif ty == "pw" and i not in plan.irt:
                    plan.pw_part[i] = torch.empty(_wgrad_floats(r.wgrad.kernel, N, Ho, Wo, L.Cout, L.Cin, 1), **f32)
                else:       # (a fused block's expansion, walked on its own by only_ops, reduces in its own launch on the fp32 MFMA)
                    ws = max(ws, _wgrad_floats(r.wgrad.kernel if ty == "conv3" else "mfma", N, Ho, Wo, L.Cout, L.Cin, L.ks))
                if r.dgrad.launches[0][3] == 2:
                    up = max(up, N * L.Cup * Ho * Wo)
            elif ty == "stem":
                ws = max(ws, lib.sc_stem_wgrad_workspace_floats(N, conv.in_channels, H, W))
            elif ty == "head":
                ws = max(ws, lib.sc_head_wgrad_workspace_floats(N, conv.in_channels, Ho, Wo))
            elif ty == "dw":
                n_dw += conv.out_channels * 9
                ti = op["ins"][0]
                if ti.bn is not None and ti.name not in irt_e:      # its BatchNorm-backward sums come out of the fused depthwise backward
                    plan.dwrows[ti.name] = lib.sc_stat_rows(STAT_DW, N, H >> ti.shift, W >> ti.shift)
                    plan.dwsums[ti.name] = torch.empty(plan.dwrows[ti.name] * ti.C * 2, dtype=torch.float64, device=dev)
        plan.spw_ws = torch.empty(spw_b + 256, dtype=torch.uint8, device=dev) if spw_b else None
        plan.spw_skip = torch.empty(spw_sk, **f32) if spw_sk else None
        plan.ws = torch.empty(ws, **f32)
        plan.up_tmp = torch.empty(max(up, 1), **f32)
        plan.dw_acc = torch.zeros(n_dw, dtype=torch.float64, device=dev)
        # one float per BatchNorm'd tensor: max |gamma*invstd * g| of its gradient, the range hint of the fp16-split kernels
        plan.gmax = torch.zeros(len(self._ops) + 1, dtype=torch.float32, device=dev)
        for t in self._tensors.values():
            if t.bn is not None:
                plan.bsums_v[t.name] = torch.empty(plan.brows[t.name] * t.C * 2, dtype=torch.float64, device=dev)
        plan.dlogits = torch.empty((N, 1, H, W), **f32)
        plan.has_grad = True

    # ------------------------------------------------------------------------------------------
    def _wanted_layouts(self, i):
        """the filter layouts _pack_all keeps for layer i: all of a 3x3 layer's (_layouts); of a pointwise layer's what the plans' routes name,
        plus "pfi" (filled by inference forwards only) for a fused inference block's filter that no plan runs on sc_conv1x1_pw3"""
        if self._layers[i].type != "pw":
            return set(_layouts(self._layers[i], self.split_bf16, self._terms))
        need = self._pw_need.get(i, set())
        return need | {"pfi"} if (i in self._irb_layers and "pf" not in need) else need

    def _pack_all(self, need_bwd):
        """(Re)pack conv filters into the MFMA kernels' layouts when the parameters changed."""
        lib = _lib.load()
        split, terms = self.split_bf16, self._terms
        ver = (tuple(p._version for p in self.parameters()), terms, split)    # a precision switch repacks too
        pv = self._pack_version
        need_irb = (not need_bwd) and bool(self._irb_layers)      # the fused inference blocks' PW3 layouts
        if pv is not None and pv[0] == ver and (pv[1] or not need_bwd) and (pv[2] or not need_irb):
            return
        st = stream()
        dev = self._pflat.device
        for i, L in self._layers.items():
            ent = self._wpk.get(i)
            if ent is None or ent["key"] != (dev, split, terms, _SP):
                ent = self._wpk[i] = {"key": (dev, split, terms, _SP), "spec": _layouts(L, split, terms)}
                self._pack_tables = {}
            for name in (self._wanted_layouts(i) if L.type == "pw" else ent["spec"]):
                if name not in ent:
                    ent[name] = torch.empty(ent["spec"][name][0], dtype=torch.float32, device=dev)
                    self._pack_tables = {}
        # one launch for all packs: device-side descriptor table, built once per (need_bwd, parameter storage)
        key = (bool(need_bwd), self._pflat.data_ptr(), terms, need_irb)
        tab = self._pack_tables.get(key)
        if tab is None:
            import numpy as np
            dt = np.dtype([("w", "<u8"), ("wpk", "<u8"), ("Cout", "<i4"), ("Cin", "<i4"), ("ks", "<i4"), ("co_t", "<i4"),
                           ("tflip", "<i4"), ("bx3", "<i4"), ("total", "<u8")])
            # two tables: the layouts the ENCODER's forward reads (pointwise layers, forward direction), and everything else -- the
            # decoder's 3x3 layouts and all backward layouts, most of the work -- which a training step packs on the weight-gradient
            # stream while the encoder runs (see the launches below)
            early, late = [], []
            for i, L in self._layers.items():
                w, ent = self._ops[i]["conv"].weight, self._wpk[i]
                wanted = self._wanted_layouts(i) if L.type == "pw" else ent["spec"]
                for name in _PACK_ORDER:
                    if name not in wanted or (name in _BWD_LAYOUTS and not need_bwd) or (name == "pfi" and not need_irb):
                        continue
                    _, cot, tflip, code = ent["spec"][name]
                    total = lib.sc_pack_work_items(L.Cout, L.Cin, L.ks, cot, tflip, int(code))
                    (early if L.type == "pw" and name in ("f", "pf", "pfi") else late).append(
                        (w.data_ptr(), ent[name].data_ptr(), L.Cout, L.Cin, L.ks, cot, tflip, int(code), total))

            tab = self._pack_tables[key] = tuple(
                _block_table(np.array(rows, dtype=dt).tobytes(), [r[-1] for r in rows], dev) if rows else None for rows in (early, late))
        # launches: the encoder's layouts on the current stream; the rest, in a training step, on the weight-gradient stream behind a
        # device-scope wait (the parameters are final on the current stream) -- the forward walk waits for it before its first 3x3
        # convolution (_forward_impl), i.e. ~0.12 ms of packing leaves the critical path and runs beside the encoder.  Otherwise
        # (inference, no overlap stream, graph capture) on the current stream too.
        self._late_pack_stream = None

        def pack(t, sx):
            check(lib.sc_pack_weights_batch(ptr(t[0]), ptr(t[1]), t[2], t[3], sx))
        if tab[0] is not None:
            pack(tab[0], st)
        if tab[1] is not None and need_bwd and self.overlap_wgrad and not torch.cuda.is_current_stream_capturing():
            sh = C.c_void_p(self._wgrad_stream(torch.cuda.current_stream()).cuda_stream)
            check(lib.sc_stream_wait_stream(sh, st))
            pack(tab[1], sh)
            self._late_pack_stream = sh
        elif tab[1] is not None:
            pack(tab[1], st)
        self._pack_version = (ver, bool(need_bwd), need_irb)

    # ------------------------------------------------------------------------------------------
    def _src_of(self, plan, t, up=0, x_cst=None):
        if t.kind == "input":
            if x_cst is None:
                return make_src(plan.buf["x"], t.C, SRC_RAW)
            return make_src(plan.buf["x"], t.C, SRC_NORM, cst=x_cst)
        if t.kind == "raw":
            return make_src(plan.buf[t.name], t.C, SRC_AFFINE, act=t.act, up=up, cst=plan.cst[t.name])
        return make_src(plan.buf[t.name], t.C, SRC_RAW, up=up)

    def _xbound(self, plan, t):
        """device float >= max |activation| of tensor t as the split convolutions stage it, or None (ReLU6 / input: the default scale
        covers it): BatchNorm-fed tensors -> their slot of plan.act_amax (raised by sc_bn_finalize to the by-construction bound in
        training, by the BatchNorm-backward reductions / the streamed record to the observed maximum), residual sums -> plan.fin_amax
        (recorded by sc_add_srcs_absmax in every forward, before any consumer runs)"""
        if t.kind == "fin" and t.name in plan.fin_slot:
            return C.c_void_p(plan.fin_amax.data_ptr() + 4 * plan.fin_slot[t.name])
        slot = plan.act_slot.get(t.name) if t.kind == "raw" else None
        return C.c_void_p(plan.act_amax.data_ptr() + 4 * slot) if slot is not None else None

    def _dy_src(self, plan, t):
        return make_src(plan.grad[t.name], t.C, SRC_BNBWD, act=t.act, cst=plan.cstb[t.name], aux=plan.buf[t.name])

    def _forward_impl(self, x, x_cst, training, need_grad, _recheck=0, head="logits", mosaic=None):
        """x: (N,C,H,W) fp32 device tensor (raw physical units if x_cst is given, else already normalised).
        head: "logits" -> plan.buf["logits"] (N,K,H,W); "classes" -> plan.classes (N,H,W) uint8 = argmax over K, no logits stored;
        "mosaic" -> the classes of every item's core rectangle into ``mosaic.classes``, see predict_classes_into: neither logits nor
        per-item classes are stored; "probmosaic" -> sigmoid and mask of the cores of the 1-class head into ``mosaic.prob`` /
        ``mosaic.mask``, see predict_masks_into: likewise nothing else is stored.  ``mosaic``: a :class:`HeadMosaic`."""
        if training and (self.classes > self.MAX_TRAIN_CLASSES or self.in_channels > self.MAX_TRAIN_IN_CHANNELS):
            raise NotImplementedError(
                f"HyperStarcopUNet(in_channels={self.in_channels}, classes={self.classes}) runs in eval mode only: training needs two "
                f"kernels that do not exist -- the stem weight gradient above {self.MAX_TRAIN_IN_CHANNELS} input channels "
                f"(sc_stem_conv_wgrad) and the backward of the K-class head (sc_head_conv_bwd is the 1-class head's)")
        _lib.require_device(x)
        lib = _lib.load()
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"HyperStarcopUNet: expected (N,{self.in_channels},H,W) input, got {tuple(x.shape)}")
        N, _, H, W = x.shape
        if H % 32 or W % 32:
            raise RuntimeError(f"Wrong input shape height={H}, width={W}. Expected image height and width "
                               "divisible by 32.")
        self._ensure_flat()
        x = x.contiguous().float()
        plan = self._get_plan(N, H, W, need_grad, want_logits=head == "logits", want_classes=head == "classes")
        plan.buf["x"] = x
        plan.x_cst, plan.head = x_cst, (head, mosaic)
        plan.generation += 1     # activations of an earlier forward of this shape are gone
        self._pack_all(need_grad)
        st = stream()
        # inference: the BatchNorm constants depend only on parameters and running statistics -- 62 five-microsecond launches of the
        # dependency chain (a tenth of a batch-16 forward) are skipped while neither has changed since this plan last computed them
        eval_key = None if training else (tuple(p._version for p in self.parameters()), tuple(b._version for b in self.buffers()), self._stat_epoch)
        # (never while a hipGraph is being captured: the graph must contain the finalize launches, or its replays would keep the
        # constants of capture time whatever happens to the parameters afterwards.  Writers that bypass torch's version counters --
        # a broadcast into the flat buffer, raw-pointer updates -- must call mark_parameters_changed().)
        eval_cst_ok = eval_key is not None and plan.eval_cst_key == eval_key and not torch.cuda.is_current_stream_capturing()
        if training:
            self._stat_epoch += 1            # running statistics are about to be updated through raw pointers
            plan.eval_cst_key = None
        if not training and not eval_cst_ok:
            # inference: every BatchNorm's constants up front (they do not depend on the data), so that a fused block can use the
            # constants of tensors it never materialises
            for t in self._tensors.values():
                if t.bn is not None:
                    self._bn_finalize(plan, t, None, 0, 1.0, None, st)
        skip = set()
        for i, op in enumerate(self._ops):
            if i in skip:
                continue
            if i in plan.irt:
                self._irt_forward(plan, i, training, st)
                skip.add(plan.irt[i])
                continue
            if not training and i in plan.irb:
                skip.update(self._fwd_irb(plan, i, st))
                continue
            ty, o = op["type"], op["out"]
            stats = ptr(plan.stats_v[o.name]) if (training and o.bn is not None) else None
            self._cur_op = o.name + ":fwd"
            tok = self._fwd_profile(plan, i)
            self._FWD[ty](self, plan, i, stats, st)
            self._pe(tok)
            if o.bn is not None and training:
                self._bn_finalize(plan, o, stats, plan.srows[o.name], float(N * (H >> o.shift) * (W >> o.shift)), self._xbound(plan, o), st)
        if self._late_pack_stream is not None:      # (no 3x3 layer ran: still order the main stream after the pack)
            check(lib.sc_stream_wait_stream(st, self._late_pack_stream))
            self._late_pack_stream = None
        if training:      # one multi-tensor launch for the 62 step counters
            torch._foreach_add_(self._nbt_list(), 1)
        else:
            plan.eval_cst_key = eval_key
        plan.training = training
        if not training and self._inference_range_clamped(plan, _recheck):
            return self._forward_impl(x, x_cst, training, need_grad, _recheck=_recheck + 1, head=head, mosaic=mosaic)
        return plan

    def _fwd_profile(self, plan, i):
        if self.profile is None:
            return None
        op = self._ops[i]
        if i not in plan.routes:
            return self._pb({"stem": "k_stem_*", "dw": "k_dw_*", "head": "k_head_*", "add": "elementwise/bn"}[op["type"]])
        L, o, route = self._layers[i], op["out"], plan.routes[i].fwd
        N, Ho, Wo = plan.N, plan.H >> o.shift, plan.W >> o.shift
        src_elems = sum(t.C * (plan.H >> t.shift) * (plan.W >> t.shift) for t in op["ins"])
        fl = 2.0 * N * Ho * Wo * L.Cout * L.Cin * L.ks ** 2
        # sub-pixel form, per low-resolution pixel: 16 slots per up-sampled channel, 16 per (skip channel, parity)
        fle = 2.0 * N * (Ho // 2) * (Wo // 2) * 16 * (-(-L.Cout // 32) * 32) * (L.Cup + 4 * L.Csk) if route.kernel == "sp" else None
        return self._pb(route.family, fl, 4.0 * (N * src_elems + N * o.C * Ho * Wo + op["conv"].weight.numel()), fle)


    def _fwd_irb(self, plan, i, st):
        """inference: the whole inverted-residual block in one launch (conv_irb.hip); returns the depthwise, projection and add ops
        it covers"""
        i_dw, i_pr, i_add = plan.irb[i]
        op, op_d, op_p = self._ops[i], self._ops[i_dw], self._ops[i_pr]
        tin, te, td, tp = op["ins"][0], op["out"], op_d["out"], op_p["out"]
        a = sc_irb_args()
        a.x = self._src_of(plan, tin)
        # (the PW3 layout of a filter: the layer's own where some plan runs it on sc_conv1x1_pw3, else the block's: _wanted_layouts)
        a.wpk_expand = self._wpk[i]["pf" if "pf" in self._pw_need[i] else "pfi"].data_ptr()
        a.wpk_project = self._wpk[i_pr]["pf" if "pf" in self._pw_need[i_pr] else "pfi"].data_ptr()
        a.cst_expand = plan.cst[te.name].data_ptr()
        a.w_dw, a.cst_dw = op_d["conv"].weight.data_ptr(), plan.cst[td.name].data_ptr()
        a.N, a.Cin, a.hidden, a.Cout = plan.N, op["conv"].in_channels, op["conv"].out_channels, op_p["conv"].out_channels
        a.H, a.W, a.stride = plan.H >> tin.shift, plan.W >> tin.shift, self._ir_blocks[i][2]
        if i_add is not None:
            tz = self._ops[i_add]["out"]
            a.residual, a.cst_project = 1, plan.cst[tp.name].data_ptr()
            a.out = plan.buf[tz.name].data_ptr()
            a.z_absmax = plan.fin_amax.data_ptr() + 4 * plan.fin_slot[tz.name]
        else:
            a.residual, a.cst_project, a.z_absmax = 0, None, None
            a.out = plan.buf[tp.name].data_ptr()
        self._cur_op = tp.name + ":fwd"
        tok = self._pb("k_irb (fused block, eval)")
        check(_lib.load().sc_irb_eval(C.byref(a), st))
        self._pe(tok)
        return [k for k in plan.irb[i] if k is not None]

    def _fwd_stem(self, plan, i, stats, st):
        op = self._ops[i]
        conv = op["conv"]
        s = self._src_of(plan, op["ins"][0], x_cst=plan.x_cst)
        check(_lib.load().sc_stem_conv_fwd(C.byref(s), ptr(conv.weight), ptr(plan.buf[op["out"].name]), plan.N, conv.in_channels,
                                           plan.H, plan.W, stats, st))

    def _fwd_dw(self, plan, i, stats, st):
        op = self._ops[i]
        tin, o = op["ins"][0], op["out"]
        s = self._src_of(plan, tin)
        check(_lib.load().sc_dwconv3x3_fwd(C.byref(s), ptr(op["conv"].weight), ptr(plan.buf[o.name]), plan.N, o.C,
                                           plan.H >> tin.shift, plan.W >> tin.shift, op["stride"], stats, st))

    def _fwd_conv(self, plan, i, stats, st):
        """a pointwise or 3x3 layer on the kernel its forward route names"""
        lib = _lib.load()
        op, L, route = self._ops[i], self._layers[i], plan.routes[i].fwd
        ins, o = op["ins"], op["out"]
        if L.type == "conv3" and self._late_pack_stream is not None:      # the decoder's filter layouts were packed beside the encoder
            check(lib.sc_stream_wait_stream(st, self._late_pack_stream))
            self._late_pack_stream = None
        a = sc_conv_args()
        a.nsrc = len(ins)
        a.src[0] = self._src_of(plan, ins[0], up=1 if L.up else 0)
        if len(ins) == 2:
            a.src[1] = self._src_of(plan, ins[1])
        a.wpk = self._wpk[i][route.layout].data_ptr()
        a.N, a.H, a.W, a.Cout = plan.N, plan.H >> o.shift, plan.W >> o.shift, o.C
        a.ks, a.co_t = L.ks, route.cot
        a.out0 = plan.buf[o.name].data_ptr(); a.out1 = None
        a.csplit, a.accum0, a.accum1 = o.C, 0, 0
        a.add0 = None; a.add1 = None
        a.stats = plan.stats_v[o.name].data_ptr() if stats is not None else None
        a.terms = self._terms[0]
        if L.type == "conv3":
            for k_, t_ in enumerate(ins):
                a.xbound[k_] = self._xbound(plan, t_)
        check(getattr(lib, route.entry)(C.byref(a), st))


    def _fwd_add(self, plan, i, stats, st):
        op = self._ops[i]
        o = op["out"]
        sa = self._src_of(plan, op["ins"][0])
        sb = self._src_of(plan, op["ins"][1])
        # the residual sums are the only inputs of a split convolution that no BatchNorm bounds (the skips taken after
        # features.3/6/13): their max |value| is recorded for split_range_report
        check(_lib.load().sc_add_srcs_absmax(C.byref(sa), C.byref(sb), ptr(plan.buf[o.name]), plan.N, o.C,
                                             (plan.H >> o.shift) * (plan.W >> o.shift),
                                             plan.fin_amax.data_ptr() + 4 * plan.fin_slot[o.name], st))

    def _fwd_head(self, plan, i, stats, st):
        lib, (head, mosaic) = _lib.load(), plan.head
        conv, o, op = self._ops[i]["conv"], self._ops[i]["out"], self._ops[i]
        N, Ho, Wo = plan.N, plan.H >> o.shift, plan.W >> o.shift
        s = self._src_of(plan, op["ins"][0])
        if head == "mosaic":
            mos = mosaic.classes
            check(lib.sc_head_conv_fwd_k_mosaic(C.byref(s), ptr(conv.weight), ptr(conv.bias), ptr(mos), mos.shape[0], mos.shape[1],
                                                mos.stride(0), mosaic.win, mosaic.win_host,
                                                N, conv.in_channels, self.classes, Ho, Wo, st))
        elif head == "probmosaic":
            prob, mask, valid = mosaic.prob, mosaic.mask, mosaic.valid
            ref = prob if prob is not None else mask
            check(lib.sc_head_conv_fwd_mosaic_prob(
                C.byref(s), ptr(conv.weight), ptr(conv.bias), ptr(prob), prob.stride(0) if prob is not None else 0,
                ptr(mask), mask.stride(0) if mask is not None else 0, ref.shape[0], ref.shape[1],
                ptr(valid), valid.stride(0) if valid is not None else 0, valid.stride(1) if valid is not None else 0,
                mosaic.fill_bits, mosaic.nodata, mosaic.win, mosaic.win_host,
                N, conv.in_channels, Ho, Wo, st))
        elif self.classes == 1 and head == "logits":
            check(lib.sc_head_conv_fwd(C.byref(s), ptr(conv.weight), ptr(conv.bias), ptr(plan.buf[o.name]),
                                       N, conv.in_channels, Ho, Wo, st))
        else:       # K classes and / or the fused argmax: exactly one of the two outputs
            check(lib.sc_head_conv_fwd_k(C.byref(s), ptr(conv.weight), ptr(conv.bias),
                                         ptr(plan.buf[o.name]) if head == "logits" else None,
                                         ptr(plan.classes) if head == "classes" else None,
                                         N, conv.in_channels, self.classes, Ho, Wo, st))
        plan.head = None      # (the caller's mosaics are not the plan's to keep)

    _FWD = {"stem": _fwd_stem, "dw": _fwd_dw, "pw": _fwd_conv, "conv3": _fwd_conv, "add": _fwd_add, "head": _fwd_head}

    def _inference_range_clamped(self, plan, _recheck):
        """The range check of an inference forward: True if the forward has to be redone with adapted operand scales."""
        if not (self.precision == "fp32" and self.range_check_every and plan.act_slot
                and not torch.cuda.is_current_stream_capturing()):
            return False
        # inference: BatchNorm uses running statistics, so no bound of its output exists before the data has flowed.  The split
        # convolutions scale their operands from the sticky records of the observed maxima (plan.act_amax); at the check cadence
        # (first forward of a shape included) the handful of tensors is streamed once more and, if a value was beyond what the
        # scale in force during THIS forward could carry (it was clamped), the forward is redone -- the records are updated by
        # then, so the scales adapt; the precision mode does not change.  (Training needs none of this: sc_bn_finalize leaves
        # the by-construction bound before any consumer runs.)
        plan.n_eval += 1
        if not (_recheck or plan.n_eval % self.range_check_every == 1 or self.range_check_every == 1):
            return False
        before = plan.act_amax.clone()
        self._record_activation_range(plan)
        used = torch.where(before * 2 > self.FP16_MAX_ACT,
                           torch.exp2(torch.floor(torch.log2(self.FP16_MAX_ACT / before.clamp_min(1e-30)))), torch.full_like(before, 2.0))
        if not bool((plan.act_amax * used > 2 * self.FP16_MAX_ACT).any()):
            return False
        import warnings
        worst = float((plan.act_amax * used).max()) / 2.0
        if _recheck < 6:
            if _recheck == 0:
                self._inference_clamped += 1
                warnings.warn(f"HyperStarcopUNet (inference, precision='fp32'): an activation of {worst:.4g} (in units of the "
                              f"operand scale in force) exceeded the fp16 range of the split convolutions "
                              f"({self.FP16_MAX_ACT:g}) and was clamped; the forward is redone with the adapted scale.  "
                              f"Forwards between two checks (range_check_every={self.range_check_every}) are not re-examined: "
                              f"set range_check_every=1 for data of unknown range")
            return True
        self._inference_unrepaired += 1
        warnings.warn(f"HyperStarcopUNet (inference, precision='fp32'): activations still outside the fp16 range after 6 "
                      f"re-runs with adapted scales ({worst:.4g}); the returned logits carry operands clamped to "
                      f"+-65504/scale.  split_range_report()['ok'] is now False; use precision='fp32-x3' for this input")
        return False

    def _irt_args(self, plan, i_e):
        i_dw = plan.irt[i_e]
        op, cv_d = self._ops[i_e], self._ops[i_dw]["conv"]
        cv, tin, te = op["conv"], op["ins"][0], op["out"]
        a = sc_irt_args()
        a.x = self._src_of(plan, tin)
        a.w_expand, a.w_dw, a.cst_expand = cv.weight.data_ptr(), cv_d.weight.data_ptr(), plan.cst[te.name].data_ptr()
        a.N, a.Cin, a.hidden = plan.N, cv.in_channels, cv.out_channels
        a.H, a.W, a.stride = plan.H >> tin.shift, plan.W >> tin.shift, self._ops[i_dw]["stride"]
        return a

    def _bn_finalize(self, plan, t, stats, rows, count, xbound, st):
        """BatchNorm constants of tensor t: from the partial statistics rows of its producer (training; updates the running
        statistics), or with stats None from the running statistics (inference)"""
        bn, train = t.bn, stats is not None
        check(_lib.load().sc_bn_finalize(stats, rows, count, ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var),
                                         float(bn.momentum), float(bn.eps), int(train), ptr(plan.cst[t.name]), t.C,
                                         ptr(plan.bn_scratch) if train else None, xbound, st))

    def _irt_forward(self, plan, i_e, training, st):
        """forward of a fused block.  Training: statistics of the (never stored) expanded tensor -> its BatchNorm constants -> raw
        depthwise output + statistics -> the depthwise BatchNorm's constants (conv_irt.hip).  Inference: the same fused forward with
        the running-statistics constants (computed up front, _forward_impl), no statistics"""
        lib = _lib.load()
        te, td = self._ops[i_e]["out"], self._ops[plan.irt[i_e]]["out"]
        a = self._irt_args(plan, i_e)
        if training:
            self._cur_op = te.name + ":fwd"
            tok = self._pb("k_irt_* (fused expand+dw)")
            check(lib.sc_irt_expand_stats(C.byref(a), ptr(plan.stats_v[te.name]), st))
            self._pe(tok)
            self._bn_finalize(plan, te, ptr(plan.stats_v[te.name]), plan.irt_rows[te.name], float(plan.N * a.H * a.W), None, st)
        self._cur_op = td.name + ":fwd"
        tok = self._pb("k_irt_* (fused expand+dw)")
        check(lib.sc_irt_fwd(C.byref(a), ptr(plan.buf[td.name]), ptr(plan.stats_v[td.name]) if training else None, st))
        self._pe(tok)
        if training:
            self._bn_finalize(plan, td, ptr(plan.stats_v[td.name]), plan.irt_rows[td.name],
                              float(plan.N * (plan.H >> td.shift) * (plan.W >> td.shift)), None, st)

    def _nbt_list(self):
        if self._nbt is None or self._nbt[0].device != self._pflat.device:
            self._nbt = [t.bn.num_batches_tracked for t in self._tensors.values() if t.bn is not None]
        return self._nbt

    # weight gradients are off the critical path (nothing in the backward pass consumes them): they run on a second
    # HIP stream, forked after each layer's BatchNorm-backward constants and joined before the optimiser, so they fill
    # the CUs the small dgrad / reduce kernels of the dependency chain leave idle.
    overlap_wgrad = True
    fuse_irt = _IRT != "0"      # training: expansion + depthwise of the stride-2 blocks the rule picks without the 6x tensor (conv_irt.hip)
    split_bf16 = True        # 3x3 convs with >= 32 output channels on the 16-bit matrix cores (False: everything on the fp32 MFMA)
    bn_small_max = 16384     # BatchNorm backward in one launch (block per channel) when a channel has at most this many elements
    # Arithmetic of the 3x3 convolutions with >= 32 channels (conv_bx3.hip): every fp32 operand is split exactly into a few
    # 16-bit terms while it is staged and the leading products are accumulated in fp32 on the matrix cores.
    #   "fp32"       two fp16 terms per operand (22 significand bits, exact power-of-two range scaling), three products:
    #                error below the fp32 accumulation error of the reduction -- the parity / bench default
    #   "fp32-x3"    three bf16 terms, six products (error = one fp32 rounding, fp32's full exponent range; 11 % slower)
    #   "fp32-bwd2"  three bf16 terms forward, two in dgrad/wgrad (operand error 2^-18; logits identical to "fp32-x3")
    #   "fp32-2"     two bf16 terms everywhere (logits ~2e-5 from the oracle, inside the 1e-4 contract with less margin)
    #   "bf16"       one bf16 term: plain bf16 matrix math, fp32 accumulation and fp32 tensors in HBM (BASELINE configs[3])
    precision = "fp32"
    _TERMS = {"fp32": (TERMS_F16X2, TERMS_F16X2), "fp32-x3": (3, 3), "fp32-bwd2": (3, 2), "fp32-2": (2, 2), "bf16": (1, 1)}

    @property
    def _terms(self):
        """(forward, backward) bf16 terms per operand"""
        if self.precision not in self._TERMS:
            raise ValueError(f"precision must be one of {sorted(self._TERMS)} (got {self.precision!r})")
        return self._TERMS[self.precision]
    _side_stream = None
    _late_pack_stream = None

    def _backward_impl(self, plan, dlogits, on_tail_ready=None, only_ops=None, exchange_follows=None):
        """Fills the flat gradient buffer from dL/dlogits.  Needs the plan of a training-mode forward.

        ``only_ops`` (a list of indices into ``self._ops``; parity tests): run the backward of just these ops, each from whatever
        ``plan.grad[out]`` / ``plan.buf`` / ``plan.cst`` hold -- the teacher-forced per-layer gates feed every layer the oracle's
        activations and upstream gradient through exactly the launches a training step makes for it.

        ``exchange_follows``: a gradient exchange (any collective that may leave the device) reads the flat gradient buffer right
        after this call -- the final join of the weight-gradient stream then uses a default (system-fence) event; default: whether
        ``on_tail_ready`` is given.  Callers with a non-bucketed exchange (a grad_sync object without begin()) pass True.

        ``on_tail_ready(lo, hi)`` is called once, when the walk leaves the decoder: every gradient of the decoder and head
        parameters (flat range [lo, hi), two thirds of the buffer) has been queued, so a data-parallel caller can start
        reducing that bucket while the encoder's backward still runs.  It is called with the weight-gradient stream
        current (ordered after the main stream), i.e. a collective issued inside it waits for both."""
        lib = _lib.load()
        w = _BwdWalk(plan, stream(), dlogits.contiguous(), self._terms[1] == TERMS_F16X2)
        main = torch.cuda.current_stream()
        if self.overlap_wgrad:
            w.side = self._wgrad_stream(main)
            w.sd = C.c_void_p(w.side.cuda_stream)      # raw handle, looked up once per walk
        if not plan.training:
            raise RuntimeError("HyperStarcopUNet.backward: gradients need a train-mode forward (BatchNorm batch "
                               "statistics); call .train() first")
        if plan.route_key != self._route_key():
            raise RuntimeError("HyperStarcopUNet.backward: precision or a kernel switch changed since this plan's forward: run it again")
        plan.dw_acc.zero_()
        if w.half_bwd:
            plan.gmax.zero_()
        tail_lo = self._tail_lo
        tail_pending = on_tail_ready is not None
        for i in (range(len(self._ops) - 1, -1, -1) if only_ops is None else only_ops):
            if i in w.irt_done:
                continue
            op = self._ops[i]
            ty, o, conv = op["type"], op["out"], op.get("conv")
            if tail_pending and (conv is None or (conv.weight.data_ptr() - self._pflat.data_ptr()) // 4 < tail_lo):
                tail_pending = False            # first encoder op: the decoder/head bucket is complete
                if w.side is not None:
                    w.side.wait_stream(main)      # (a default event: the collective that starts here may leave the device)
                    with torch.cuda.stream(w.side):
                        on_tail_ready(tail_lo, self._gflat.numel())
                else:
                    on_tail_ready(tail_lo, self._gflat.numel())
            self._cur_op = o.name + ":bwd"
            if ty == "head":
                self._bwd_head(w, i)
                continue
            if ty == "add":
                # z = a + BN(p): dL/d(BN(p)) = dL/dz (alias); a receives dL/dz through its expand-conv dgrad epilogue
                p_t = op["ins"][1]
                plan.grad[p_t.name] = plan.grad[o.name]
                w.written.add(p_t.name)
                continue
            tok = self._pb("elementwise/bn")
            self._bn_backward(w, o, i if (w.half_bwd and ty == "conv3") else None)
            self._pe(tok)
            dy = self._dy_src(plan, o)
            if ty == "stem":
                self._bwd_stem(w, i, dy)
            elif ty == "dw":
                (self._bwd_irt if i in plan.irt_of_dw else self._bwd_dw)(w, i, dy)
                if i == self._last_dw:
                    self._cast_dw_gradients(w)
            else:
                self._bwd_wgrad(w, i, dy)
                if op["ins"][0].kind != "input":
                    self._bwd_dgrad(w, i, dy)
        self._reduce_pointwise_batch(w)
        self._cast_dw_gradients(w)
        if w.side is not None:
            # join: every weight gradient is in the flat buffer before Adam / all-reduce.  With a gradient exchange to follow
            # (on_tail_ready: the data-parallel path) a default event, otherwise the device-scope one
            if exchange_follows if exchange_follows is not None else on_tail_ready is not None:
                main.wait_stream(w.side)
            else:
                check(lib.sc_stream_wait_stream(w.st, w.sd))

    def _wgrad_stream(self, main):
        if self._side_stream is None or self._side_stream.device != main.device:
            self._side_stream = torch.cuda.Stream(device=main.device)
        return self._side_stream

    def _wgrad_launch(self, w, fn):
        """run fn(stream_handle) on the weight-gradient stream, ordered after everything queued on the main stream.  (One fork per
        launch: serving two to eight launches with one fork -- fewer markers in the main queue -- measured 0.5-2.5 % SLOWER, the
        weight gradients then start too late to fill the gaps of the data-gradient chain.)"""
        if w.side is None:
            fn(w.st)
        else:
            check(_lib.load().sc_stream_wait_stream(w.sd, w.st))      # same-device ordering without the system-scope fence of a default event
            fn(w.sd)       # (every fn launches through the C ABI with the handle it is given: no stream context switch needed)

    def _bn_backward(self, w, t, slot=None):
        lib, plan, st, gv = _lib.load(), w.plan, w.st, self._grad_view
        N, Ho, Wo = plan.N, plan.H >> t.shift, plan.W >> t.shift
        amax = w.gmax_slot[t.name] = plan.gmax.data_ptr() + 4 * slot if slot is not None else None
        if t.name in w.reduced:          # the launch that wrote this gradient left the sums (and raised the range-hint slot)
            self._bn_bwd_finalize(w, t, plan.dwsums[t.name], plan.dwrows[t.name], N * Ho * Wo)
            return
        aslot = plan.act_slot.get(t.name)           # BatchNorm-fed input of a split convolution: sticky max |BN(y)| record
        aact = plan.act_amax.data_ptr() + 4 * aslot if aslot is not None else None
        if N * Ho * Wo <= self.bn_small_max and t.C >= 64:        # low-resolution layers: one launch, one block per channel
            check(lib.sc_bn_bwd_small(ptr(plan.grad[t.name]), ptr(plan.buf[t.name]), ptr(plan.cst[t.name]), t.act, N, t.C,
                                      Ho * Wo, ptr(gv(t.bn.weight)), ptr(gv(t.bn.bias)), ptr(plan.cstb[t.name]), amax, aact, st))
            return
        check(lib.sc_bn_bwd_reduce(ptr(plan.grad[t.name]), ptr(plan.buf[t.name]), ptr(plan.cst[t.name]), t.act,
                                   ptr(plan.bsums_v[t.name]), N, t.C, Ho * Wo, amax, aact, st))
        self._bn_bwd_finalize(w, t, plan.bsums_v[t.name], plan.brows[t.name], N * Ho * Wo)

    def _bn_bwd_finalize(self, w, t, sums, rows, count):
        gv, plan = self._grad_view, w.plan
        check(_lib.load().sc_bn_bwd_finalize(ptr(sums), rows, float(count), ptr(plan.cst[t.name]), ptr(gv(t.bn.weight)), ptr(gv(t.bn.bias)),
                                             ptr(plan.cstb[t.name]), t.C, w.st))

    def _reduce_pointwise_batch(self, w):
        """ONE launch (weight-gradient stream) sums the K-slice partials of every pointwise weight gradient queued so far"""
        if not w.pw_pending:
            return
        lib, plan = _lib.load(), w.plan
        raw = b"".join(bytes(p_) for p_ in w.pw_pending)
        if raw not in plan.pw_table:
            # descriptors are static for a plan, so the device table is built once -- and another one when a descriptor changes
            # (parameters re-flattened / moved, a partial backward of the parity tests); earlier tables stay alive because a
            # launch on the weight-gradient stream may still be reading them
            plan.pw_table[raw] = _block_table(raw, [p_.total for p_ in w.pw_pending], self._pflat.device)
        tab = plan.pw_table[raw]
        tok = self._pb("k_wgrad_mfma<1> (+reduce)")
        self._wgrad_launch(w, lambda sx: check(lib.sc_wgrad_reduce_batch(ptr(tab[0]), ptr(tab[1]), tab[2], tab[3], sx)))
        self._pe(tok)
        w.pw_pending.clear()

    def _cast_dw_gradients(self, w):
        """ONE launch (weight-gradient stream) rounds every depthwise filter gradient accumulated so far to fp32 -- per layer it was
        a 5 us kernel behind its own fork of the weight-gradient stream, i.e. 17 more markers in the main queue per step"""
        if not w.dw_casts:
            return
        lib, plan = _lib.load(), w.plan
        key = tuple(w.dw_casts)
        if key not in plan.dw_cast_table:
            import numpy as np
            arr = np.array([(a, b, n) for a, b, n in w.dw_casts], dtype=np.uint64)
            plan.dw_cast_table[key] = (torch.from_numpy(arr.view(np.uint8).copy()).to(self._pflat.device), len(w.dw_casts))
        tab = plan.dw_cast_table[key]
        self._wgrad_launch(w, lambda sx: check(lib.sc_cast_f64_f32_batch(ptr(tab[0]), tab[1], sx)))
        w.dw_casts.clear()

    def _bwd_head(self, w, i):
        lib, plan, gv = _lib.load(), w.plan, self._grad_view
        op = self._ops[i]
        conv, tin, o = op["conv"], op["ins"][0], op["out"]
        N, Ho, Wo = plan.N, plan.H >> o.shift, plan.W >> o.shift
        s = self._src_of(plan, tin)
        tok = self._pb("k_head_*")
        # one sweep over (dlogits, x) for gin, dW and dbias (sc_head_conv_bwd) -- and, the head being the only consumer
        # of the decoder's last tensor, that tensor's BatchNorm-backward sums and range hint (its raw values stream
        # through the kernel anyway): saves sc_bn_bwd_reduce's pass over 2 x 268 MB at 16 x 512^2
        bns = bna = None
        if tin.bn is not None and tin.kind == "raw" and self._n_cons.get(tin.name, 0) == 1:
            if tin.name not in plan.dwsums:
                plan.dwrows[tin.name] = lib.sc_head_bwd_bn_rows(N, Ho, Wo)
                plan.dwsums[tin.name] = torch.empty(plan.dwrows[tin.name] * tin.C * 2, dtype=torch.float64, device=self._pflat.device)
            bns = ptr(plan.dwsums[tin.name])
            if w.half_bwd:
                bna = plan.gmax.data_ptr() + 4 * self._prod_idx[tin.name]
            w.reduced.add(tin.name)
        check(lib.sc_head_conv_bwd(ptr(w.dlogits), C.byref(s), ptr(conv.weight), ptr(plan.grad[tin.name]), ptr(plan.ws),
                                   plan.ws.numel(), ptr(gv(conv.weight)), ptr(gv(conv.bias)), N, conv.in_channels, Ho, Wo,
                                   bns, bna, w.st))
        self._pe(tok)
        w.written.add(tin.name)

    def _bwd_stem(self, w, i, dy):
        lib, plan, gv = _lib.load(), w.plan, self._grad_view
        conv = self._ops[i]["conv"]
        s = self._src_of(plan, self._ops[i]["ins"][0], x_cst=plan.x_cst)
        tok = self._pb("k_stem_*")
        self._wgrad_launch(w, lambda sx: check(lib.sc_stem_conv_wgrad(
            C.byref(dy), C.byref(s), ptr(plan.ws), plan.ws.numel(), ptr(gv(conv.weight)), plan.N, conv.in_channels, plan.H, plan.W, sx)))
        self._pe(tok)

    def _bwd_irt(self, w, i, dy):
        """fused block: ONE sweep over (dy_d, x) for the depthwise filter gradient, the BatchNorm-backward sums of the
        expanded tensor and the part of dx that does not depend on them; the constants; the Cin -> Cin fix-up of dx; the
        expansion filter's gradient from the partial rows on the weight-gradient stream.  Covers the expand op too."""
        lib, plan, st, gv = _lib.load(), w.plan, w.st, self._grad_view
        op = self._ops[i]
        conv, o = op["conv"], op["out"]
        i_e = plan.irt_of_dw[i]
        w.irt_done.add(i_e)
        op_e = self._ops[i_e]
        te, tin, cv_e = op_e["out"], op_e["ins"][0], op_e["conv"]
        a_irt = self._irt_args(plan, i_e)
        acc = plan.dw_acc[self._dw_offs[i]:self._dw_offs[i] + o.C * 9]
        work, esums = plan.irt_work[te.name], plan.irt_esums[te.name]
        tok = self._pb("k_irt_* (fused expand+dw)")
        self._wgrad_launch(w, lambda sx: check(lib.sc_irt_xmoments(C.byref(a_irt), ptr(work), sx)))
        check(lib.sc_irt_bwd(C.byref(a_irt), C.byref(dy), ptr(esums), ptr(acc), ptr(work), st))
        w.dw_casts.append((acc.data_ptr(), gv(conv.weight).data_ptr(), o.C * 9))
        self._bn_bwd_finalize(w, te, esums, lib.sc_irt_bwd_rows(plan.N, te.C, a_irt.H, a_irt.W), plan.N * a_irt.H * a_irt.W)
        z = self._res_of.get(tin.name)
        check(lib.sc_irt_bwd_fix(C.byref(a_irt), ptr(plan.cstb[te.name]), ptr(work), ptr(plan.grad[tin.name]),
                                 ptr(plan.grad[z]) if z is not None else None, 1 if tin.name in w.written else 0, st))
        self._wgrad_launch(w, lambda sx: check(lib.sc_irt_wgrad_finalize(
            C.byref(a_irt), ptr(plan.cstb[te.name]), ptr(work), ptr(gv(cv_e.weight)), sx)))
        self._pe(tok)
        w.written.add(tin.name)

    def _bwd_dw(self, w, i, dy):
        lib, plan, st, gv = _lib.load(), w.plan, w.st, self._grad_view
        op = self._ops[i]
        conv, o, tin = op["conv"], op["out"], op["ins"][0]
        N, Hi, Wi = plan.N, plan.H >> tin.shift, plan.W >> tin.shift
        s = self._src_of(plan, tin)
        acc = plan.dw_acc[self._dw_offs[i]:self._dw_offs[i] + o.C * 9]
        tok = self._pb("k_dw_*")
        if (tin.name not in w.written and tin.bn is not None and tin.name in plan.dwsums
                and self._n_cons.get(tin.name, 0) == 1):      # the fused sums are complete only for a single-consumer input
            # one pass: dx, dW and the BatchNorm-backward sums of the (6x expanded) input tensor
            check(lib.sc_dwconv3x3_bwd_fused(C.byref(dy), C.byref(s), ptr(conv.weight), ptr(plan.grad[tin.name]), ptr(acc),
                                             ptr(plan.dwsums[tin.name]), N, o.C, Hi, Wi, op["stride"], st))
            w.dw_casts.append((acc.data_ptr(), gv(conv.weight).data_ptr(), o.C * 9))
            w.reduced.add(tin.name)
        else:
            def dw_wgrad(sx):
                check(lib.sc_dwconv3x3_wgrad(C.byref(dy), C.byref(s), ptr(acc), N, o.C, Hi, Wi, op["stride"], sx))
                check(lib.sc_cast_f64_f32(ptr(acc), ptr(gv(conv.weight)), o.C * 9, sx))
            self._wgrad_launch(w, dw_wgrad)
            check(lib.sc_dwconv3x3_dgrad(C.byref(dy), ptr(conv.weight), ptr(plan.grad[tin.name]),
                                         1 if tin.name in w.written else 0, N, o.C, Hi, Wi, op["stride"], st))
        self._pe(tok)
        w.written.add(tin.name)

    def _bwd_wgrad(self, w, i, dy):
        """weight gradient of a pointwise / 3x3 layer on the kernel its route names, on the weight-gradient stream"""
        lib, plan, gv = _lib.load(), w.plan, self._grad_view
        op, L, route = self._ops[i], self._layers[i], plan.routes[i].wgrad
        conv, ins, o = op["conv"], op["ins"], op["out"]
        N, Ho, Wo = plan.N, plan.H >> o.shift, plan.W >> o.shift

        def args(src, xb_of, Cin, part, part_floats, dw):
            wa = sc_wgrad_args()
            wa.dy, wa.nsrc = dy, len(src)
            for k_, s_ in enumerate(src):
                wa.src[k_] = s_
            wa.N, wa.H, wa.W, wa.Cout, wa.Cin, wa.ks = N, Ho, Wo, o.C, Cin, L.ks
            wa.part, wa.part_floats, wa.dw = part, part_floats, dw
            wa.terms, wa.absmax = self._terms[1], w.gmax_slot.get(o.name)
            if L.type == "conv3":
                for k_, t_ in enumerate(xb_of):
                    wa.xbound[k_] = self._xbound(plan, t_)
            return wa

        srcs = [self._src_of(plan, ins[0], up=1 if L.up else 0)] + ([self._src_of(plan, ins[1])] if len(ins) == 2 else [])
        flop = 2.0 * N * Ho * Wo * L.Cout * L.Cin * L.ks * L.ks
        if L.type == "pw" and i not in plan.pw_part:
            # (a fused block's expansion walked on its own -- only_ops -- has no partials buffer: its own launch on the fp32 MFMA)
            route = route._replace(kernel="mfma", entry="sc_conv2d_wgrad_mfma")
        wfn = getattr(lib, route.entry)
        if route.kernel == "spw":
            wu = args(srcs[:1], ins[:1], L.Cin, None, 0, gv(conv.weight).data_ptr())
            wsb, nb = C.c_void_p((plan.spw_ws.data_ptr() + 255) & ~255), plan.spw_ws.numel() - 256
            tok = self._pb(route.family, flop, 0.0, 2.0 * N * (Ho // 2) * (Wo // 2) * 9 * L.Cout * L.Cup + 2.0 * N * Ho * Wo * 9 * L.Cout * L.Csk)
            self._wgrad_launch(w, lambda sx: check(wfn(C.byref(wu), wsb, nb, sx)))
            if route.skip:
                wk = args(srcs[1:], ins[1:], L.Csk, plan.ws.data_ptr(), plan.ws.numel(), plan.spw_skip.data_ptr())
                wsk = getattr(lib, route.skip.entry)

                def skip_cols(sx):
                    check(wsk(C.byref(wk), sx))
                    check(lib.sc_wgrad_scatter_cols(ptr(plan.spw_skip), ptr(gv(conv.weight)), o.C, L.Csk, L.Cin, L.Cup, sx))
                self._wgrad_launch(w, skip_cols)
            self._pe(tok)
            return
        tok = self._pb(route.family, flop)
        part = plan.pw_part.get(i, plan.ws)
        wa = args(srcs, ins, L.Cin, part.data_ptr(), part.numel(), gv(conv.weight).data_ptr())
        if i in plan.pw_part:
            pend = sc_wgrad_pending()
            self._wgrad_launch(w, lambda sx: check(wfn(C.byref(wa), C.byref(pend), sx)))
            w.pw_pending.append(pend)
            if i == w.last_pw:
                # every pointwise layer has been walked: queue the batched reduction NOW, behind this layer's weight gradient, where it
                # runs beside the main stream's last data-gradient kernels (features.1's depthwise backward, 0.16 ms).  At the end of
                # the walk it was the side stream's last launch, 67 us exposed behind the stem's weight gradient before Adam.
                self._reduce_pointwise_batch(w)
        else:
            self._wgrad_launch(w, lambda sx: check(wfn(C.byref(wa), sx)))
        self._pe(tok)

    def _bwd_dgrad(self, w, i, dy):
        """data gradient of a pointwise / 3x3 layer by the launches its route names, on the main stream"""
        lib, plan, st, written = _lib.load(), w.plan, w.st, w.written
        op, L, route, ent = self._ops[i], self._layers[i], plan.routes[i].dgrad, self._wpk[i]
        conv, ins, o = op["conv"], op["ins"], op["out"]
        N, Ho, Wo = plan.N, plan.H >> o.shift, plan.W >> o.shift
        if route.fallback is not None and (ins[0].name in written or self._res_of.get(ins[0].name) is not None):
            route = route.fallback
        a = sc_conv_args()
        a.nsrc = 1
        a.src[0] = dy
        a.N, a.H, a.W, a.ks = N, Ho, Wo, L.ks
        a.terms = self._terms[1]
        a.absmax = w.gmax_slot.get(o.name)
        a.add1 = None; a.stats = None
        flop = 2.0 * N * Ho * Wo * L.Cout * L.Cin * L.ks * L.ks
        # algorithmic bytes of the data gradient: g and y of the output once each, the input gradient once, the filter
        gin_elems = N * L.Cin * Ho * Wo
        if L.up and _tiles(L, self.split_bf16)[3]:      # the upsampled source's gradient is stored 2x2-summed (quarter size)
            gin_elems -= N * L.Cup * Ho * Wo * 3 // 4
        fle = None
        if route.launches[0][1] == "spd":
            # up-sampled channels: 4 parity planes x 4 taps per low-resolution pixel; skip channels: the 3x3 form
            fle = (2.0 * N * (Ho // 2) * (Wo // 2) * 16 * L.Cout * (-(-L.Cup // 128) * 128 + (128 * -(-L.Csk // 32) if route.kernel == "spd+stiles" else 0))
                   + (2.0 * N * Ho * Wo * 9 * L.Cout * L.Csk if route.kernel == "spd+bx3" else 0.0))
        tok = self._pb(route.family, flop, 4.0 * (2 * N * o.C * Ho * Wo + gin_elems + conv.weight.numel()), fle)
        for entry, lay, cot, down, srcs in route.launches:
            ts = [ins[k] for k in srcs]
            acc = [1 if t.name in written else 0 for t in ts]
            a.Cout, a.csplit, a.co_t = sum(t.C for t in ts), ts[0].C, cot
            a.wpk = ent[lay].data_ptr()
            if lay == "bB":       # the skip channels' tile of the 32-wide pack
                a.wpk += 4 * (ent[lay].numel() // (-(-L.Cin // 32)) * (L.Cup // 32))
            if down == 2:
                a.out0, a.accum0, a.down0 = plan.up_tmp.data_ptr(), 0, 0
            else:
                a.out0, a.accum0, a.down0 = plan.grad[ts[0].name].data_ptr(), acc[0], down
            a.out1, a.accum1 = (plan.grad[ts[1].name].data_ptr(), acc[1]) if len(ts) == 2 else (None, 0)
            z = None if L.up else self._res_of.get(ts[0].name)
            a.add0 = plan.grad[z].data_ptr() if z is not None else None
            check(getattr(lib, entry)(C.byref(a), st))
            if down == 2:
                self._pe(tok)
                tok = None
                check(lib.sc_downsum2x2(ptr(plan.up_tmp), ptr(plan.grad[ts[0].name]), acc[0], N, L.Cup, Ho // 2, Wo // 2, st))
            written.update(t.name for t in ts)
        self._pe(tok)

    # ------------------------------------------------------------------------------------------
    def forward(self, x, normalizer_consts=None):
        """(B,C,H,W) -> (B,classes,H,W) logits.  ``normalizer_consts`` (C,8) fuses DataNormalizer.normalize_x into the stem."""
        need_grad = torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters())
        if need_grad:
            self._ensure_flat()
            return _UNetFunction.apply(self, x, normalizer_consts, *list(self.parameters()))
        plan = self._forward_impl(x, normalizer_consts, self.training, False)
        return plan.buf["logits"].clone()

    @torch.no_grad()
    def predict_classes(self, x, normalizer_consts=None):
        """(B,C,H,W) -> (B,H,W) uint8 = ``torch.argmax(logits, dim=1).type(torch.uint8)`` (starcop/sentinel2/models.py:75-78), eval mode
        only.  Same plan and launches as the eval forward up to the head, which writes the class index instead of the logits
        (sc_head_conv_fwd_k with logits = NULL): the logits are never stored, and a plan that only serves this call has no buffer for them."""
        if self.training:
            raise RuntimeError("HyperStarcopUNet.predict_classes: eval mode only (call .eval() first)")
        plan = self._forward_impl(x, normalizer_consts, False, False, head="classes")
        return plan.classes.clone()

    @torch.no_grad()
    def predict_classes_into(self, x, mosaic, table, normalizer_consts=None):
        """``predict_classes`` for the windows of a scene: of batch item i only the core rectangle is kept, written by the head itself
        (sc_head_conv_fwd_k_mosaic) into ``mosaic``, a uint8 (h, w) device tensor with unit column stride.  ``table`` = (device int32
        (n, 8) tensor, the same contiguous int32 numpy array on the host, first row): rows first .. first + N - 1 are the
        ``sc_scene_win`` of the batch -- core y0, y1, x0, x1 inside the window at [2:6], the core's row and column in the mosaic at
        [6:8] (scene.scene_table).  No logits and no (N, H, W) class tensor exist.  Eval mode only.  Returns ``mosaic``."""
        if self.training:
            raise RuntimeError("HyperStarcopUNet.predict_classes_into: eval mode only (call .eval() first)")
        _lib.require_device(mosaic)
        if mosaic.dtype != torch.uint8 or mosaic.dim() != 2 or mosaic.stride(1) != 1:
            raise ValueError("predict_classes_into: mosaic must be a uint8 (h, w) tensor with unit column stride")
        win, win_host = scene.table_rows("predict_classes_into", *table, x.shape[0])
        self._forward_impl(x, normalizer_consts, False, False, head="mosaic", mosaic=HeadMosaic(win, win_host, classes=mosaic))
        return mosaic

    @torch.no_grad()
    def predict_masks_into(self, x, prob, mask, table, normalizer_consts=None, valid=None, fill_value=None, nodata=-9999.0):
        """The binary model over the windows of a scene: of batch item i only the core rectangle is kept, and the head itself
        (sc_head_conv_fwd_mosaic_prob) writes ``sigmoid(logit)`` into ``prob`` (float32 (h, w) device tensor, unit column stride) and
        ``sigmoid(logit) > 0.5`` into ``mask`` (uint8, likewise) -- the values ``masks_from_logits`` derives from the eval forward's
        logits.  Either of ``prob`` / ``mask`` may be None, not both.  ``table`` as for ``predict_classes_into``.  ``valid``: an
        (h, w) float32 device plane (any non-negative strides) whose pixels with the bits of float32(``fill_value``) get
        ``nodata`` / 0 instead.  No logits and no per-window tensors exist.  Eval mode, ``classes == 1`` only.  Returns (prob, mask)."""
        if self.training:
            raise RuntimeError("HyperStarcopUNet.predict_masks_into: eval mode only (call .eval() first)")
        if self.classes != 1:
            raise ValueError(f"HyperStarcopUNet.predict_masks_into: the probability head is the 1-class model's (classes={self.classes})")
        if prob is None and mask is None:
            raise ValueError("predict_masks_into: at least one of prob / mask must be given")
        shapes = set()
        for name, t, dt in (("prob", prob, torch.float32), ("mask", mask, torch.uint8)):
            if t is None:
                continue
            _lib.require_device(t)
            if t.dtype != dt or t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"predict_masks_into: {name} must be a {dt} (h, w) tensor with unit column stride")
            shapes.add(tuple(t.shape))
        if len(shapes) != 1:
            raise ValueError("predict_masks_into: prob and mask must have one shape")
        fill_bits = 0
        if valid is not None:
            _lib.require_device(valid)
            if valid.dtype != torch.float32 or tuple(valid.shape) not in shapes or fill_value is None:
                raise ValueError("predict_masks_into: valid must be a float32 plane of the mosaics' shape, with a fill_value")
            fill_bits = scene.float_bits(fill_value)
        win, win_host = scene.table_rows("predict_masks_into", *table, x.shape[0])
        self._forward_impl(x, normalizer_consts, False, False, head="probmosaic",
                           mosaic=HeadMosaic(win, win_host, prob=prob, mask=mask, valid=valid, fill_bits=fill_bits, nodata=float(nodata)))
        return prob, mask


class _UNetFunction(torch.autograd.Function):
    """Whole-network autograd node: backward runs the HIP backward pass into the flat grad buffer."""

    @staticmethod
    def forward(ctx, net, x, x_cst, *params):
        plan = net._forward_impl(x, x_cst, True, True)
        ctx.net, ctx.plan, ctx.generation = net, plan, plan.generation
        return plan.buf["logits"].clone()

    @staticmethod
    def backward(ctx, g):
        net, plan = ctx.net, ctx.plan
        if plan.generation != ctx.generation:
            raise RuntimeError("HyperStarcopUNet.backward: another forward of the same input shape ran after this one; the "
                               "network keeps ONE set of activation buffers per (N, H, W), so call backward() before the next "
                               "train-mode forward of that shape (or use a different batch shape)")
        params = list(net.parameters())
        # Gradient accumulation (accumulate_grad_batches > 1, zero_grad(set_to_none=False)): a p.grad left over from the last
        # backward IS a view of the flat gradient buffer, which _backward_impl overwrites.  Move those accumulators onto a
        # snapshot first and hand autograd fresh copies, so AccumulateGrad computes old + new (never new + new).
        aliased = [p.grad is not None and p.grad.data_ptr() == net._grad_view(p).data_ptr() for p in params]
        if any(aliased):
            snap = net._gflat.clone()
            base = net._gflat.data_ptr()
            for p, al in zip(params, aliased):
                if al:
                    off = (p.grad.data_ptr() - base) // 4
                    p.grad = snap[off:off + p.numel()].view(p.shape)
        net._backward_impl(plan, g.float())
        grads = [net._grad_view(p).clone() if al else net._grad_view(p) for p, al in zip(params, aliased)]
        return (None, None, None) + tuple(grads)
