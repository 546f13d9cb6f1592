"""Time of the Sentinel-2 cloud detector's network (HyperStarcopUNet(13, 4), starcop/sentinel2/models.py:63-78) with the argmax fused
into the head against the eval forward followed by torch.argmax, and of the two kernels that are new for it, in one process.

    python tools/bench_cdmodel.py [--batch 16] [--size 512] [--rounds 6] [--reps 10] [--out profiles/cdmodel.txt]

Case: seeded weights and BatchNorm statistics, a seeded randn batch of --batch x 13 x --size x --size.
  (a)  net.predict_classes(x): the plan's launches with the head writing uint8 class indices (sc_head_conv_fwd_k, logits = NULL),
       and the copy of the (N, H, W) uint8 result out of the plan
  (b)  net(x) followed by torch.argmax(dim=1).to(torch.uint8): the same launches with the head writing (N, 4, H, W) fp32 logits, the
       copy of the logits out of the plan, and torch's reduction and cast
  (c)  the first and the last layer on their own, through the C ABI: sc_stem_conv_fwd at 13 channels; sc_head_conv_fwd_k on a
       (N, 16, H, W) tensor writing classes only, and writing logits only followed by torch.argmax(dim=1).to(torch.uint8)
(a) and (b) -- and the two head forms of (c) -- alternate in rounds of --reps calls after 3 warm-up calls each (device events);
the figure is the mean over all rounds, the spread the minimum and maximum round.  Their results are asserted equal before
anything is timed.  Bytes: what each kernel must read and write once, from the shapes.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from starcop_amd import _lib  # noqa: E402
from starcop_amd._lib import ACT_RELU, SC_CST, SRC_AFFINE, SRC_RAW, check, make_src, ptr, stream  # noqa: E402
from starcop_amd.network import HyperStarcopUNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    N, S, Cin, K = args.batch, args.size, 13, 4
    torch.manual_seed(0)
    net = HyperStarcopUNet(Cin, K)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
        net.segmentation_head[0].bias.copy_(torch.randn(K, generator=g) * 0.1)
    net = net.cuda().eval()
    x = torch.randn(N, Cin, S, S, generator=torch.Generator().manual_seed(2)).cuda()

    def run_a():
        return net.predict_classes(x)

    def run_b():
        with torch.no_grad():
            return torch.argmax(net(x), dim=1).to(torch.uint8)

    # (c) operands: the stem on x; the head on a seeded tensor read through a BatchNorm + ReLU prologue, as in the network
    w_stem = net.encoder.features[0][0].weight
    stem_out = torch.empty(N, 32, S // 2, S // 2, device="cuda")
    src_x = make_src(x, Cin, SRC_RAW)
    h_in = torch.randn(N, 16, S, S, generator=torch.Generator().manual_seed(3)).cuda()
    cst = torch.zeros(16, SC_CST, device="cuda")
    cst[:, 0], cst[:, 1] = 1.0, 0.1
    src_h = make_src(h_in, 16, SRC_AFFINE, act=ACT_RELU, cst=cst)
    w_head, b_head = net.segmentation_head[0].weight, net.segmentation_head[0].bias
    h_logits = torch.empty(N, K, S, S, device="cuda")
    h_classes = torch.empty(N, S, S, dtype=torch.uint8, device="cuda")

    def run_stem():
        check(lib.sc_stem_conv_fwd(C.byref(src_x), ptr(w_stem), ptr(stem_out), N, Cin, S, S, None, stream()))

    def run_head_classes():
        check(lib.sc_head_conv_fwd_k(C.byref(src_h), ptr(w_head), ptr(b_head), None, ptr(h_classes), N, 16, K, S, S, stream()))
        return h_classes

    def run_head_logits():
        check(lib.sc_head_conv_fwd_k(C.byref(src_h), ptr(w_head), ptr(b_head), ptr(h_logits), None, N, 16, K, S, S, stream()))

    def run_head_logits_argmax():
        run_head_logits()
        return torch.argmax(h_logits, dim=1).to(torch.uint8)

    def events(fn, reps=args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps          # ms per call

    # results first: the fused argmax is the argmax of the logits the other form stores
    got_a, got_b = run_a(), run_b()
    torch.cuda.synchronize()
    assert got_a.shape == (N, S, S) and got_a.dtype == torch.uint8
    assert torch.equal(got_a, got_b), "predict_classes differs from argmax of the eval logits"
    counts = torch.bincount(got_a.flatten().long(), minlength=K).tolist()
    hc = run_head_classes().clone()
    assert torch.equal(hc, run_head_logits_argmax()), "the head's fused argmax differs from torch.argmax of its logits"
    del got_a, got_b, hc
    fns = (run_a, run_b, run_stem, run_head_classes, run_head_logits, run_head_logits_argmax)
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(args.rounds):
        for i, fn in enumerate(fns):
            t[i].append(events(fn))

    def fig(v, unit=1.0):
        return f"{float(np.mean(v)) * unit:9.1f}   (rounds {min(v) * unit:.1f} .. {max(v) * unit:.1f})"

    px = N * S * S
    stem_bytes = 4 * (N * Cin * S * S + N * 32 * (S // 2) * (S // 2))
    head_in = 4 * 16 * px
    lines = [
        f"HyperStarcopUNet(13, 4) inference, batch {N} x 13 x {S} x {S} (seeded randn), precision {net.precision!r}; "
        f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
        f"{args.rounds} alternating rounds of {args.reps} calls after 3 warm-up calls each, device events; (a) == (b) in all {px} pixels "
        f"(class counts {counts}), and the head's fused argmax == torch.argmax of its stored logits",
        f"(a) predict_classes (head writes uint8 classes)                 {fig(t[0])} ms per call",
        f"(b) eval forward + torch.argmax(dim=1).to(uint8)                {fig(t[1])} ms per call",
        f"(c) sc_stem_conv_fwd, 13 -> 32 channels, stride 2               {fig(t[2], 1e3)} us per call; "
        f"{stem_bytes / 1e6:.1f} MB read + written once",
        f"(c) sc_head_conv_fwd_k, 16 -> 4, classes only                   {fig(t[3], 1e3)} us per call; "
        f"{head_in / 1e6:.1f} MB read + {px / 1e6:.1f} MB written",
        f"(c) sc_head_conv_fwd_k, 16 -> 4, logits only                    {fig(t[4], 1e3)} us per call; "
        f"{head_in / 1e6:.1f} MB read + {4 * K * px / 1e6:.1f} MB written",
        f"(c) ... logits only, then torch.argmax(dim=1).to(uint8)         {fig(t[5], 1e3)} us per call",
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
