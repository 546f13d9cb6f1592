"""Time of the pointwise regression networks: the fused training step and the inference forward of SimpleCNN_v2 / SimpleCNN_v3
next to the same work with stock torch ops on the GPU, in one process.

    python tools/bench_pwreg.py [--batch 16] [--size 512] [--rounds 6] [--loss l1] [--out profiles/pwreg.txt]

Input: seeded batch x 13 x size x size -> 12 (float32), targets at a distance from the prediction (so that L1's sign is no draw).
  (a)  ModelModuleRegression.fused_train_step: sc_pwreg_train_sweep + sc_pwreg_finalize + the fused Adam
  (b)  the same step with stock torch ops: F.conv2d (1x1) per layer, F.l1_loss / F.mse_loss, backward(), torch.optim.Adam.step()
  (c)  the inference forward sc_pwreg_fwd          (d)  F.conv2d per layer under no_grad
(a)/(b) and (c)/(d) alternate in rounds of 10 calls after 10 warm-up calls each (device events); the figure is the mean over all
rounds, the spread the minimum and maximum round.  Before anything is timed, one step of (a) and of (b) from the same parameters
are asserted equal to 1e-5 of the largest parameter, and the two forwards to 1e-5 of the largest prediction.
Bytes of (a): x and y once, (Cin + Cout) * 4 * N * H * W; of (c): x read and the prediction written, the same count.
"""
import argparse
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from starcop_amd import _lib, model_module as mm, model_module_regression as mmr  # noqa: E402

CIN, COUT = 13, 12


def settings(model_type, loss):
    s = mm.default_settings(model_mode="regression_output", model_type=model_type, loss=loss, num_classes=COUT, lr=1e-4)
    s.dataset.input_products = [f"TOA_S2B_B{b}" for b in ("1", "2", "3", "4", "5", "6", "7", "8", "8A", "9", "10", "11", "12")]
    s.dataset.output_products = ["TOA_WV3_SWIR1"]
    return s


def events(fn, reps=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps          # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--loss", default="l1", choices=("l1", "mse"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    N, S = args.batch, args.size
    gen = torch.Generator().manual_seed(1355)
    x = (torch.rand(N, CIN, S, S, generator=gen) * 2).cuda()
    nbytes = (CIN + COUT) * 4 * N * S * S
    lines = [f"pointwise regression networks, {N} x {CIN} x {S} x {S} -> {COUT}, loss {args.loss}; {torch.cuda.get_device_name(0)} "
             f"({torch.cuda.get_device_properties(0).gcnArchName})",
             f"{args.rounds} alternating rounds of 10 calls after 10 warm-up calls each, device events; results asserted equal first",
             f"bytes per call (x and y once, or x read and the prediction written): {nbytes / 1e6:.1f} MB"]
    for model_type in ("cnn_v2", "cnn_v3"):
        torch.manual_seed(7)
        model = mmr.ModelModuleRegression(settings(model_type, args.loss)).cuda().train()
        stock = [(c.weight.detach().clone().requires_grad_(True), c.bias.detach().clone().requires_grad_(True))
                 for c in model.network.cnn_layers]
        start = copy.deepcopy(model.network.state_dict())

        def stock_fwd(t):
            for w, b in stock:
                t = F.conv2d(t, w, b)
            return t

        with torch.no_grad():
            pred = model(x)
            want = stock_fwd(x)
            assert float((pred - want).abs().max()) <= 1e-5 * float(want.abs().max()), "forwards disagree"
            y = pred + (torch.rand(pred.shape, generator=gen).cuda() * 0.2 + 0.01) * (torch.randint(0, 2, pred.shape, generator=gen).cuda() * 2 - 1)
        batch = {"input": x, "output": y}
        opt_a = model.configure_optimizers()["optimizer"]
        opt_b = torch.optim.Adam([p for wb in stock for p in wb], 1e-4)
        loss_b = F.l1_loss if args.loss == "l1" else F.mse_loss

        def run_a():
            model.fused_train_step(batch, opt_a)

        def run_b():
            opt_b.zero_grad(set_to_none=True)
            loss_b(stock_fwd(x), y).backward()
            opt_b.step()

        def run_c():
            with torch.no_grad():
                return model(x)

        def run_d():
            with torch.no_grad():
                return stock_fwd(x)

        run_a()
        run_b()
        torch.cuda.synchronize()
        flat_b = torch.cat([p.detach().reshape(-1) for wb in stock for p in wb])
        flat_a = model.network.flat_parameters()
        assert float((flat_a - flat_b).abs().max()) <= 1e-5 * float(flat_b.abs().max()), "one training step disagrees"
        assert not torch.equal(flat_a, torch.cat([v.reshape(-1) for v in start.values()]).cuda())
        t = {}
        for a, b in ((run_a, run_b), (run_c, run_d)):
            for fn in (a, b):
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(events(a))
                tb.append(events(b))
            t[a.__name__], t[b.__name__] = ta, tb

        def row(tag, key, other=None):
            m = float(np.mean(t[key]))
            s = f"{model_type} {tag:<58s}{m:9.3f} ms per call   (rounds {min(t[key]):.3f} .. {max(t[key]):.3f})   {nbytes / (m * 1e-3) / 1e12:.2f} TB/s"
            if other:
                s += f"   stock / HIP = {float(np.mean(t[other])) / m:.1f}"
            return s

        lines += [row("(a) fused step: sweep + finalize + Adam", "run_a", "run_b"),
                  row("(b) stock torch: conv2d, loss, backward, Adam", "run_b"),
                  row("(c) sc_pwreg_fwd", "run_c", "run_d"),
                  row("(d) stock torch: conv2d", "run_d")]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
