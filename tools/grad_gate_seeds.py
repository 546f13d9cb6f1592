"""How often does tests/test_gpu_unet.py::test_train_forward_backward_and_adam's per-parameter gate (HIP error vs the fp64 oracle <=
max(1e-3, 6 x the fp32 CPU path's own error)) trip for OTHER seeds than the test's -- i.e. is a failing parameter a property of a kernel
or a draw?   usage: python tools/grad_gate_seeds.py [first_seed=3] [n=6]"""
import copy, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from test_gpu_unet import make_pair, ref_normalize, synth_batch, to_dev, relerr, GRAD_RATIO_GATE

s0 = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else 6
B, H, W = 4, 128, 128
for seed in range(s0, s0 + n):
    model, ref = make_pair(seed=seed, pos_weight=1.0)
    model.train(); ref.train()
    ref64 = copy.deepcopy(ref).double()
    batch = synth_batch(B, H, W, seed=seed + 2)

    def oracle_step(net, dt):
        logits = net(ref_normalize(batch["input"]).to(dt))
        loss = (F.binary_cross_entropy_with_logits(logits, batch["output"].to(dt), pos_weight=torch.tensor(1.0, dtype=dt),
                                                   reduction="none") * batch["weight_loss"].to(dt)).mean()
        net.zero_grad(); loss.backward()
        return {k: p.grad.clone() for k, p in net.named_parameters()}

    g32, g64 = oracle_step(ref, torch.float32), oracle_step(ref64, torch.float64)
    opt = model.configure_optimizers()["optimizer"]
    loss = model.training_step(to_dev(batch), 0)
    opt.zero_grad(); loss.backward()
    bad, ratios = [], []
    for k, p in model.network.named_parameters():
        e_hip, e_ref = relerr(p.grad, g64[k]), relerr(g32[k], g64[k])
        ratios.append(e_hip / max(e_ref, 1e-7))
        if not e_hip <= max(1e-3, GRAD_RATIO_GATE * e_ref):
            bad.append((k, round(e_hip, 5), round(e_ref, 5)))
    print(f"seed {seed}: {len(bad)} parameters over the gate, median ratio {float(np.median(ratios)):.2f}  {bad[:4]}")
