"""Regression path on the GPU: sc_pwreg_fwd, sc_reg_loss, the fused sweep + finalize and the autograd path of SimpleCNN_v2 / v3
against the float64 oracle (tests/golden/g14_regression.npz for the stored cases, tests/regression_util.py for B and E, which are too
large to store), ModelModuleRegression's steps, the unet_semseg regression step and the learned band-ratio feature.

Gates.  Prediction: within 1e-4 of the float64 oracle relative to its largest value (the project's logit contract).  Loss and every
parameter gradient: max |delta| to the float64 oracle relative to max |oracle| is at most 4 x the same quantity of the float32
torch CPU path, floored at 1e-6 (a few fp32 ulps: the CPU path's error on a small case can fall near zero by chance).  The kernels
accumulate in fp64, so the ratio should sit at or below 1; the measured figures are printed (pytest -s) and recorded in
profiles/pwreg_parity.txt."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import regression_util as ru  # noqa: E402
from mlr_util import wv3_tile  # noqa: E402
from starcop_amd import _lib, features, model_module as mm, model_module_regression as mmr  # noqa: E402
from starcop_amd.pointwise_net import SimpleCNN_v2, SimpleCNN_v3  # noqa: E402

DEV = "cuda"
GEO = {33550: (12, (3.7, 3.7, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 500000.0, 4100000.0, 0.0)),
       34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32611))}
MARGIN, FLOOR = 4.0, 1e-6
KIND = {"l1": _lib.REG_L1, "mse": _lib.REG_MSE}
GPU_CASES = ("A_v2", "A_v3", "B", "C", "D", "E")


@pytest.fixture(scope="module")
def g14():
    return ru.load_g14()


@pytest.fixture(scope="module")
def cases(g14):
    """name -> case with its CPU oracle: [loss][f64 | f32] = dict(loss, grads), and the float64 prediction"""
    out = {}
    for name in GPU_CASES:
        if name in ru.STORED:
            c = dict(g14[name])
        else:
            c = ru.build_case(name)
            c.update(ru.oracle(c))
        c["pred64"] = ru.run(c["params"], c["x"], c["y"], "mse", torch.float64)["pred"]
        out[name] = c
    return out


def _net(c, params=None):
    net = (SimpleCNN_v3 if c["layers"] == 2 else SimpleCNN_v2)(c["cin"], c["cout"])
    net.load_state_dict({k: torch.from_numpy(np.asarray(p)) for k, p in zip(net.state_dict(), params if params is not None else c["params"])})
    return net.to(DEV)


def _fused(net, x, y, loss):
    acc = torch.empty(1, dtype=torch.float64, device=DEV)
    n = net.sweep_gradients(x, y, KIND[loss], acc)
    return acc / n, [net._grad_view(p).clone() for p in net.parameters()]


def _autograd(net, x, y, loss):
    for p in net.parameters():
        p.grad = None
    val = getattr(mmr, loss)(net(x), y)
    val.backward()
    return val.detach().clone(), [p.grad.clone() for p in net.parameters()]


def _gate(tag, got, o64, o32):
    e, e32 = ru.rel_err(got, o64), ru.rel_err(o32, o64)
    print(f"parity {tag}: gpu {e:.3e}  fp32 cpu {e32:.3e}  ratio {e / e32 if e32 > 0 else float('inf'):.3g}")
    assert e <= max(MARGIN * e32, FLOOR), (tag, e, e32)


@pytest.mark.parametrize("name", GPU_CASES)
def test_cases(hip, cases, name):
    c = cases[name]
    net = _net(c)
    x, y = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["y"]).to(DEV)
    with torch.no_grad():
        pred = net(x)
    assert pred.shape == c["pred64"].shape and pred.dtype == torch.float32
    e = ru.rel_err(pred.cpu().numpy(), c["pred64"])
    print(f"parity {name} prediction: gpu {e:.3e}")
    assert e <= 1e-4, (name, e)
    with torch.no_grad():
        assert torch.equal(net(x), pred)
    # the condition of the L1 gates: no element's sign(pred - y) is a rounding draw
    assert int((np.sign(pred.cpu().numpy() - c["y"]) != np.sign(c["pred64"] - c["y"])).sum()) == 0
    for loss in ru.LOSSES:
        o64, o32 = c[loss]["f64"], c[loss]["f32"]
        for path, fn in (("fused", _fused), ("autograd", _autograd)):
            val, grads = fn(net, x, y, loss)
            _gate(f"{name} {loss} {path} loss", val.cpu().numpy(), o64["loss"], o32["loss"])
            for i, (gr, key) in enumerate(zip(grads, net.state_dict())):
                assert gr.shape == o64["grads"][i].shape
                _gate(f"{name} {loss} {path} {key}", gr.cpu().numpy(), o64["grads"][i], o32["grads"][i])
            val2, grads2 = fn(net, x, y, loss)
            assert torch.equal(val, val2) and all(torch.equal(a, b) for a, b in zip(grads, grads2)), (name, loss, path, "determinism")


def test_misaligned_views_and_refusals(hip, cases):
    """a tensor that starts 4 bytes off a 16-byte boundary takes the element path and gives the same bits; x.requires_grad raises"""
    c = cases["C"]
    net = _net(c)
    x = torch.from_numpy(c["x"]).to(DEV)
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=DEV)
    xo = buf[1:].view(x.shape)
    xo.copy_(x)
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    with torch.no_grad():
        assert torch.equal(net(xo), net(x))
    y = torch.from_numpy(c["y"]).to(DEV)
    a, b = _fused(net, xo, y, "mse"), _fused(net, x, y, "mse")
    assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))
    with pytest.raises(RuntimeError, match="no input gradient"):
        net(x.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        net(x[:, :5])


def test_sign_of_zero(hip):
    """zero weights, bias b, y == b on a known subset: L1's db is (n+ - n-) / n and the loss is the oracle's"""
    N, H, W = 2, 9, 11
    net = SimpleCNN_v2(3, 2)
    b = np.array([0.25, -0.5], np.float32)
    net.load_state_dict({"cnn_layers.0.weight": torch.zeros(2, 3, 1, 1), "cnn_layers.0.bias": torch.from_numpy(b)})
    net = net.to(DEV)
    rng = np.random.default_rng(7)
    x = rng.integers(0, 4 * ru.QUANT_X, size=(N, 3, H, W)).astype(np.float32) / ru.QUANT_X
    pick = rng.integers(0, 3, size=(N, 2, H, W))                  # 0: y == pred, 1: pred > y, 2: pred < y
    y = (b[None, :, None, None] + np.array([0.0, -0.5, 0.5], np.float32)[pick]).astype(np.float32)
    n = y.size
    want_db = ((pick == 1).sum(axis=(0, 2, 3)) - (pick == 2).sum(axis=(0, 2, 3))) / n
    want = ru.run([np.zeros((2, 3, 1, 1), np.float32), b], x, y, "l1", torch.float64)
    assert np.abs(want["grads"][1] - want_db).max() < 1e-15          # torch's sign(0) is 0
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    val, grads = _fused(net, xd, yd, "l1")
    assert abs(float(val) - float(want["loss"])) <= 1e-12
    # exact integer sums in fp64, a product with 1/n in fp64, one rounding to fp32
    assert (np.abs(grads[1].cpu().numpy().astype(np.float64) - want_db) <= 2.0 ** -24 * (1 + 1e-9) * np.abs(want_db)).all()
    assert ru.rel_err(grads[0].cpu().numpy(), want["grads"][0]) <= FLOOR
    val, grads = _autograd(net, xd, yd, "l1")
    assert abs(float(val) - float(want["loss"])) <= 1e-7 * float(want["loss"])       # the mean as one fp32 number
    # the stored gradient is +-fl32(1/n) or 0: their fp64 sum is (n+ - n-) fl32(1/n), two fp32 roundings from the exact value
    assert np.abs(grads[1].cpu().numpy() - want_db).max() <= 2 ** -22 * np.abs(want_db).max()


def _settings(model_type, loss, n_in, n_out, lr=1e-4):
    s = mm.default_settings(model_mode="regression_output", model_type=model_type, loss=loss, num_classes=n_out, lr=lr)
    s.dataset.input_products = [f"TOA_WV3_SWIR{i % 8 + 1}" for i in range(n_in)]
    s.dataset.output_products = ["TOA_WV3_SWIR8"]
    return s


def _cpu_adam(c, loss, dtype, steps, lr):
    """torch.optim.Adam on the restatement -> parameters after each step"""
    with ru.one_thread():
        ps = [torch.from_numpy(p).to(dtype).clone().requires_grad_(True) for p in c["params"]]      # (a copy: Adam steps in place)
        x, y = torch.from_numpy(c["x"]).to(dtype), torch.from_numpy(c["y"]).to(dtype)
        opt = torch.optim.Adam(ps, lr)
        trail = []
        for _ in range(steps):
            opt.zero_grad()
            ru.loss_fn(loss)(ru.forward(ps, x), y).backward()
            opt.step()
            trail.append(np.concatenate([p.detach().numpy().reshape(-1).astype(np.float64) for p in ps]))
    return trail


def test_twenty_adam_steps(hip, cases):
    c, loss, lr, steps = cases["A_v3"], "l1", 1e-4, 20
    t64, t32 = _cpu_adam(c, loss, torch.float64, steps, lr), _cpu_adam(c, loss, torch.float32, steps, lr)
    batch = {"input": torch.from_numpy(c["x"]).to(DEV), "output": torch.from_numpy(c["y"]).to(DEV)}

    def module():
        m = mmr.ModelModuleRegression(_settings("cnn_v3", loss, c["cin"], c["cout"], lr))
        m.network.load_state_dict({k: torch.from_numpy(p) for k, p in zip(m.network.state_dict(), c["params"])})
        return m.to(DEV).train()

    def flat(m):
        return m.network.flat_parameters().cpu().numpy().astype(np.float64)

    fused = module()
    opt = fused.configure_optimizers()["optimizer"]
    first = None
    for i in range(steps):
        acc = fused.fused_train_step(batch, opt)
        if i == 0:
            first = flat(fused)
            want = ru.run(c["params"], c["x"], c["y"], loss, torch.float64)["loss"]
            assert abs(float(acc) / fused.loss_n - want) <= FLOOR * want
    scale = np.abs(t64[-1]).max()
    d, d32 = np.abs(flat(fused) - t64[-1]).max() / scale, np.abs(t32[-1] - t64[-1]).max() / scale
    print(f"parity adam20 A_v3 l1: gpu {d:.3e}  fp32 cpu {d32:.3e}")
    assert d <= max(MARGIN * d32, FLOOR), (d, d32)

    auto = module()
    opt = auto.configure_optimizers()["optimizer"]
    val = auto.training_step(batch, 0)
    val.backward()
    opt.step()
    gate = max(MARGIN * np.abs(t32[0] - t64[0]).max() / scale, FLOOR)
    d1, da = np.abs(first - t64[0]).max() / scale, np.abs(flat(auto) - first).max() / scale
    print(f"parity adam1 A_v3 l1: fused {d1:.3e}  training_step vs fused {da:.3e}  gate {gate:.3e}")
    assert d1 <= gate and da <= gate, (d1, da, gate)
    if not mm.HAVE_LIGHTNING:
        assert auto._logged["train_l1_loss"] is val
    auto.eval()
    with torch.no_grad():
        assert auto.validation_step(batch, 0) is None
        out = auto.batch_with_preds(batch)
    assert out["logits"] is out["prediction"] and torch.equal(out["differences"], out["prediction"] - batch["output"])


def test_unet_semseg_regression(hip):
    rng = np.random.default_rng(11)
    pred, y = rng.standard_normal((2, 1, 64, 64)).astype(np.float32), rng.standard_normal((2, 1, 64, 64)).astype(np.float32)
    y.reshape(-1)[::7] = pred.reshape(-1)[::7]                      # exact zeros of pred - y
    pd_, yd = torch.from_numpy(pred).to(DEV), torch.from_numpy(y).to(DEV)
    for loss in ru.LOSSES:
        p64 = torch.from_numpy(pred).double().requires_grad_(True)
        want = ru.loss_fn(loss)(p64, torch.from_numpy(y).double())
        want.backward()
        d = torch.empty_like(pd_)
        got = float(mmr.reg_loss_sum(pd_, yd, loss, d)) / pred.size
        want = want.detach()
        # fp64 sums of fp32 differences; the gradient is two or three fp32 roundings of an exact value: a few fp32 ulps
        assert abs(got - float(want)) <= FLOOR * float(want), loss
        assert ru.rel_err(d.cpu().numpy(), p64.grad.numpy()) <= FLOOR, loss
        d2 = torch.empty_like(pd_)
        assert float(mmr.reg_loss_sum(pd_, yd, loss, d2)) / pred.size == got and torch.equal(d, d2)
    torch.manual_seed(3)
    s = mm.default_settings(model_mode="regression_output", loss="mse")
    model = mmr.ModelModuleRegression(s).to(DEV).train()
    x = torch.from_numpy(rng.uniform(0, 2, (2, 4, 64, 64)).astype(np.float32)).to(DEV)
    before = model.network.flat_parameters().clone()
    acc = model.fused_train_step({"input": x, "output": yd})
    assert np.isfinite(float(acc)) and model.loss_n == 2 * 64 * 64
    after = model.network.flat_parameters()
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)


def test_learned_feature(hip, g14, tmp_path):
    import pandas as pd
    from starcop_amd import io_formats as io
    f = g14["feature"]
    net = SimpleCNN_v2(6, 1)
    net.load_state_dict({k: torch.from_numpy(p) for k, p in zip(net.state_dict(), f["params"])})
    name = "ratio_lrn_bands2band8only_60ep_512_l1"
    fn = features.FEATURES[name]["function"]
    features.set_learned_model(net.to(DEV))
    try:
        for tile in f["names"]:
            bands, target = f[f"{tile}_bands"], f[f"{tile}_target"]
            args = [torch.from_numpy(b).to(DEV) for b in bands] + [torch.from_numpy(target).to(DEV)]
            got = fn(*args).cpu().numpy()
            assert got.shape == target.shape and got.dtype == np.float32 and np.isfinite(got).all()
            f64, f32 = f[f"{tile}_f64"], f[f"{tile}_f32"].astype(np.float64)
            e64, own = np.abs(got - f64).max(), np.abs(f32 - f64).max()
            print(f"parity feature {tile}: gpu {e64:.3e}  fp32 reference {own:.3e}")
            assert e64 <= 2e-6, (tile, e64)                     # tests/test_gpu_mlr.py: TOL64["c_matched_outliers"] and its fp32 rule
            assert np.abs(got - f32).max() <= max(1e-5, 1.5 * own), tile
            assert (got[target == 0] == np.float32(-0.5)).all()
            assert torch.equal(fn(*[a[None] for a in args])[0], torch.from_numpy(got).to(DEV))       # batched over leading dimensions
        assert (f["border_target"] == 0).sum() > 0
        rng = np.random.default_rng(31)
        folders = []
        for i in range(2):
            d = tmp_path / f"wv3_{i}"
            d.mkdir()
            b, t = wv3_tile(rng, 128, 128, k=6, border=3 * i)
            for j in range(6):
                io.write_tiff(str(d / f"TOA_WV3_SWIR{j + 1}.tif"), b[j], extra_tags=GEO)
            io.write_tiff(str(d / "TOA_WV3_SWIR8.tif"), t, extra_tags=GEO)
            folders.append(str(d))
        features.extract_features([name], pd.DataFrame({"folder": folders}), device=DEV)
        for d in folders:
            got = io.read_tiff(os.path.join(d, f"{name}.tif"))
            ins = torch.from_numpy(io.load_sample(d, features.FEATURES[name]["inputs"])).to(DEV)
            assert got.shape == (1, 128, 128) and np.array_equal(got, fn(*[ins[i:i + 1] for i in range(7)]).cpu().numpy())
    finally:
        features.set_learned_model(None)
    with pytest.raises(NotImplementedError):
        fn()
