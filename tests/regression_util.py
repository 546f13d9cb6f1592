"""Plain-torch restatement of the reference's regression networks and losses (SimpleCNN_v2 / SimpleCNN_v3 of
starcop/models/architectures/baselines.py:43-70, l1 / mse of starcop/models/utils/losses.py), run on the CPU in float32 and
float64, plus the seeded cases shared by tests/golden/make_golden_regression.py and the regression tests.  It is checked against
the reference's own outputs (tests/golden/g14_regression.npz) and is the oracle for the shapes too large to store there."""
import contextlib
import os

import numpy as np
import torch
import torch.nn.functional as F

QUANT_X = 16384        # inputs are uint16 counts of 1 / QUANT_X (exact in float32), as the tiles of g12 are
QUANT_Y = 4096         # targets are int16 counts of 1 / QUANT_Y
LOSSES = ("l1", "mse")

# name -> shape; `x` names the stored input (A's two networks share one)
CASES = {
    "A_v2": dict(N=3, cin=13, cout=12, layers=1, H=37, W=41, seed=1401, x="A"),
    "A_v3": dict(N=3, cin=13, cout=12, layers=2, H=37, W=41, seed=1402, x="A"),
    "B": dict(N=2, cin=6, cout=1, layers=1, H=128, W=160, seed=1403, x="B"),
    "C": dict(N=1, cin=16, cout=16, layers=2, H=64, W=64, seed=1404, x="C"),
    "D": dict(N=1, cin=1, cout=1, layers=1, H=5, W=3, seed=1405, x="D"),
    "E": dict(N=4, cin=13, cout=12, layers=1, H=256, W=256, seed=1406, x="E"),
    "mini_v2": dict(N=2, cin=13, cout=12, layers=1, H=5, W=7, seed=1407, x="mini"),
    "mini_v3": dict(N=2, cin=13, cout=12, layers=2, H=5, W=7, seed=1408, x="mini"),
}
STORED = ("A_v2", "A_v3", "C", "D", "mini_v2", "mini_v3")      # in g14; B and E are too large and come from this module
X_SEED = {"A": 1411, "B": 1412, "C": 1413, "D": 1414, "E": 1415, "mini": 1416}


def state_dict_spec(cin, cout, layers):
    """[(key, shape)] of the reference's state_dict"""
    c1 = cin if layers == 2 else cout
    spec = [("cnn_layers.0.weight", (c1, cin, 1, 1)), ("cnn_layers.0.bias", (c1,))]
    if layers == 2:
        spec += [("cnn_layers.1.weight", (cout, c1, 1, 1)), ("cnn_layers.1.bias", (cout,))]
    return spec


def seeded_params(seed, cin, cout, layers):
    """float32 parameters in state_dict order, shaped as state_dict_spec"""
    rng = np.random.default_rng(seed)
    out = []
    for _, shape in state_dict_spec(cin, cout, layers):
        fan = shape[1] if len(shape) == 4 else 4
        out.append((rng.integers(-1000, 1001, size=shape) / (1000.0 * np.sqrt(fan))).astype(np.float32))
    return out


def seeded_x_q(name, N, cin, H, W):
    return np.random.default_rng(X_SEED[name]).integers(0, 4 * QUANT_X, size=(N, cin, H, W)).astype(np.uint16)


def x_from_q(x_q):
    return x_q.astype(np.float32) / np.float32(QUANT_X)


def y_from_q(y_q):
    return y_q.astype(np.float32) / np.float32(QUANT_Y)


@contextlib.contextmanager
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def forward(params, x):
    """params: tensors in state_dict order, of x's dtype"""
    for i in range(0, len(params), 2):
        x = F.conv2d(x, params[i], params[i + 1])
    return x


def loss_fn(name):
    return {"l1": F.l1_loss, "mse": F.mse_loss}[name]


def run(params, x, y, loss, dtype):
    """forward, loss and autograd of the restatement on the CPU in ``dtype`` -> dict(pred, loss, grads, differences), numpy.
    One thread: the order of torch's float32 sums, and with it their last bits, must not depend on the machine's core count."""
    with one_thread():
        return _run(params, x, y, loss, dtype)


def _run(params, x, y, loss, dtype):
    ps = [torch.from_numpy(np.asarray(p)).to(dtype).requires_grad_(True) for p in params]
    xt, yt = torch.from_numpy(np.asarray(x)).to(dtype), torch.from_numpy(np.asarray(y)).to(dtype)
    pred = forward(ps, xt)
    val = loss_fn(loss)(pred, yt)
    val.backward()
    return dict(pred=pred.detach().numpy(), loss=val.detach().numpy().reshape(()), grads=[p.grad.numpy() for p in ps],
                differences=(pred.detach() - yt).numpy())


def targets_q(pred64, seed):
    """y = pred64 + s u with u in [0.0102, 0.2098] and a random sign s, rounded to counts of 1 / QUANT_Y: every element keeps
    |pred64 - y| >= 0.01, so the sign of pred - y is never a rounding draw"""
    rng = np.random.default_rng(seed + 500)
    u = 0.0102 + (0.2098 - 0.0102) * rng.integers(0, 10001, size=pred64.shape) / 10000.0
    s = 2.0 * rng.integers(0, 2, size=pred64.shape) - 1.0
    y_q = np.round((pred64 + s * u) * QUANT_Y)
    assert np.abs(y_q).max() < 32767
    y_q = y_q.astype(np.int16)
    assert np.abs(pred64 - y_q / QUANT_Y).min() >= 0.01
    return y_q


def build_case(name):
    """a case from its seeds alone: params, x, y (float32 numpy; y from this module's own float64 forward)"""
    c = CASES[name]
    params = seeded_params(c["seed"], c["cin"], c["cout"], c["layers"])
    x = x_from_q(seeded_x_q(c["x"], c["N"], c["cin"], c["H"], c["W"]))
    pred64 = run(params, x, np.zeros((c["N"], c["cout"], c["H"], c["W"]), np.float32), "mse", torch.float64)["pred"]
    out = dict(c)
    out.update(params=params, x=x, y=y_from_q(targets_q(pred64, c["seed"])))
    return out


def oracle(case):
    """{loss: {"f64": run(...), "f32": run(...)}} of a case on the CPU"""
    return {ls: {"f64": run(case["params"], case["x"], case["y"], ls, torch.float64),
                 "f32": run(case["params"], case["x"], case["y"], ls, torch.float32)} for ls in LOSSES}


def load_g14(path=os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_regression.npz")):
    """tests/golden/g14_regression.npz (see make_golden_regression.py) unpacked.  Per stored case ``n``: g[n] = dict(params, x, y,
    keys, shapes, and per loss {"f64": .., "f32": ..} with loss, grads (state_dict order) and, for the small cases, pred and
    differences).  g["feature"] = the learned-feature tiles."""
    z = np.load(path)
    g = {}
    for n in STORED:
        c = dict(CASES[n])
        keys = [str(k) for k in z[f"{n}_keys"]]
        c["keys"], c["shapes"] = keys, [tuple(int(v) for v in z[f"{n}_shape{i}"]) for i in range(len(keys))]
        c["params"] = [z[f"{n}_p{i}"] for i in range(len(keys))]
        c["x"], c["y"] = x_from_q(z[f"{c['x']}_x_q"]), y_from_q(z[f"{n}_y_q"])
        for ls in LOSSES:
            c[ls] = {}
            for tag in ("f32", "f64"):
                r = dict(loss=z[f"{n}_{ls}_{tag}_loss"], grads=[z[f"{n}_{ls}_{tag}_g{i}"] for i in range(len(keys))])
                c[ls][tag] = r
        if f"{n}_f32_pred" in z:
            pred = {"f32": z[f"{n}_f32_pred"], "f64": z[f"{n}_f64_pred"]}
            for ls in LOSSES:
                for tag in ("f32", "f64"):
                    c[ls][tag]["pred"] = pred[tag]
                    c[ls][tag]["differences"] = z[f"{n}_{tag}_differences"]
        g[n] = c
    feat = dict(params=[z["feature_p0"], z["feature_p1"]], names=[str(k) for k in z["feature_names"]])
    for n in feat["names"]:
        feat[f"{n}_bands"] = z[f"feature_{n}_bands_q"].astype(np.float32) / np.float32(QUANT_X)
        feat[f"{n}_target"] = z[f"feature_{n}_target_q"].astype(np.float32) / np.float32(QUANT_X)
        feat[f"{n}_f32"], feat[f"{n}_f64"] = z[f"feature_{n}_f32"], z[f"feature_{n}_f64"]
    g["feature"] = feat
    return g


def rel_err(got, want):
    """max |got - want| relative to max |want| (1 if want is all zero)"""
    want = np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / (scale if scale > 0 else 1.0))
