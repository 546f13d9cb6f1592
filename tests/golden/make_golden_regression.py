"""Generates tests/golden/g14_regression.npz by IMPORTING THE REFERENCE ITSELF (starcop/models/architectures/baselines.py,
starcop/models/utils/losses.py, starcop/data/feature_extration.py).

Run in the build container only (needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_regression.py

For the seeded cases of tests/regression_util.py (STORED) it runs the reference's SimpleCNN_v2 / SimpleCNN_v3 with losses.l1 and
losses.mse on the CPU in float32 and in float64 and stores: the state_dict key lists and shapes, the parameters, both losses and
every parameter gradient, and for the small cases the predictions and ``differences``.  The targets are y = pred64 + s u
(regression_util.targets_q).  It also stores use_pretrained_model_b1to6_b8 of a seeded 6 -> 1 model on two WV3-like tiles
(tests/mlr_util.py), one with a zero border.  Only DATA is written (read it with regression_util.load_g14): inputs as uint16
counts of 2^-14, targets as int16 counts of 2^-12.
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(OUT))
sys.modules.setdefault("rasterio", types.ModuleType("rasterio"))

from starcop.models.architectures.baselines import SimpleCNN_v2, SimpleCNN_v3  # noqa: E402
from starcop.models.utils import losses  # noqa: E402
from starcop.data import feature_extration as ref_feat  # noqa: E402
import regression_util as ru  # noqa: E402
from mlr_util import wv3_tile  # noqa: E402

SMALL = ("D", "mini_v2", "mini_v3")


def ref_model(c, params, dtype):
    m = (SimpleCNN_v3 if c["layers"] == 2 else SimpleCNN_v2)(c["cin"], c["cout"])
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == ru.state_dict_spec(c["cin"], c["cout"], c["layers"])
    m.load_state_dict({k: torch.from_numpy(p) for k, p in zip(sd, params)})
    return m.to(dtype)


def ref_run(c, params, x, y, loss, dtype):
    m = ref_model(c, params, dtype)
    xt, yt = torch.from_numpy(x).to(dtype), torch.from_numpy(y).to(dtype)
    pred = m(xt)
    val = getattr(losses, loss)(pred, yt)
    val.backward()
    return dict(pred=pred.detach().numpy(), loss=val.detach().numpy().reshape(()), grads=[p.grad.numpy() for p in m.parameters()],
                differences=(pred.detach() - yt).numpy())


def feature(data):
    rng = np.random.default_rng(1420)
    params = [(rng.integers(50, 301, size=(1, 6, 1, 1)) / 1000.0).astype(np.float32), np.array([0.02], np.float32)]
    data["feature_p0"], data["feature_p1"] = params
    tiles = {"plain": wv3_tile(rng, 48, 56, k=6, border=0), "border": wv3_tile(rng, 40, 44, k=6, border=4)}
    c = dict(cin=6, cout=1, layers=1)

    class _Model(SimpleCNN_v2):
        device = torch.device("cpu")

    for name, (b, t) in tiles.items():
        b_q, t_q = np.round(b * ru.QUANT_X).astype(np.uint16), np.round(t * ru.QUANT_X).astype(np.uint16)
        data[f"feature_{name}_bands_q"], data[f"feature_{name}_target_q"] = b_q, t_q
        bands, target = b_q.astype(np.float32) / np.float32(ru.QUANT_X), t_q.astype(np.float32) / np.float32(ru.QUANT_X)
        m = _Model(6, 1)
        m.load_state_dict(ref_model(c, params, torch.float32).state_dict())
        ref_feat.model_preloaded = m
        with np.errstate(invalid="ignore", divide="ignore"):
            f32 = ref_feat.use_pretrained_model_b1to6_b8(*[bands[j][None] for j in range(6)], target[None])
            # the same lines (feature_extration.py:163-174) with a float64 forward
            out64 = ref_model(c, params, torch.float64)(torch.from_numpy(bands[None].astype(np.float64))).detach().numpy()[0][0]
            t64 = target.astype(np.float64)
            f64 = ref_feat.ratio_2c_match_c_from_sums_outlier(t64, out64, zero_value_out=-0.5)
            f64 = np.where(t64 == 0.0, -0.5, f64)
        assert f32.dtype == np.float32 and f32.shape == target.shape
        data[f"feature_{name}_f32"], data[f"feature_{name}_f64"] = f32, f64
    ref_feat.model_preloaded = None
    data["feature_names"] = np.array(list(tiles))


def main():
    torch.set_num_threads(1)          # as regression_util.run: float32 sums in one fixed order
    data = {}
    for name in ru.STORED:
        c = ru.CASES[name]
        params = ru.seeded_params(c["seed"], c["cin"], c["cout"], c["layers"])
        xkey = f"{c['x']}_x_q"
        if xkey not in data:
            data[xkey] = ru.seeded_x_q(c["x"], c["N"], c["cin"], c["H"], c["W"])
        x = ru.x_from_q(data[xkey])
        zeros = np.zeros((c["N"], c["cout"], c["H"], c["W"]), np.float32)
        y_q = ru.targets_q(ref_run(c, params, x, zeros, "mse", torch.float64)["pred"], c["seed"])
        y = ru.y_from_q(y_q)
        data[f"{name}_y_q"] = y_q
        spec = ru.state_dict_spec(c["cin"], c["cout"], c["layers"])
        data[f"{name}_keys"] = np.array([k for k, _ in spec])
        for i, ((_, shape), p) in enumerate(zip(spec, params)):
            data[f"{name}_shape{i}"], data[f"{name}_p{i}"] = np.array(shape, np.int64), p
        for ls in ru.LOSSES:
            for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
                r = ref_run(c, params, x, y, ls, dt)
                data[f"{name}_{ls}_{tag}_loss"] = r["loss"]
                for i, g in enumerate(r["grads"]):
                    data[f"{name}_{ls}_{tag}_g{i}"] = g
                if name in SMALL:
                    data[f"{name}_{tag}_pred"], data[f"{name}_{tag}_differences"] = r["pred"], r["differences"]
    feature(data)
    np.savez_compressed(os.path.join(OUT, "g14_regression.npz"), **data)


if __name__ == "__main__":
    main()
