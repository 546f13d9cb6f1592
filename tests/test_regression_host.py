"""Host side of the regression path (no GPU): tests/regression_util.py reproduces the reference's own outputs
(tests/golden/g14_regression.npz), and SimpleCNN_v2 / SimpleCNN_v3 / ModelModuleRegression / get_model / the learned-feature
registry entry have the reference's surface and fail loudly without a device."""
import numpy as np
import pytest
import torch

import regression_util as ru
from starcop_amd import _lib, features, model_module as mm, model_module_regression as mmr, model_setup
from starcop_amd.pointwise_net import SimpleCNN_v2, SimpleCNN_v3


@pytest.fixture(scope="module")
def g():
    return ru.load_g14()


def _settings(model_type="cnn_v2", loss="l1", mode="regression_output", n_in=13, n_out=12):
    s = mm.default_settings(model_mode=mode, model_type=model_type, loss=loss, num_classes=n_out)
    s.dataset.input_products = [f"TOA_WV3_SWIR{i % 8 + 1}" for i in range(n_in)]
    s.dataset.output_products = ["TOA_WV3_SWIR8"]
    return s


def _ulp_close(a, b):
    """float32 arrays equal exactly or to one ulp of the larger magnitude of the pair"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool((np.abs(a.astype(np.float64) - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all())


def test_restatement_reproduces_the_reference(g):
    for name in ru.STORED:
        c = g[name]
        for ls in ru.LOSSES:
            r64, r32 = ru.run(c["params"], c["x"], c["y"], ls, torch.float64), ru.run(c["params"], c["x"], c["y"], ls, torch.float32)
            want64, want32 = c[ls]["f64"], c[ls]["f32"]
            assert abs(r64["loss"] - want64["loss"]) <= 1e-12 * abs(want64["loss"]), (name, ls)
            assert _ulp_close(r32["loss"], want32["loss"]), (name, ls)
            for i, (a, b) in enumerate(zip(r64["grads"], want64["grads"])):
                assert a.shape == b.shape and ru.rel_err(a, b) <= 1e-12, (name, ls, i)
            for i, (a, b) in enumerate(zip(r32["grads"], want32["grads"])):
                # a float32 sum over many pixels: one ulp of the array's largest entry
                assert a.dtype == np.float32 and np.abs(a - b).max() <= np.spacing(np.abs(b).max()), (name, ls, i)
            if "pred" in want64:
                assert ru.rel_err(r64["pred"], want64["pred"]) <= 1e-12 and ru.rel_err(r64["differences"], want64["differences"]) <= 1e-12
                assert _ulp_close(r32["pred"], want32["pred"]), (name, ls)
                assert np.abs(r32["differences"] - want32["differences"]).max() <= np.spacing(np.float32(np.abs(want32["pred"]).max()))


def test_targets_keep_their_distance(g):
    for name in ru.STORED:
        c = g[name]
        pred64 = ru.run(c["params"], c["x"], c["y"], "mse", torch.float64)["pred"]
        assert np.abs(pred64 - c["y"]).min() >= 0.01 - 1e-9, name


def test_state_dict_matches_the_reference(g):
    for name in ru.STORED:
        c = g[name]
        net = (SimpleCNN_v3 if c["layers"] == 2 else SimpleCNN_v2)(c["cin"], c["cout"])
        sd = net.state_dict()
        assert list(sd) == c["keys"] and [tuple(v.shape) for v in sd.values()] == c["shapes"], name
        net.load_state_dict({k: torch.from_numpy(p) for k, p in zip(c["keys"], c["params"])}, strict=True)
        for p, want in zip(net.parameters(), c["params"]):
            assert np.array_equal(p.detach().numpy(), want)
        flat = net.flat_parameters()                     # state_dict order, one buffer
        assert np.array_equal(flat.numpy(), np.concatenate([p.reshape(-1) for p in c["params"]]))
        assert flat.numel() == _lib.load().sc_pwreg_param_floats(c["cin"], net.c1, c["cout"], c["layers"])
        model = mmr.ModelModuleRegression(_settings("cnn_v3" if c["layers"] == 2 else "cnn_v2", n_in=c["cin"], n_out=c["cout"]))
        msd = {k: v for k, v in model.state_dict().items() if k.startswith("network.")}
        assert list(msd) == ["network." + k for k in c["keys"]] and [tuple(v.shape) for v in msd.values()] == c["shapes"]
        model.network.load_state_dict({k: torch.from_numpy(p) for k, p in zip(c["keys"], c["params"])}, strict=True)


def test_defaults_are_the_reference_defaults():
    assert (SimpleCNN_v2().cin, SimpleCNN_v2().cout, SimpleCNN_v3().c1) == (13, 12, 13)


def test_get_model_serves_both_modes():
    m = model_setup.get_model(_settings("cnn_v2"))
    assert type(m) is mmr.ModelModuleRegression and isinstance(m.network, SimpleCNN_v2) and m.inhibit_normalisation is True
    assert type(model_setup.get_model(_settings("cnn_v3")).network) is SimpleCNN_v3
    assert type(model_setup.get_model(mm.default_settings())) is mm.ModelModule


def test_get_model_loads_test_weights(tmp_path, g):
    c = g["mini_v2"]
    s = _settings("cnn_v2")
    (tmp_path / "exp").mkdir()
    ref = mmr.ModelModuleRegression(s)
    ref.network.load_state_dict({k: torch.from_numpy(p) for k, p in zip(c["keys"], c["params"])})
    torch.save(ref.state_dict(), tmp_path / "exp" / "model.pt")
    s.model.test, s.model.model_folder = True, str(tmp_path)
    m = model_setup.get_model(s, "exp")
    assert np.array_equal(m.network.cnn_layers[0].weight.detach().numpy(), c["params"][0])


def test_constructor_contract():
    with pytest.raises(AssertionError):
        mmr.ModelModuleRegression(_settings("cnn_v2", mode="segmentation_output"))
    assert mmr.ModelModuleRegression(_settings(loss="l1")).loss_name == "l1_loss"
    assert mmr.ModelModuleRegression(_settings(loss="mse")).loss_name == "mse_loss"
    with pytest.raises(NotImplementedError, match="cnn_v1"):
        mmr.ModelModuleRegression(_settings("cnn_v1"))
    with pytest.raises(Exception, match="No model implemented for model_type: resnet"):
        mmr.ModelModuleRegression(_settings("resnet"))
    cfg = mmr.ModelModuleRegression(_settings()).configure_optimizers
    assert callable(cfg)
    u = mmr.ModelModuleRegression(_settings("unet_semseg", n_in=4, n_out=1))
    assert type(u.network).__name__ == "HyperStarcopUNet" and (u.network.in_channels, u.network.classes) == (4, 1)
    with pytest.raises(NotImplementedError):             # ModelModule keeps refusing the regression losses
        mm.ModelModule(mm.default_settings(loss="l1"))


def test_channel_limits():
    for bad in (0, 17):
        with pytest.raises(ValueError):
            SimpleCNN_v2(bad, 3)
        with pytest.raises(ValueError):
            SimpleCNN_v3(3, bad)
    lib = _lib.load()
    assert lib.sc_pwreg_param_floats(13, 12, 12, 1) == 13 * 12 + 12
    assert lib.sc_pwreg_param_floats(13, 13, 12, 2) == 13 * 13 + 13 + 13 * 12 + 12
    assert lib.sc_pwreg_param_floats(17, 12, 12, 1) == 0 and lib.sc_pwreg_param_floats(13, 12, 0, 2) == 0
    assert lib.sc_pwreg_param_floats(13, 11, 12, 1) == 0          # one layer: hidden == output
    # the sweep's grid is a function of the pixel count only: one work-group per 512 pixels, at most 512
    assert lib.sc_pwreg_sweep_blocks(1, 5, 3) == 1 and lib.sc_pwreg_sweep_blocks(3, 37, 41) == 9
    assert lib.sc_pwreg_sweep_blocks(16, 512, 512) == 512 and lib.sc_pwreg_sweep_blocks(0, 4, 4) == 0


def test_learned_feature_without_a_model():
    assert features.set_learned_model(None) is None
    fn = features.FEATURES["ratio_lrn_bands2band8only_60ep_512_l1"]["function"]
    assert fn is features.use_pretrained_model_b1to6_b8
    with pytest.raises(NotImplementedError):
        fn()
    with pytest.raises(NotImplementedError, match="gs://"):
        features.set_learned_model("gs://starcop/experiments/wv3_cnn_v2_bands2band8only_60ep_512_l1/final_checkpoint_model.ckpt")
    with pytest.raises(NotImplementedError):             # the refused path set nothing
        fn()


def test_no_cpu_fallback(g):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    c = g["mini_v3"]
    x, y = torch.from_numpy(c["x"]), torch.from_numpy(c["y"])
    net = SimpleCNN_v3(13, 12)
    with pytest.raises(_lib.StarcopHipError):
        net(x)
    model = mmr.ModelModuleRegression(_settings("cnn_v3"))
    batch = {"input": x, "output": y}
    for call in (lambda: model(x), lambda: model.training_step(batch, 0), lambda: model.fused_train_step(batch),
                 lambda: mmr.l1(y, y), lambda: mmr.mse(y, y)):
        with pytest.raises(_lib.StarcopHipError):
            call()
    features.set_learned_model(SimpleCNN_v2(6, 1))
    try:
        with pytest.raises(_lib.StarcopHipError):
            features.use_pretrained_model_b1to6_b8(*[torch.zeros(1, 8, 8)] * 7)
    finally:
        features.set_learned_model(None)
