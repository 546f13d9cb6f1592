"""Host side of the multi-class network: the 13-band, 4-class U-Net and the Sentinel-2 cloud detector built on it
(starcop/sentinel2/models.py) -- state_dict surface, padding arithmetic, argument checks.  No device needed."""
import math

import pytest
import torch

from oracle.unet_ref import UnetMobileNetV2
from starcop_amd import sentinel2
from starcop_amd.network import HyperStarcopUNet


def test_state_dict_surface_equals_the_oracle():
    ref = UnetMobileNetV2(13, 4).state_dict()
    assert len(ref) == 374
    net = HyperStarcopUNet(13, 4)
    sd = net.state_dict()
    assert list(sd) == list(ref)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    assert tuple(sd["encoder.features.0.0.weight"].shape) == (32, 13, 3, 3)
    assert tuple(sd["segmentation_head.0.weight"].shape) == (4, 16, 3, 3)
    cd = sentinel2.CDModel(device="cpu")
    assert not cd.model.training            # (as in the reference, only the inner network is switched to eval mode)
    sdc = cd.state_dict()
    assert set(sdc) == {"model." + k for k in ref}
    for k, v in ref.items():
        assert sdc["model." + k].shape == v.shape and sdc["model." + k].dtype == v.dtype, k
    assert sum(k.endswith("num_batches_tracked") for k in sdc) == sum(k.endswith("num_batches_tracked") for k in ref) == 62
    # the reference's checkpoint layout loads strictly, num_batches_tracked entries included; and back
    cd.load_state_dict({"model." + k: v for k, v in ref.items()}, strict=True)
    assert torch.equal(cd.model.segmentation_head[0].weight, ref["segmentation_head.0.weight"])
    UnetMobileNetV2(13, 4).load_state_dict(net.state_dict(), strict=True)


def test_initialisation_follows_the_oracle():
    """same generator state -> the same parameters as the oracle's reset_parameters (in_channels != 3: the first conv re-drawn)"""
    torch.manual_seed(7)
    ref = UnetMobileNetV2(13, 4).state_dict()
    torch.manual_seed(7)
    sd = HyperStarcopUNet(13, 4).state_dict()
    for k, v in ref.items():
        assert torch.equal(sd[k], v), k
    bound = 1.0 / math.sqrt(13 * 9)         # Conv2d.reset_parameters: kaiming_uniform(a = sqrt(5))
    assert float(sd["encoder.features.0.0.weight"].abs().max()) <= bound


def test_find_padding_is_the_reference_arithmetic():
    import numpy as np

    def reference(v, divisor=8):            # starcop/sentinel2/models.py:20-25
        v_divisible = max(divisor, int(divisor * np.ceil(v / divisor)))
        total_pad = v_divisible - v
        pad_1 = total_pad // 2
        pad_2 = total_pad - pad_1
        return pad_1, pad_2

    for divisor in (8, 32):
        for v in range(1, 101):
            assert tuple(sentinel2.find_padding(v, divisor)) == reference(v, divisor), (v, divisor)


def test_load_weights(tmp_path):
    with pytest.raises(NotImplementedError):
        sentinel2.load_weights("gs://dtacs/experiments_results/atmospheric_correction_lightning/CDmodel.ckpt", map_location="cpu")
    with pytest.raises(ValueError):
        sentinel2.load_weights(str(tmp_path / "missing.ckpt"))
    path = tmp_path / "cd.ckpt"
    sd = sentinel2.CDModel(device="cpu").state_dict()
    torch.save({"state_dict": sd}, path)
    got = sentinel2.load_weights(str(path), map_location="cpu")["state_dict"]
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


def test_constructor_limits():
    with pytest.raises(ValueError):
        HyperStarcopUNet(17, 1)
    with pytest.raises(ValueError):
        HyperStarcopUNet(4, 9)
    with pytest.raises(ValueError):
        HyperStarcopUNet(0, 1)
    with pytest.raises(ValueError):
        HyperStarcopUNet(4, 0)
    assert HyperStarcopUNet(16, 8).segmentation_head[0].weight.shape == (8, 16, 3, 3)
    assert sentinel2.INTERPRETATION_CLOUDSEN12 == ["clear", "Thick cloud", "Thin cloud", "Cloud shadow"]


def test_train_mode_is_refused_at_the_first_forward_not_in_the_constructor():
    """the refusal names the two missing kernels and comes before any device is needed"""
    for cin, k in ((13, 4), (4, 2), (9, 1)):
        net = HyperStarcopUNet(cin, k).train()
        with pytest.raises(NotImplementedError, match="stem weight gradient.*K-class head"):
            net(torch.zeros(1, cin, 32, 32))


def test_cdmodel_checks_the_channel_count():
    import numpy as np
    with pytest.raises(AssertionError, match="Expected 13 channels found 12"):
        sentinel2.CDModel(device="cpu").predict(np.zeros((12, 40, 40), dtype=np.float32))


def test_model_module_with_two_classes_constructs_and_refuses_training():
    """settings.model.num_classes is a configuration value in the reference: such a module builds and takes a state_dict;
    training_step raises the network's NotImplementedError"""
    from starcop_amd import model_module as mm
    model = mm.ModelModule(mm.default_settings(num_classes=2))
    assert model.num_classes == 2 and model.network.segmentation_head[0].weight.shape == (2, 16, 3, 3)
    model.network.load_state_dict(UnetMobileNetV2(4, 2).state_dict(), strict=True)
    model.train()
    batch = {"input": torch.zeros(1, 4, 32, 32), "output": torch.zeros(1, 1, 32, 32), "weight_loss": torch.ones(1, 1, 32, 32)}
    with pytest.raises(NotImplementedError, match="K-class head"):
        model.training_step(batch, 0)
