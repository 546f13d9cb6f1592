"""``EMITDataModule``: fake EMIT scenes on disk -> items in the AVIRIS value range, bit-equal to the numpy restatement of the
reference's per-item arithmetic (emit_dataset.py:80-105), and ``run_validation`` over its test loader."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emit_scene_util import write_scene  # noqa: E402
from starcop_amd import baselines, emit_data, validation  # noqa: E402
from starcop_amd.model_module import Settings  # noqa: E402

INPUTS = ["mag1c", "TOA_AVIRIS_640nm", "TOA_AVIRIS_550nm", "TOA_AVIRIS_460nm"]
DEFAULTS = dict(MAGIC_DIV_BY=240., RGB_DIV_BY=20., MAGIC_CLIP_TO=[0., 2.], RGB_CLIP_TO=[0., 2.], MAGIC_MULT_BY=1750., RGB_MULT_BY=60.)


def _settings(input_products=INPUTS):
    return Settings(products_plot=["rgb_aviris", "mag1c", "label", "pred"], dataloader=dict(batch_size=1, num_workers=0),
                    dataset=dict(input_products=list(input_products), output_products=["labelbinary"], use_weight_loss=True,
                                 weight_loss="weight_mag1c", weight_sampling=False),
                    model=dict(model_mode="segmentation_output"))


def _scene(rng, shape, plume_px):
    rgb = rng.uniform(-2, 50, (3,) + shape).astype(np.float32)        # below 0 and above 2 * 20: both clip bounds are hit
    rgb[:, 3:6, 10:14] = np.nan
    rgb[1, 40, 50] = np.inf
    magic = rng.normal(0, 60, shape).astype(np.float32)
    label = np.zeros(shape, np.uint8)
    side = int(round(plume_px ** 0.5))
    label[8:8 + side, 12:12 + side] = 255
    magic += (label > 0) * np.float32(400)
    magic[60, 3] = np.nan
    return rgb, magic, label


@pytest.fixture(scope="module")
def scenes(tmp_path_factory, hip):
    root = tmp_path_factory.mktemp("emit")
    rng = np.random.default_rng(8)
    a = _scene(rng, (70, 101), 1600)
    b = _scene(rng, (64, 96), 0)
    write_scene(root, "plume_events", "EMIT_A", a[0], a[1], a[2])
    write_scene(root, "confounders", "EMIT_B", b[0], b[1], None)          # no label file
    return root, [a, b]


def _want_input(rgb, magic, hp, mag1c_only=False):
    """emit_dataset.py:80-105 in numpy: crop, clip(x / DIV, lo, hi) * MULT in float32, into a float32 tensor, nan_to_num"""
    h, w = (magic.shape[0] // 32) * 32, (magic.shape[1] // 32) * 32
    with np.errstate(invalid="ignore"):
        e_magic = np.clip(magic[:h, :w] / hp["MAGIC_DIV_BY"], hp["MAGIC_CLIP_TO"][0], hp["MAGIC_CLIP_TO"][1]) * hp["MAGIC_MULT_BY"]
        e_rgb = np.clip(rgb[:, :h, :w] / hp["RGB_DIV_BY"], hp["RGB_CLIP_TO"][0], hp["RGB_CLIP_TO"][1]) * hp["RGB_MULT_BY"]
    out = np.ones((1 if mag1c_only else 4, h, w), np.float32)
    out[0] = e_magic
    if not mag1c_only:
        out[1:] = e_rgb
    assert out.dtype == np.float32 and e_magic.dtype == np.float32
    return np.nan_to_num(out)


def test_items_match_the_numpy_restatement(scenes):
    root, data = scenes
    module = emit_data.EMITDataModule(_settings(), "label.tif", {}, str(root))
    module.prepare_data()
    ds = module.test_dataset
    assert len(ds) == 2 and len(module.test_dataset_plot) == 2 and module.load_products == "all"
    for idx, (rgb, magic, label) in enumerate(data):
        item = ds[idx]
        assert item["input"].shape == (4, 64, 96) and item["input"].dtype == torch.float32 and item["input"].is_cuda
        assert np.array_equal(item["input"].cpu().numpy(), _want_input(rgb, magic, DEFAULTS))
        assert not torch.isnan(item["input"]).any()
        assert item["output"].shape == (1, 64, 96) and item["weight_loss"].shape == (1, 64, 96)
        assert torch.equal(item["weight_loss"], torch.ones_like(item["output"]))
        assert item["id"] == [idx] and item["debug_rgb_path"][0].endswith("_radiance_RGB")
    # integer labels give a float64 output (label / 255.), the zeros that stand in for a missing label are float32 like the magic band
    a, b = ds[0], ds[1]
    assert a["output"].dtype == torch.float64 and np.array_equal(a["output"][0].cpu().numpy(), data[0][2][:64, :96] / 255.)
    assert a["has_plume"] == [True] and float(a["output"].max()) == 1.0
    assert b["output"].dtype == torch.float32 and not b["output"].any() and b["has_plume"] == [False]


def test_mag1c_only_and_hyperparams(scenes):
    root, data = scenes
    solo = emit_data.EMITDataModule(_settings(["mag1c"]), "label.tif", {}, str(root))
    solo.prepare_data()
    assert solo.load_products == "mag1c_only"
    item = solo.test_dataset[0]
    assert item["input"].shape == (1, 64, 96)
    assert np.array_equal(item["input"].cpu().numpy(), _want_input(data[0][0], data[0][1], DEFAULTS, mag1c_only=True))
    hp = dict(MAGIC_DIV_BY=300., RGB_DIV_BY=16., MAGIC_CLIP_TO=[0.1, 1.5], RGB_CLIP_TO=[0.05, 1.0], MAGIC_MULT_BY=1000., RGB_MULT_BY=90.)
    tuned = emit_data.EMITDataModule(_settings(), "label.tif", hp, str(root))
    tuned.prepare_data()
    for idx, (rgb, magic, _) in enumerate(data):
        got = tuned.test_dataset[idx]["input"].cpu().numpy()
        assert np.array_equal(got, _want_input(rgb, magic, hp))
        assert not np.array_equal(got, _want_input(rgb, magic, DEFAULTS))
    # another labels file name: none present -> every scene is a no-plume scene
    other = emit_data.EMITDataModule(_settings(), "label_released.tif", {}, str(root))
    other.prepare_data()
    assert other.test_dataset[0]["has_plume"] == [False]


def test_run_validation_over_the_test_dataloader(scenes, tmp_path_factory):
    """run_validation aggregates by (has_plume, difficulty) and needs a scene of each group: the two scenes (an "easy" plume and
    a scene without a label) plus a third with a small plume"""
    import shutil
    root, data = scenes
    root3 = tmp_path_factory.mktemp("emit3")
    for kind in ("plume_events", "confounders"):
        shutil.copytree(str(root / kind), str(root3 / kind))
    c = _scene(np.random.default_rng(9), (64, 96), 100)
    write_scene(root3, "plume_events", "EMIT_C", c[0], c[1], c[2])
    module = emit_data.EMITDataModule(_settings(), "label.tif", {}, str(root3))
    module.prepare_data()
    loader = module.test_dataloader()
    assert len(loader) == 3 and loader.batch_size == 1 and loader.dataset is module.test_dataset
    batch = next(iter(loader))
    assert batch["input"].shape == (1, 4, 64, 96) and batch["output"].shape == (1, 1, 64, 96)
    model = baselines.Mag1cBaseline(INPUTS).to("cuda")
    table, metrics = validation.run_validation(model, loader, verbose=False, show_plots=False)
    assert len(table) == 3 and int(metrics["confusion_matrix"].sum()) == 3 * 64 * 96
    assert list(table["label_pixels_plume"]) == [1600, 100, 0] and metrics["recall"] > 0.9
