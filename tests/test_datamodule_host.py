"""Host side of the data modules (no GPU): the raw-product list, the raw / feature split, ``load_dataframe``, the tiled
table's columns and CSV round trip, and ``load_emit_dataset`` / ``load_data`` on a fake folder tree."""
import json
import os

import numpy as np
import pandas as pd

from emit_scene_util import write_scene
from starcop_amd import datamodule as dm, emit_data, features
from starcop_amd.model_module import Settings

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raw_bands_available.json")


def _settings(root, inputs, weight_loss="weight_mag1c"):
    return Settings(products_plot=["rgb_aviris"], dataloader=dict(batch_size=2, num_workers=0),
                    dataset=dict(input_products=list(inputs), output_products=["labelbinary"], training_size=(64, 64),
                                 training_size_overlap=(32, 32), root_folder=str(root), train_csv="train_easy.csv",
                                 use_weight_loss=weight_loss is not None, weight_loss=weight_loss, weight_sampling=True),
                    model=dict(model_mode="segmentation_output"))


def test_raw_bands_available_matches_the_recorded_names():
    names = features.raw_bands_available()
    assert names == json.load(open(GOLDEN))
    assert len(names) == 425 + 3 + 8 + 26 + 3 and names[0] == "TOA_AVIRIS_376nm" and names[-3:] == ["mag1c", "labelbinary", "label_rgba"]
    assert "TOA_AVIRIS_640nm" in names and "TOA_WV3_SWIR8" in names and "TOA_S2B_B8A" in names and "weight_mag1c" not in names


def test_products_split_into_raw_bands_and_features(tmp_path):
    inputs = ["mag1c", "TOA_AVIRIS_640nm", "ratio_wv3_B7_B5_varon21_sum_c_out", "TOA_WV3_SWIR1"]
    module = dm.Permian2019DataModule(_settings(tmp_path, inputs))
    raw, feats = module.split_products()
    assert raw == ["mag1c", "TOA_AVIRIS_640nm", "TOA_WV3_SWIR1", "labelbinary"]
    assert feats == ["ratio_wv3_B7_B5_varon21_sum_c_out", "weight_mag1c"] and all(f in features.FEATURES for f in feats)
    off = dm.Permian2019DataModule(_settings(tmp_path, ["mag1c"], weight_loss=None))
    assert off.weight_loss is None and off.split_products() == (["mag1c", "labelbinary"], [])
    assert off.tiled_csv_path() == os.path.join(str(tmp_path), "train_easy_tiled_64_64.csv")
    assert (off.batch_size, off.num_workers, off.training_size_overlap, off.test_csv) == (2, 0, (32, 32), "test.csv")


def _table(path):
    rows = [{"id": f"s{i}", "name": f"ang{i}", "has_plume": bool(i % 2), "qplume": 100.0 * i, "window_col_off": 0,
             "window_row_off": 0, "window_width": 128, "window_height": 96} for i in range(3)]
    pd.DataFrame(rows).to_csv(path, index=False)


def test_load_dataframe(tmp_path):
    _table(tmp_path / "train_easy.csv")
    module = dm.Permian2019DataModule(_settings(tmp_path, ["mag1c"]))
    df = module.load_dataframe(str(tmp_path / "train_easy.csv"))
    assert df.index.name == "id" and list(df.index) == ["s0", "s1", "s2"]
    assert list(df["folder"]) == [os.path.join(str(tmp_path), f"s{i}") for i in range(3)]
    w = df["window"].iloc[1]
    assert isinstance(w, dm.Window) and w == (0, 0, 96, 128) and (w.row_off, w.col_off, w.height, w.width) == (0, 0, 96, 128)


class _Labels:
    """what ``tiled_dataframe`` needs of a tile set, with the label sums taken on the host"""
    def __init__(self, y):
        self.outputs, self.shape = y, tuple(y.shape[-2:])


def test_tiled_table_columns_and_round_trip(tmp_path, monkeypatch):
    _table(tmp_path / "train_easy.csv")
    module = dm.Permian2019DataModule(_settings(tmp_path, ["mag1c"]))
    df = module.load_dataframe(str(tmp_path / "train_easy.csv"))
    df["tile"] = np.arange(3)
    import torch
    y = torch.zeros((3, 1, 96, 128))
    y[1, 0, 10:50, 20:90] = 1

    def host_sums(labels, wins):          # the kernel's contract, on the host
        return torch.stack([labels[:, r:r + h, c:c + w].double().sum((1, 2)) for (r, c, h, w) in wins], 1)
    monkeypatch.setattr(dm, "tile_window_sums", host_sums)
    tiled = dm.tiled_dataframe(df, _Labels(y), (64, 64), (32, 32))
    wins = dm.create_windows((96, 128), (64, 64), (32, 32))
    assert len(wins) == 2 * 3 and len(tiled) == 3 * 6 and tiled.index.name == "id"
    assert set(tiled.columns) == {"name", "has_plume", "qplume", "folder", "tile", "window"} | set(dm.TILED_COLUMNS)
    assert tiled.index[7] == "s1_r0_c32_w64_h64" and tiled["id_original"].iloc[7] == "s1" and tiled["qplume"].iloc[7] == 100.0
    assert tiled["frac_positives"].iloc[7] == float(y[1, 0, 0:64, 32:96].sum()) / 4096 and bool(tiled["has_plume"].iloc[7])
    assert not tiled["has_plume"].iloc[:6].any()                      # has_plume is the window's, not the sample's
    path = tmp_path / "tiled.csv"
    tiled[[c for c in tiled.columns if c not in ("window", "tile")]].to_csv(path)
    back = pd.read_csv(path)
    assert list(back.columns) == ["id", "name", "has_plume", "qplume", "folder", "frac_positives", "window_col_off", "window_row_off",
                                  "window_width", "window_height", "id_original"]
    back = dm._add_windows(back).set_index("id")
    assert list(back["window"]) == list(tiled["window"]) and list(back.index) == list(tiled.index)
    for col in ("frac_positives", "has_plume", "id_original", "qplume", "window_row_off", "window_col_off"):
        assert list(back[col]) == list(tiled[col]), col


def test_load_emit_dataset_and_load_data(tmp_path):
    rng = np.random.default_rng(0)
    rgb = rng.uniform(0, 30, (3, 40, 50)).astype(np.float32)
    magic = rng.normal(0, 50, (40, 50)).astype(np.float32)
    label = np.zeros((40, 50), np.uint8)
    label[4:9, 5:20] = 255
    write_scene(tmp_path, "plume_events", "EMIT_P1", rgb, magic, label)
    write_scene(tmp_path, "plume_events", "EMIT_P0", rgb + 1, magic + 1, label, labels_name="label_released.tif")
    write_scene(tmp_path, "confounders", "EMIT_N0", rgb + 2, magic + 2)
    (tmp_path / "plume_events" / "notes.txt").write_text("not a scene folder")
    paths = emit_data.load_emit_dataset(str(tmp_path))
    assert [os.path.basename(p[0]) for p in paths] == ["EMIT_P0_radiance_RGB", "EMIT_P1_radiance_RGB", "EMIT_N0_radiance_RGB"]
    assert [os.path.basename(p[1]) for p in paths] == ["EMIT_P0_radiance_magic", "EMIT_P1_radiance_magic", "EMIT_N0_radiance_magic"]
    assert [p[2] is not None for p in paths] == [False, True, False] and paths[1][2].endswith("label.tif")
    assert [p[2] is not None for p in emit_data.load_emit_dataset(str(tmp_path), labels_name="label_released.tif")] == [True, False, False]
    data = emit_data.load_data(paths)
    assert np.array_equal(data[1][0], rgb) and np.array_equal(data[1][1], magic) and np.array_equal(data[1][2], label)
    assert data[1][2].dtype == np.uint8 and data[1][3] == paths[1][0]
    assert data[0][2].dtype == np.float32 and not data[0][2].any() and data[0][2].shape == (40, 50)
    only = emit_data.load_data(paths, "mag1c_only")
    assert len(only[2]) == 3 and np.array_equal(only[2][0], magic + 2) and only[2][2] == paths[2][0]
    ds = emit_data.STARCOPEMITDataset(only, ["mag1c"], ["labelbinary"])
    assert len(ds) == 3 and ds.load_products == "mag1c_only"
    ds.add_extra_products(["mag1c", "rgb"])
    assert ds.extra_products == ["rgb"]


def test_run_validation_accepts_collated_scene_ids():
    """the EMIT loader hands ``id`` over as torch's collate does, a one-element list of a host tensor: it must serve as a row label"""
    import torch
    rows = [{"id": torch.tensor([i]), "v": i} for i in range(3)]
    assert list(pd.DataFrame(rows).set_index("id")["v"]) == [0, 1, 2]
