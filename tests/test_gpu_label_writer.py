"""write_label_masks (sampling_dataset.py:453-460, proposed_mask cached as labelbinary.tif) end to end: sample folders holding
mag1c.tif and a 4-band label_rgba.tif -> labelbinary.tif (checked against the scipy restatement) -> load_tileset -> one fused
train step."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import labels_util as lu  # noqa: E402

DEV = "cuda"
GEO = {33550: (12, (3.7, 3.7, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 500000.0, 4100000.0, 0.0)),
       34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32611))}
NODATA = {42113: (2, ("-9999",))}
RGB = ("TOA_AVIRIS_640nm", "TOA_AVIRIS_550nm", "TOA_AVIRIS_460nm")


def _folders(tmp_path, shapes, seed=40):
    from starcop_amd import io_formats as io
    rng = np.random.default_rng(seed)
    out = []
    for i, (H, W) in enumerate(shapes):
        d = tmp_path / f"ang_{i:03d}"
        d.mkdir()
        mag, rgba = lu.plume_field(rng, H, W, blobs=6, nan_frac=0.0)
        io.write_tiff(str(d / "mag1c.tif"), np.clip(mag, 0, None).astype(np.float32), extra_tags={**GEO, **NODATA})
        io.write_tiff(str(d / "label_rgba.tif"), rgba, extra_tags=GEO)
        io.write_tiff(str(d / "weight_mag1c.tif"), np.ones((1, H, W), np.float32), extra_tags=GEO)
        for band in RGB:
            io.write_tiff(str(d / f"{band}.tif"), rng.uniform(5, 100, (1, H, W)).astype(np.float32), extra_tags=GEO)
        out.append(str(d))
    return out


def test_write_label_masks_end_to_end(hip, tmp_path):
    import pandas as pd
    from starcop_amd import io_formats as io, mask_creation as mc, model_module as mm
    folders = _folders(tmp_path, [(256, 256)] * 3 + [(130, 200)])
    df = pd.DataFrame({"folder": folders})
    mc.write_label_masks(df, batch_size=2, device=DEV)
    mtimes = {}
    for d in folders:
        path = os.path.join(d, "labelbinary.tif")
        info = io.tiff_info(path)
        assert info.dtype == np.uint8 and info.block == (128, 128)
        assert all(info.tags[t] == v for t, v in GEO.items()), "georeferencing"
        assert 42113 not in info.tags                                     # no nodata value (fill_value_default=None)
        assert 'role="description">labelbinary<' in info.tags[42112][1][0]
        got = io.read_tiff(path)
        want = lu.proposed_mask(io.read_tiff(os.path.join(d, "label_rgba.tif")), io.read_tiff(os.path.join(d, "mag1c.tif")))
        assert got.shape == (1,) + want.shape and np.array_equal(got[0], want.astype(np.uint8)), d
        mtimes[path] = os.stat(path).st_mtime_ns
    assert sum(int(io.read_tiff(p).sum()) for p in mtimes) > 0
    # a second call writes nothing; overwrite=True rewrites every file
    mc.write_label_masks(df, device=DEV)
    assert all(os.stat(p).st_mtime_ns == t for p, t in mtimes.items())
    for p in mtimes:
        os.utime(p, ns=(1, 1))
    mc.write_label_masks(df, overwrite=True, device=DEV)
    assert all(os.stat(p).st_mtime_ns != 1 for p in mtimes)

    # the written targets feed a training step
    same = folders[:3]
    settings = mm.default_settings(pos_weight=15)
    ts = io.load_tileset(same, settings.dataset["input_products"], ("labelbinary",), "weight_mag1c", device=DEV)
    assert ts.outputs.shape == (3, 1, 256, 256)
    assert set(torch.unique(ts.outputs).tolist()) == {0.0, 1.0}
    torch.manual_seed(0)
    model = mm.ModelModule(settings).to(DEV).train()
    opt = model.configure_optimizers()["optimizer"]
    batch = {"input": ts.inputs[:2, :, :128, :128].contiguous(), "output": ts.outputs[:2, :, :128, :128].contiguous(),
             "weight_loss": ts.weight_loss[:2, :, :128, :128].contiguous()}
    loss = float(model.fused_train_step(batch, opt).item())
    assert np.isfinite(loss)


def test_write_label_masks_errors(hip, tmp_path):
    import pandas as pd
    from starcop_amd import io_formats as io, mask_creation as mc
    folders = _folders(tmp_path, [(64, 64), (64, 64)])
    os.remove(os.path.join(folders[1], "label_rgba.tif"))
    with pytest.raises(FileNotFoundError, match="label_rgba"):
        mc.write_label_masks(pd.DataFrame({"folder": folders}), device=DEV)
    assert not any(os.path.exists(os.path.join(d, "labelbinary.tif")) for d in folders)     # nothing written before the check
    io.write_tiff(os.path.join(folders[1], "label_rgba.tif"), np.zeros((4, 64, 80), np.uint8), extra_tags=GEO)
    with pytest.raises(ValueError, match="label_rgba"):
        mc.write_label_masks(pd.DataFrame({"folder": folders}), device=DEV)
    assert not any(os.path.exists(os.path.join(d, "labelbinary.tif")) for d in folders)
    os.remove(os.path.join(folders[0], "mag1c.tif"))
    with pytest.raises(FileNotFoundError, match="mag1c"):
        mc.write_label_masks(pd.DataFrame({"folder": folders[:1]}), device=DEV)
