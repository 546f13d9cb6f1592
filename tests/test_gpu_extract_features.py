"""extract_features (feature_extration.py:249-286) end to end: raw WV3 sample folders -> cached product GeoTIFFs -> load_tileset ->
one fused train step, and SanchezBaseline on the written product."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mlr_util import wv3_tile  # noqa: E402

DEV = "cuda"
SANCHEZ = ["ratio_wv3_B7_B7MLR_SanchezGarcia22_sum_c_out", "ratio_wv3_B8_B8MLR_SanchezGarcia22_sum_c_out", "TOA_WV3_SWIR1"]
GEO = {33550: (12, (3.7, 3.7, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 500000.0, 4100000.0, 0.0)),
       34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32611))}


def _folders(tmp_path, n, H, W):
    from starcop_amd import io_formats as io
    rng = np.random.default_rng(30)
    out = []
    for i in range(n):
        d = tmp_path / f"wv3_{i:03d}"
        d.mkdir()
        b7, t7 = wv3_tile(rng, H, W, k=5)
        _, t8 = wv3_tile(rng, H, W, k=5)
        swir = {1: b7[0], 2: b7[1], 3: 0.5 * (b7[1] + b7[2]), 4: b7[2], 5: b7[3], 6: b7[4], 7: t7, 8: t8}
        for j, a in swir.items():
            io.write_tiff(str(d / f"TOA_WV3_SWIR{j}.tif"), a.astype(np.float32), extra_tags=GEO)
        mag = np.clip(rng.normal(0, 400, (H, W)), 0, None).astype(np.float32)
        mag[H // 3:H // 3 + 30, W // 4:W // 4 + 40] += 1500
        io.write_tiff(str(d / "mag1c.tif"), mag, extra_tags=GEO)
        io.write_tiff(str(d / "labelbinary.tif"), (mag > 900).astype(np.uint8), extra_tags=GEO)
        out.append(str(d))
    return out


def test_extract_features_end_to_end(hip, tmp_path):
    import pandas as pd
    from starcop_amd import features, io_formats as io, model_module as mm
    from starcop_amd.baselines import SanchezBaseline
    folders = _folders(tmp_path, 3, 256, 256)
    prods = [p for p in SANCHEZ if p.startswith("ratio")] + ["ratio_wv3_B8_B8MLR_SanchezGarcia22_simplediv", "weight_mag1c"]
    df = pd.DataFrame({"folder": folders})
    features.extract_features(prods, df, batch_size=2, device=DEV)
    mtimes = {}
    for d in folders:
        for p in prods:
            path = os.path.join(d, f"{p}.tif")
            info = io.tiff_info(path)
            assert all(info.tags[t] == v for t, v in GEO.items()), (p, "georeferencing")
            assert f'role="description">{p}<' in info.tags[42112][1][0]
            got = io.read_tiff(path)
            assert got.shape == (1, 256, 256) and got.dtype == np.float32
            ins = torch.from_numpy(io.load_sample(d, features.FEATURES[p]["inputs"])).to(DEV)
            want = features.FEATURES[p]["function"](*[ins[i:i + 1] for i in range(ins.shape[0])]).cpu().numpy()
            assert np.array_equal(got, want), (d, p)
            mtimes[path] = os.stat(path).st_mtime_ns
    features.extract_features(prods, df, device=DEV)
    assert all(os.stat(p).st_mtime_ns == t for p, t in mtimes.items())

    ts = io.load_tileset(folders, SANCHEZ, ("labelbinary",), "weight_mag1c", device=DEV)
    assert ts.inputs.shape == (3, 3, 256, 256)
    settings = mm.default_settings(pos_weight=15)
    settings.dataset["input_products"] = list(SANCHEZ)
    torch.manual_seed(0)
    model = mm.ModelModule(settings).to(DEV).train()
    opt = model.configure_optimizers()["optimizer"]
    batch = {"input": ts.inputs[:2, :, :128, :128].contiguous(), "output": ts.outputs[:2, :, :128, :128].contiguous(),
             "weight_loss": ts.weight_loss[:2, :, :128, :128].contiguous()}
    loss = float(model.fused_train_step(batch, opt).item())
    assert np.isfinite(loss)

    base = SanchezBaseline(SANCHEZ).to(DEV)
    out = base.batch_with_preds({"input": ts.inputs, "output": ts.outputs})
    assert out["pred_binary"].shape == (3, 1, 256, 256)
    assert torch.equal(out["prediction"], out["input_norm"][:, 1:2])
