"""Cutting windows on the GPU: sc_window_cut through the C ABI and WindowDataset end to end against the numpy restatement of
tests/window_cut_util.py (sampling_dataset.py:259-303 of the reference).  Every comparison is equality (NaN equals NaN, the sign of
a zero is not part of the contract), 100 % of the elements, no tolerance."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import window_cut_util as U  # noqa: E402
from hip_ops import DEV  # noqa: E402
from starcop_amd import _lib, aviris, features, io_formats as io, mask_creation, sampling, window_dataset as wd  # noqa: E402

SCENES = ((70, 45), (20, 20))
OUTS = ((32, 32, 0), (16, 30, 0), (5, 7, 0), (32, 32, 4))        # (height, width, byte offset of `out`)
PAD = 64                                                          # guard bytes around `out`


def spec(t, origin=(0, 0), fill=None, scale=None, clip=None, host=None):
    return {"t": t, "origin": origin, "fill": fill, "scale": scale, "clip": clip, "host": host}


def bits_of(value, dt):
    return int(np.array(value, dtype=dt).reshape(1).view(f"u{np.dtype(dt).itemsize}")[0])


def call_abi(hip, specs, offs, out_hw, scene, byte_off=0, offs_dev=None, P=None, elem=None, scene_override=None):
    """one raw sc_window_cut call -> (status, result [n][P][h][w] numpy or None, guard bytes untouched)"""
    dt = specs[0]["t"].dtype
    nd = torch.empty(0, dtype=dt).numpy().dtype
    off = np.ascontiguousarray(np.array(offs, dtype=np.int32).reshape(-1, 2))
    off_d = torch.from_numpy(off if offs_dev is None else np.ascontiguousarray(np.array(offs_dev, dtype=np.int32))).to(DEV)
    n, nP = off.shape[0], len(specs)
    nbytes = n * nP * out_hw[0] * out_hw[1] * nd.itemsize
    buf = torch.full((PAD + byte_off + nbytes + PAD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    a = _lib.sc_wcut_args()
    a.scene_rows, a.scene_cols = scene if scene_override is None else scene_override
    a.out_h, a.out_w = out_hw
    a.P = nP if P is None else P
    a.elem_bytes = nd.itemsize if elem is None else elem
    a.n_win = n
    a.win_off, a.win_off_host = off_d.data_ptr(), off.ctypes.data
    for k in range(min(max(a.P, 0), 64)):
        s = specs[min(k, nP - 1)]
        t = s["t"]
        a.src[k] = t.data_ptr()
        a.row_stride[k], a.col_stride[k] = t.stride()
        a.row0[k], a.col0[k] = s["origin"]
        a.rows[k], a.cols[k] = t.shape
        ops = 0
        if s["fill"] is not None:
            ops |= _lib.WCUT_FILL
            a.fill_bits[k] = bits_of(s["fill"], nd)
        if s["scale"] is not None:
            ops |= _lib.WCUT_SCALE
            a.scale[k] = float(np.float32(s["scale"]))
        if s["clip"] is not None:
            ops |= _lib.WCUT_CLIP
            a.clip_lo[k], a.clip_hi[k] = s["clip"]
        a.ops[k] = ops
    a.out = buf.data_ptr() + PAD + byte_off
    rc = hip.sc_window_cut(a, _lib.stream())
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    lo, hi = PAD + byte_off, PAD + byte_off + nbytes
    guards = bool((raw[:lo] == 0xA5).all() and (raw[hi:] == 0xA5).all())
    if rc != 0:
        return rc, None, guards and bool((raw == 0xA5).all())
    return rc, raw[lo:hi].copy().view(nd).reshape(n, nP, *out_hw), guards


def oracle(specs, offs, out_hw):
    return np.stack([np.stack([U.cut(s["host"], (r, c, *out_hw), s["origin"], s["fill"], s["scale"], s["clip"]) for s in specs])
                     for r, c in offs])


def check(hip, specs, offs, out_hw, scene, byte_off, what):
    rc, got, guards = call_abi(hip, specs, offs, out_hw, scene, byte_off)
    assert rc == 0, (what, hip.sc_last_error())
    want = oracle(specs, offs, out_hw)
    bad = int((~((got == want) | ((got != got) & (want != want)))).sum()) if got.dtype.kind == "f" else int((got != want).sum())
    print(f"{what}: {got.dtype} {got.shape}, mismatching elements {bad} of {got.size}, guards intact {guards}")
    assert guards, what
    assert U.equal(got, want), what
    return got


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def sources():
    """per scene: the host arrays and their device copies, built once"""
    out = {}
    for H, W in SCENES:
        rng = np.random.default_rng(100 * H + W)
        f = {k: U.float_plane(rng, (H, W)) for k in ("toa", "scaled", "mag1c", "nanfill", "plain")}
        f["toa"][3, 5], f["toa"][4, 5] = np.float32(1e30), np.float32(-1e30)          # far beyond both clip bounds
        band_rows = (17, 49) if H == 70 else (5, 14)
        f["band"] = f["plain"][band_rows[0]:band_rows[1]].copy()
        rgba = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        rgba[rng.random((H, W, 4)) < .2] = 255
        i16 = rng.integers(-32768, 32768, (H, W), dtype=np.int16)
        i16[rng.random((H, W)) < .1] = -9999
        cube = rng.standard_normal((H, W, 7)).astype(np.float32)                      # a BIP cube: band = strided plane
        out[(H, W)] = {"f": f, "fd": {k: up(v) for k, v in f.items()}, "band_rows": band_rows, "rgba": rgba, "rgba_d": up(rgba),
                       "i16": i16, "i16_d": up(i16), "cube": cube, "cube_d": up(cube)}
    return out


@pytest.mark.parametrize("out", OUTS, ids=lambda o: f"{o[0]}x{o[1]}+{o[2]}")
@pytest.mark.parametrize("scene", SCENES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bit_equal_to_the_restatement(hip, sources, scene, out):
    S = sources[scene]
    out_hw, byte_off = out[:2], out[2]
    offs = U.windows_for(scene, out_hw)
    f, fd = S["f"], S["fd"]
    s = 3.1 / 100 / 0.08775                      # factor / 100 / solar irradiance, evaluated in float64
    b0 = S["band_rows"][0]
    floats = [spec(fd["toa"], fill=-9999.0, scale=s, clip=(0.0, 2.0), host=f["toa"]),
              spec(fd["scaled"], scale=3.1, host=f["scaled"]),
              spec(fd["mag1c"], fill=-9999.0, clip=(0.0, 10000.0), host=f["mag1c"]),
              spec(fd["nanfill"], fill=float("nan"), scale=0.5, host=f["nanfill"]),
              spec(fd["band"], origin=(b0, 0), fill=-9999.0, clip=(0.0, 2.0), host=f["band"]),
              spec(S["cube_d"][:, :, 3], scale=1.5, host=S["cube"][:, :, 3]),
              spec(fd["plain"][:, 2:scene[1] - 1], origin=(0, 2), host=f["plain"][:, 2:scene[1] - 1])]
    got = check(hip, floats, offs, out_hw, scene, byte_off, "float32, scale / clip")
    outside = [k for k, (r, c) in enumerate(offs) if r + out_hw[0] <= 0 or r >= scene[0] or c + out_hw[1] <= 0 or c >= scene[1]]
    assert len(outside) >= 6 and not got[outside].any()                  # wholly outside: all zeros
    assert np.isnan(got[:, 3]).any() and (got[:, 0] == 2).any() and (got[:, 0] == 0).any()
    # pure data movement: float32 (NaN payloads and -0.0 survive: compared as raw bits), chunky uint8 as four planes, int16
    plain = [spec(fd["plain"], fill=-9999.0, host=f["plain"]), spec(fd["band"], origin=(b0, 0), host=f["band"])]
    got = check(hip, plain, offs, out_hw, scene, byte_off, "float32, pure movement")
    assert np.array_equal(got.view(np.uint32), oracle(plain, offs, out_hw).view(np.uint32))
    rgba = [spec(S["rgba_d"][:, :, k], fill=255 if k == 3 else None, host=S["rgba"][:, :, k]) for k in range(4)]
    assert rgba[0]["t"].stride() == (4 * scene[1], 4)
    check(hip, rgba, offs, out_hw, scene, byte_off, "uint8, chunky (H, W, 4)")
    check(hip, [spec(S["i16_d"], fill=-9999, host=S["i16"])], offs, out_hw, scene, byte_off, "int16")


def test_one_plane_and_sixty_four_planes(hip, sources):
    scene = SCENES[0]
    S = sources[scene]
    offs = U.windows_for(scene, (32, 32))[:9]
    check(hip, [spec(S["fd"]["mag1c"], fill=-9999.0, clip=(0.0, 10000.0), host=S["f"]["mag1c"])], offs, (32, 32), scene, 0, "P = 1")
    names = ("toa", "scaled", "mag1c", "plain")
    many = [spec(S["fd"][names[k % 4]], fill=-9999.0 if k % 3 else None, scale=0.25 * (k + 1) if k % 2 else None,
                 clip=(0.0, float(k + 1)) if k % 5 == 0 else None, host=S["f"][names[k % 4]]) for k in range(64)]
    check(hip, many, offs, (32, 32), scene, 0, "P = 64")
    check(hip, many, offs[:3], (5, 7), scene, 0, "P = 64, element stores")


def test_argument_errors_launch_nothing(hip, sources):
    scene = SCENES[0]
    S = sources[scene]
    offs = [(0, 0), (3, -2)]
    f32 = [spec(S["fd"]["plain"], host=S["f"]["plain"])]
    u8 = [spec(S["rgba_d"][:, :, 0], scale=2.0, host=S["rgba"][:, :, 0])]

    def bad(what, *args, **kw):
        rc, _, untouched = call_abi(hip, *args, **kw)
        msg = hip.sc_last_error().decode()
        print(f"{what}: status {rc}, {msg}")
        assert rc == -1 and untouched, what
        return msg
    assert "scale" in bad("scale at 1 byte", u8, offs, (8, 8), scene)
    assert "P=65" in bad("P = 65", f32, offs, (8, 8), scene, P=65)
    assert "scene" in bad("plane outside the scene", f32, offs, (8, 8), scene, scene_override=(scene[0] - 1, scene[1]))
    assert "scene" in bad("plane origin pushes it outside", [spec(S["fd"]["plain"], origin=(1, 0))], offs, (8, 8), scene)
    assert "differ" in bad("mismatched window tables", f32, offs, (8, 8), scene, offs_dev=[(0, 0), (3, -3)])
    assert "width" in bad("8-byte elements", f32, offs, (8, 8), scene, elem=8)
    with pytest.raises(ValueError):
        wd.window_cut([wd.Plane(S["rgba_d"][:, :, 0], scale=2.0)], offs, (8, 8))
    rc, got, guards = call_abi(hip, f32, offs, (8, 8), scene)
    assert rc == 0 and guards and U.equal(got, oracle(f32, offs, (8, 8)))


def test_two_calls_give_identical_bytes(hip, sources):
    scene = SCENES[0]
    S = sources[scene]
    offs = U.windows_for(scene, (32, 32))
    specs = [spec(S["fd"]["toa"], fill=-9999.0, scale=0.37, clip=(0.0, 2.0), host=S["f"]["toa"]), spec(S["cube_d"][:, :, 5], host=S["cube"][:, :, 5])]
    _, a, _ = call_abi(hip, specs, offs, (32, 32), scene)
    _, b, _ = call_abi(hip, specs, offs, (32, 32), scene)
    assert a.tobytes() == b.tobytes()


def test_python_wrapper(sources):
    scene = SCENES[0]
    S = sources[scene]
    offs = U.windows_for(scene, (16, 30))
    planes = [wd.Plane(S["fd"]["toa"], fill=-9999.0, scale=0.37, clip=(0, 2)), wd.Plane(S["fd"]["nanfill"], fill=float("nan")),
              wd.Plane(S["fd"]["band"], row0=S["band_rows"][0], fill=-9999.0)]
    got = wd.window_cut(planes, offs, (16, 30), scene_shape=scene).cpu().numpy()
    want = oracle([spec(None, fill=-9999.0, scale=0.37, clip=(0, 2), host=S["f"]["toa"]), spec(None, fill=float("nan"), host=S["f"]["nanfill"]),
                   spec(None, origin=(S["band_rows"][0], 0), fill=-9999.0, host=S["f"]["band"])], offs, (16, 30))
    assert U.equal(got, want)
    many = [wd.Plane(S["i16_d"], fill=-9999 if k % 2 else None) for k in range(70)]              # more planes than one launch takes
    got = wd.window_cut(many, offs[:4], (5, 7)).cpu().numpy()
    assert got.shape == (4, 70, 5, 7)
    assert U.equal(got, oracle([spec(None, fill=p.fill, host=S["i16"]) for p in many], offs[:4], (5, 7)))


# ------------------------------------------------------------------------------------------------ end to end
GEO = {33550: (12, (5.0, 5.0, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 600000.0, 3500000.0, 0.0)),
       34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32613))}
FACTORS = (3.4, 2.9)


def make_flightline(folder, shape, seed, envi):
    """mag1c, label_rgba, three simulated bands and the AVIRIS bands (an ENVI cube, or metadata.json + one file per band)"""
    os.makedirs(folder)
    rng = np.random.default_rng(seed)
    H, W = shape
    src = {}
    mag = (rng.random((H, W)) * 900).astype(np.float32)
    mag[H // 3:H // 3 + 12, W // 4:W // 4 + 14] += 2500            # a plume
    mag[rng.random((H, W)) < .05] = -9999
    src["mag1c"] = mag[None]
    rgba = np.zeros((4, H, W), np.uint8)
    rgba[:3] = rng.integers(0, 256, (3, H, W))
    rgba[3, H // 3 + 2:H // 3 + 8, W // 4 + 3:W // 4 + 9] = 255
    src["label_rgba"] = rgba
    for name in ("S2A_B12", "S2B_B1", "WV3_SWIR1"):
        a = (rng.random((H, W)) * 12).astype(np.float32)
        a[rng.random((H, W)) < .05] = -9999
        a[rng.random((H, W)) < .05] = 500                          # clips at 2
        src[name] = a[None]
    for name, a in src.items():
        tags = dict(GEO)
        if a.dtype == np.float32:
            tags[42113] = (2, ("-9999",))
        io.write_tiff(os.path.join(folder, f"{name}.tif"), a, blocksize=128, extra_tags=tags)
    centres = [450.0, 640.0, 2305.0, 2312.0, 2346.0, 2400.0] if envi else [455.0, 2311.0, 2352.0, 630.0]
    cube = (rng.random((H, W, len(centres))) * 20).astype(np.float32)
    cube[rng.random(cube.shape) < .05] = -9999
    name = os.path.basename(folder.rstrip("/"))
    if envi:
        cube.tofile(os.path.join(folder, f"{name}_img"))
        with open(os.path.join(folder, f"{name}_img.hdr"), "w") as fh:
            fh.write(f"ENVI\nsamples = {W}\nlines = {H}\nbands = {len(centres)}\nheader offset = 0\ndata type = 4\ninterleave = bip\n"
                     f"byte order = 0\ndata ignore value = -9999\nmap info = {{UTM, 1, 1, 600000, 3500000, 5, 5, 13, North, WGS-84}}\n"
                     f"wavelength = {{{', '.join(str(c) for c in centres)}}}\n")
        picks = {"2350nm": 4, "2310nm": 3}
    else:
        with open(os.path.join(folder, "metadata.json"), "w") as fh:
            json.dump({"wavelengths": centres}, fh)
        picks = {"2350nm": 2, "2310nm": 1}
        for b in picks.values():
            io.write_tiff(os.path.join(folder, f"{b}.tif"), cube[:, :, b], blocksize=128, extra_tags={**GEO, 42113: (2, ("-9999",))})
    for key, b in picks.items():
        src[key] = cube[:, :, b][None]
    return src


@pytest.fixture(scope="module")
def cached(tmp_path_factory):
    root = tmp_path_factory.mktemp("wcut")
    fa, fb = str(root / "ang20191018t141549") + "/", str(root / "ang20191021t160052") + "/"
    srcs = {fa: make_flightline(fa, (96, 40), 1, envi=True), fb: make_flightline(fb, (80, 52), 2, envi=False)}
    wins = [(10, 4, 32, 32), (80, 20, 32, 32), (2, 30, 15, 15), (0, 0, 32, 32), (60, 30, 32, 32)]
    table = pd.DataFrame({"folder": [fa, fa, fa, fb, fb], "window": wins,
                          "window_row_off": [w[0] for w in wins], "window_col_off": [w[1] for w in wins],
                          "window_height": [w[2] for w in wins], "window_width": [w[3] for w in wins],
                          "has_plume": [True, False, False, True, False]}, index=[f"s{k}" for k in range(5)])
    table.index.name = "id"
    ds = sampling.WindowDataset(table, ["mag1c", "label_rgba", "S2A_B12", "S2B_B1", "WV3_SWIR1"], wavelengths=[2350., 2310.],
                                output_size=(32, 32), toa_correction_factor={fa: FACTORS[0], fb: FACTORS[1]},
                                memory_budget=64 * 2000)                       # flight line A is cut in two chunks
    out = str(root / "out")
    ds.cache(out, "train")
    return {"ds": ds, "out": out, "srcs": srcs, "table": table, "factor": {fa: FACTORS[0], fb: FACTORS[1]}}


def expected_item(src, window, factor):
    irr = {"S2A_B12": aviris.SOLAR_IRRADIANCE_S2A["B12"], "S2B_B1": aviris.SOLAR_IRRADIANCE_S2B["B01"],
           "WV3_SWIR1": aviris.SOLAR_IRRADIANCE_WV3["SWIR1"]}
    want = {}
    for key, a in src.items():
        fill = -9999.0 if a.dtype == np.float32 else None
        if key in irr:
            scale, clip = factor / 100 / irr[key], (0, 2)
        elif key.endswith("nm"):
            scale, clip = factor, None
        else:
            scale, clip = None, ((0, 10_000) if key == "mag1c" else None)
        want[key] = np.stack([U.cut(p, window, (0, 0), fill, scale, clip) for p in a])
    return want


def test_cache_writes_the_restatement(cached):
    ds, out = cached["ds"], cached["out"]
    assert ds.windows[2] == (-6, 22, 32, 32)                               # the 15 x 15 window, padded across two edges
    assert len(wd.plan_chunks(ds.folders, ds.windows, {f: s["shape"][0] for f, s in ds._sources.items()},
                              {f: s["row_bytes"] for f, s in ds._sources.items()}, ds.memory_budget)) == 3
    names = {"mag1c": "mag1c", "label_rgba": "label_rgba", "S2A_B12": "TOA_S2A_B12", "S2B_B1": "TOA_S2B_B1", "WV3_SWIR1": "TOA_WV3_SWIR1",
             "2350nm": "TOA_AVIRIS_2350nm", "2310nm": "TOA_AVIRIS_2310nm"}
    for k, idx in enumerate(ds.dataframe.index):
        folder, window = ds.folders[k], ds.windows[k]
        want = expected_item(cached["srcs"][folder], window, cached["factor"][folder])
        sample = os.path.join(out, idx)
        assert sorted(os.listdir(sample)) == sorted(f"{n}.tif" for n in list(names.values()) + ["labelbinary"])
        cut = {}
        for key, stem in names.items():
            path = os.path.join(sample, f"{stem}.tif")
            info = io.tiff_info(path)
            got = io.read_tiff(path, info=info)
            assert U.equal(got, want[key]), (idx, key)
            cut[key] = got
            assert info.block == (128, 128) and info.tiled
            assert info.tags[42113][1][0].strip("\0") == "0"
            desc = info.tags[42112][1][0]
            for d in (["r", "g", "b", "a"] if key == "label_rgba" else [stem]):
                assert f'role="description">{d}</Item>' in desc
            assert info.tags[33550][1] == (5.0, 5.0, 0.0)
            assert info.tags[33922][1] == (0.0, 0.0, 0.0, 600000.0 + 5.0 * window[1], 3500000.0 - 5.0 * window[0], 0.0)
            assert info.tags[34735][1][-1] == 32613
        info = io.tiff_info(os.path.join(sample, "labelbinary.tif"))
        assert 42113 not in info.tags and 'role="description">labelbinary</Item>' in info.tags[42112][1][0]
        assert info.tags[33922][1][3:5] == (600000.0 + 5.0 * window[1], 3500000.0 - 5.0 * window[0])
        lb = io.read_tiff(os.path.join(sample, "labelbinary.tif"), info=info)
        assert lb.dtype == np.uint8 and lb.shape == (1, 32, 32)
        assert np.array_equal(lb[0], mask_creation.proposed_mask(cut["label_rgba"], cut["mag1c"]).astype(np.uint8))
        item = ds[k]                                                       # __getitem__ gives the same arrays under the reference's keys
        assert sorted(item) == sorted(list(names) + ["labelbinary"])
        assert all(U.equal(item[key], cut[key]) for key in names) and np.array_equal(item["labelbinary"], lb)
    assert any(io.read_tiff(os.path.join(out, i, "labelbinary.tif")).any() for i in ds.dataframe.index)


def test_cache_tables(cached):
    out, table = cached["out"], cached["table"]
    cols = [c for c in table.columns if c != "window"]
    sampled = pd.read_csv(os.path.join(out, "train_sampled_data.csv"), index_col=0)
    assert list(sampled.columns) == cols and list(sampled.index) == list(table.index)
    assert list(sampled["folder"]) == list(table["folder"])
    assert list(sampled["window_row_off"]) == [10, 80, 2, 0, 60] and list(sampled["window_width"]) == [32, 32, 15, 32, 32]
    new = pd.read_csv(os.path.join(out, "train.csv"), index_col=0)
    assert list(new.columns) == cols and "window" not in new.columns
    assert list(new["folder"]) == [os.path.join(out, i) for i in table.index]
    assert (new["window_row_off"] == 0).all() and (new["window_col_off"] == 0).all()
    assert (new["window_width"] == 32).all() and (new["window_height"] == 32).all()


def test_second_cache_writes_nothing_and_missing_sources_raise(cached, tmp_path):
    ds, out = cached["ds"], cached["out"]
    files = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs]
    before = {f: os.stat(f).st_mtime_ns for f in files}
    ds.cache(out, "train", overwrite=False)
    assert {f: os.stat(f).st_mtime_ns for f in files} == before
    missing = sampling.WindowDataset(cached["table"], ["mag1c", "label_rgba", "S2A_B11"], output_size=(32, 32),
                                     toa_correction_factor=cached["factor"])
    with pytest.raises(FileNotFoundError):
        missing.cache(str(tmp_path / "never"), "train")
    assert not os.path.exists(tmp_path / "never")


def test_steps_four_five_six_chain(cached):
    out = cached["out"]
    new = pd.read_csv(os.path.join(out, "train.csv"), index_col=0)
    kept = {i: io.read_tiff(os.path.join(out, i, "labelbinary.tif")) for i in new.index}
    mask_creation.write_label_masks(new, overwrite=True)
    for i in new.index:
        assert np.array_equal(io.read_tiff(os.path.join(out, i, "labelbinary.tif")), kept[i])
    feats = ["weight_mag1c", "ratio_aviris_2350_2310_out"]
    features.extract_features(feats, new)
    for i in new.index:
        for f in feats:
            a = io.read_tiff(os.path.join(out, i, f"{f}.tif"))
            assert a.shape == (1, 32, 32) and a.dtype == np.float32
