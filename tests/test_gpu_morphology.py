"""starcop_amd.morphology on the device against the oracles of morphology_util.py: every comparison is exact.  sc_edt (both row
passes, every output, strided inputs, batches), the disc operators against scipy.ndimage, the sieve against scipy's labelling,
tolerant plume matching, products.clean and the clean= argument of the three scene calls of starcop_amd.pipeline."""
import functools
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import morphology_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = dict(U.case_table())
NAMES = list(CASES)
RADII = (0, 1, 1.5, 2, 3.2, 5, 17.5)


@functools.lru_cache(maxsize=None)
def oracle(name, to):
    """the reference of a case, computed once and never modified"""
    m = CASES[name]
    d2 = U.d2_oracle(m != 0 if to == "set" else m == 0)
    d2.setflags(write=False)
    return d2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_distance_transform(hip, name):
    from starcop_amd import morphology as mo
    m = dev(CASES[name])
    for to in ("set", "unset"):
        d2 = oracle(name, to)
        got = mo.distance_transform(m, to=to, squared=True)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), d2.astype(np.int32))
        assert torch.equal(got, mo.distance_transform(m, to=to, squared=True))                  # two calls, identical bytes
        for ps in (1.0, 5.0):
            d = mo.distance_transform(m, to=to, pixel_size=ps)
            assert same_bits(d.cpu().numpy(), U.dist_f32(d2, ps))
            assert torch.equal(d.view(torch.int32), mo.distance_transform(m, to=to, pixel_size=ps).view(torch.int32))


@pytest.mark.parametrize("name", NAMES)
def test_row_pass_variants_agree(hip, name):
    from starcop_amd import morphology as mo
    R = mo.WINDOW_MAX_R
    m = dev(CASES[name])
    H, W = CASES[name].shape
    for to in ("set", "unset"):
        d2 = oracle(name, to)
        for md in (1, 1.5, 5, 17, R, R + 1):
            cap = int(np.floor(md * md))
            want = U.capped(d2, cap).astype(np.int32)
            rule = mo.edt_variant(H, W, cap)
            assert rule == ("window" if md <= R else "envelope")
            res = {v: mo.distance_transform(m, to=to, max_distance=md, squared=True, variant=v).cpu().numpy()
                   for v in ((None, "envelope", "window") if md <= R else (None, "envelope"))}
            for v, got in res.items():
                assert np.array_equal(got, want), (to, md, v)
            d = mo.distance_transform(m, to=to, max_distance=md, pixel_size=5.0).cpu().numpy()
            assert same_bits(d, U.dist_f32(U.capped(d2, cap), 5.0))
    with pytest.raises(ValueError):
        mo.distance_transform(m, max_distance=R + 1, variant="window")
    zero = mo.distance_transform(m, max_distance=0, squared=True).cpu().numpy()              # only the targets lie within 0
    assert np.array_equal(zero, U.capped(oracle(name, "set"), 0).astype(np.int32))


def test_batch_numpy_and_dtypes(hip):
    from starcop_amd import morphology as mo
    H, W = 37, 53
    batch = np.stack([np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8), U.bernoulli((H, W), 0.05, 11)])
    for to in ("set", "unset"):
        want = np.stack([U.d2_brute(b != 0 if to == "set" else b == 0) for b in batch]).astype(np.int32)
        got = mo.distance_transform(dev(batch), to=to, squared=True)
        assert got.shape == (3, H, W) and np.array_equal(got.cpu().numpy(), want)
        host = mo.distance_transform(batch, to=to, squared=True)                               # numpy in, numpy out
        assert isinstance(host, np.ndarray) and host.dtype == np.int32 and np.array_equal(host, want)
        d = mo.distance_transform(batch[2], to=to)
        assert isinstance(d, np.ndarray) and same_bits(d, U.dist_f32(want[2].astype(np.int64)))
    assert np.isinf(mo.distance_transform(batch[0])).all() and (mo.distance_transform(batch[0], squared=True) == U.FAR).all()
    m = batch[2]
    want = U.d2_brute(m != 0).astype(np.int32)
    for other in (m.astype(bool), m.astype(np.float32) * -2.5, m.astype(np.int64) * 7):          # anything but uint8 is x != 0
        assert np.array_equal(mo.distance_transform(other, squared=True), want)
        assert np.array_equal(mo.distance_transform(dev(other), squared=True).cpu().numpy(), want)
    assert np.array_equal(mo.dilate(m * 200, 2), U.dilate(m, 2))                                  # uint8: any non-zero value is set


def test_strided_masks_are_read_in_place(hip):
    from starcop_amd import morphology as mo
    H, W = 64, 130
    rng = np.random.default_rng(5)
    inter = dev((rng.random((H, W, 4)) < 0.03).astype(np.uint8))
    wide = dev(U.bernoulli((H, 2 * W), 0.03, 6))
    stack = dev((rng.random((3, 2, H, W)) < 0.03).astype(np.uint8))
    for view in (inter[:, :, 2], wide[:, ::2], stack[:, 1], inter.permute(2, 0, 1)[1:3]):
        assert not view.is_contiguous()
        copy = view.contiguous()
        ref = np.stack([U.d2_brute(c != 0) for c in copy.cpu().numpy().reshape(-1, H, W)]).reshape(copy.shape).astype(np.int32)
        for kw in (dict(), dict(max_distance=5), dict(to="unset")):
            got = mo.distance_transform(view, squared=True, **kw)
            assert torch.equal(got, mo.distance_transform(copy, squared=True, **kw))
        assert np.array_equal(mo.distance_transform(view, squared=True).cpu().numpy(), ref)
        assert torch.equal(mo.dilate(view, 3.2), mo.dilate(copy, 3.2)) and torch.equal(mo.erode(view, 1), mo.erode(copy, 1))


@pytest.mark.parametrize("name", NAMES)
def test_dilate_erode(hip, name):
    from starcop_amd import morphology as mo
    m = CASES[name]
    d = dev(m)
    for r in RADII:
        got = mo.dilate(d, r)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), U.dilate(m, r)), ("dilate", r)
        assert np.array_equal(mo.erode(d, r).cpu().numpy(), U.erode(m, r)), ("erode", r)
    cross = ndimage.generate_binary_structure(2, 1)                          # the 3 x 3 cross proposed_mask dilates and erodes with
    assert np.array_equal(mo.dilate(d, 1).cpu().numpy(), ndimage.binary_dilation(m != 0, cross).astype(np.uint8))
    assert np.array_equal(mo.erode(d, 1).cpu().numpy(), ndimage.binary_erosion(m != 0, cross, border_value=1).astype(np.uint8))


@pytest.mark.parametrize("name", ["bern0.5_37x53", "bern0.05_64x130", "checker_37x53", "full_9x257", "empty_9x64", "bern0.5_9x65"])
def test_opening_closing(hip, name):
    from starcop_amd import morphology as mo
    m = CASES[name]
    blobs = ndimage.binary_dilation(m != 0, U.disc(2)).astype(np.uint8) if "bern0.05" in name else m
    for r in (1, 1.5, 3.2):
        for src in (m, blobs):
            d = dev(src)
            op, cl = mo.opening(d, r), mo.closing(d, r)
            assert torch.equal(op, mo.dilate(mo.erode(d, r), r)) and torch.equal(cl, mo.erode(mo.dilate(d, r), r))
            assert np.array_equal(op.cpu().numpy(), U.dilate(U.erode(src, r), r))
            assert np.array_equal(cl.cpu().numpy(), U.erode(U.dilate(src, r), r))
            assert torch.equal(mo.opening(op, r), op)
            assert np.array_equal(mo.opening(src, r), op.cpu().numpy())                        # numpy in, numpy out


def test_remove_small_objects(hip):
    from starcop_amd import morphology as mo
    masks = [U.bernoulli((37, 53), 0.3, 21), U.bernoulli((64, 130), 0.45, 22), CASES["checker_37x53"], CASES["empty_37x53"],
             CASES["full_9x257"], U.bernoulli((300, 1100), 0.35, 23)]
    for m in masks:
        for conn in (1, 2):
            for a in (1, 2, 5, 50):
                got = mo.remove_small_objects(dev(m), a, connectivity=conn)
                assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), U.sieve(m, a, conn)), (m.shape, conn, a)
    batch = np.stack([U.bernoulli((37, 53), d, 30 + k) for k, d in enumerate((0.0, 0.3, 0.5, 1.0))])
    for conn in (1, 2):
        got = mo.remove_small_objects(batch, 5, connectivity=conn)
        assert isinstance(got, np.ndarray) and np.array_equal(got, np.stack([U.sieve(b, 5, conn) for b in batch]))
        for k, b in enumerate(batch):
            assert np.array_equal(mo.remove_small_objects(b, 5, connectivity=conn), got[k])


def _match_counts(r):
    return r["tp"], r["fp"], r["fn"]


def test_match_plumes_tolerance(hip):
    from starcop_amd import plumes
    pred, lab = np.zeros((20, 30), np.uint8), np.zeros((20, 30), np.uint8)
    pred[5:11, 2:8] = 1
    lab[5:11, 10:16] = 1                                 # the nearest pixels of the two 6 x 6 blobs are 3 pixels apart
    assert U.d2_brute(lab != 0)[pred != 0].min() == 9
    assert _match_counts(plumes.match_plumes(pred, lab)) == (0, 1, 1)
    assert _match_counts(plumes.match_plumes(pred, lab, tolerance_px=2.9)) == (0, 1, 1)
    r = plumes.match_plumes(pred, lab, tolerance_px=3)
    assert _match_counts(r) == (1, 0, 0) and r["pred"]["overlap_px"].tolist() == [6] and r["precision"] == r["recall"] == 1.0
    assert _match_counts(plumes.match_plumes(dev(pred), dev(lab), tolerance_px=3.0)) == (1, 0, 0)
    # a Bernoulli pair: the tolerant match is the plain reduction of each side against the numpy-dilated other side
    p, q = U.bernoulli((64, 130), 0.02, 41), U.bernoulli((64, 130), 0.02, 42)
    p, q = U.dilate(p, 1.5), U.dilate(q, 1)
    for t in (1, 2.5, 6):
        for mo_px in (1, 3):
            r = plumes.match_plumes(p, q, min_overlap_px=mo_px, tolerance_px=t)
            a = plumes.plume_table(p, label_mask=U.dilate(q, t))
            b = plumes.plume_table(q, label_mask=U.dilate(p, t))
            assert r["pred"].equals(a) and r["label"].equals(b)
            tp = int((a["overlap_px"] >= mo_px).sum())
            assert _match_counts(r) == (tp, len(a) - tp, int((b["overlap_px"] < mo_px).sum()))
    plain, zero = plumes.match_plumes(p, q), plumes.match_plumes(p, q, tolerance_px=0)
    assert plain["pred"].equals(zero["pred"]) and plain["label"].equals(zero["label"]) and _match_counts(plain) == _match_counts(zero)
    assert plain["pred"].equals(plumes.plume_table(p, label_mask=q))
    # polygons: the same rule with the burnt image as the label side
    ring = [np.array([[10.0, 5.0], [16.0, 5.0], [16.0, 11.0], [10.0, 11.0]])]
    assert _match_counts(plumes.match_plumes_polygons(dev(pred), [ring])) == (0, 1, 1)
    assert _match_counts(plumes.match_plumes_polygons(dev(pred), [ring], tolerance_px=2.9)) == (0, 1, 1)
    assert _match_counts(plumes.match_plumes_polygons(dev(pred), [ring], tolerance_px=3)) == (1, 0, 0)


def _clean_ref(m, open_radius=0.0, min_area=1, exclude=None, exclude_buffer_px=0.0, connectivity=2):
    m0 = (m != 0).astype(np.uint8)
    m1 = U.dilate(U.erode(m0, open_radius), open_radius)
    m2 = U.sieve(m1, min_area, connectivity)
    m3 = m2 & (1 - U.dilate(exclude, exclude_buffer_px)) if exclude is not None else m2
    n = [int(x.sum()) for x in (m0, m1, m2, m3)]
    return m3, {"opened_px": n[0] - n[1], "sieved_px": n[1] - n[2], "excluded_px": n[2] - n[3]}


def test_products_clean(hip, tmp_path):
    from starcop_amd import io_formats, products
    H, W = 70, 100
    m = np.maximum(U.dilate(U.bernoulli((H, W), 0.01, 51), 2), U.bernoulli((H, W), 0.03, 52))       # blobs and speckle
    excl = np.zeros((H, W), np.uint8)
    excl[20:40, 10:30] = 3
    prob = dev(np.random.default_rng(53).random((H, W)).astype(np.float32))
    steps = [dict(), dict(open_radius=1), dict(open_radius=1.5), dict(min_area=4), dict(min_area=4, connectivity=1),
             dict(exclude=excl), dict(exclude=excl, exclude_buffer_px=2), dict(open_radius=1, min_area=4, exclude=excl, exclude_buffer_px=2)]
    for kw in steps:
        want, counts = _clean_ref(m, **kw)
        for mask in (dev(m), dev(m).bool()):
            out = {"pred_binary": mask, "prediction": prob, "mf": prob}
            assert products.clean(out, **kw) is out
            assert out["pred_binary"].dtype == mask.dtype and np.array_equal(out["pred_binary"].cpu().numpy().astype(np.uint8), want), kw
            assert out["clean"] == counts and out["prediction"] is prob and out["mf"] is prob
    want, counts = _clean_ref(m, **steps[-1])
    assert counts["opened_px"] > 0 and counts["sieved_px"] >= 0 and counts["excluded_px"] > 0 and 0 < want.sum() < (m != 0).sum()
    path = str(tmp_path / "exclude.tif")
    io_formats.write_tiff(path, excl, blocksize=128)
    for e in (dev(excl), dev(excl.astype(np.float32)), path):
        out = {"pred_binary": dev(m)}
        products.clean(out, open_radius=1, min_area=4, exclude=e, exclude_buffer_px=2)
        assert np.array_equal(out["pred_binary"].cpu().numpy(), want) and out["clean"] == counts
    with pytest.raises(ValueError, match="reproject_like"):
        products.clean({"pred_binary": dev(m)}, exclude=excl[:, :-1])


def test_aviris_scene_predict_clean(hip, tmp_path):
    """the 70 x 100 flight line of the scene tests: with clean= the mask file, the table and the outlines describe the cleaned
    mask and pred.tif keeps its bytes; with clean=None every file is what a call without the argument writes"""
    import json
    import pandas as pd
    import plume_scene_util as S
    from starcop_amd import io_formats, pipeline, plumes, products
    from test_gpu_plume_scene import _model
    H, W = 70, 100
    model = _model(bias=-0.93)
    wl = np.array([440.0, 461.0, 500.0, 549.0, 600.0, 641.0, 700.0])
    valid = S.strip_mask(H, W, centre=30.0, slope=0.3, half_width=25.0)
    rng = np.random.default_rng(61)
    cube = rng.uniform(0.5, 12.0, size=(H, W, wl.size)).astype(np.float32)
    cube[~valid] = S.FILL
    mf = (600.0 * rng.standard_normal((H, W)) + 200.0).astype(np.float32)
    mf[~valid] = S.FILL
    folder = S.write_flight_line(str(tmp_path / "ang20190101t180000_rdn"), cube, wl)
    io_formats.write_tiff(os.path.join(folder, "mag1c.tif"), mf, blocksize=128, extra_tags={42113: (2, ("-9999",))})
    kw = dict(toa_correction_factor=1.037, tile=32, halo=32, plumes=True, plume_outlines=True)
    names = ["plumes.csv", "plumes.geojson", "pred.tif", "predbinary.tif"]

    def data(sub, name):
        return open(str(tmp_path / sub / name), "rb").read()
    base = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "a"), **kw)
    mask = base["pred_binary"].cpu().numpy().astype(np.uint8)
    area = np.bincount(ndimage.label(mask, np.ones((3, 3)))[0].ravel())[1:]
    assert area.min() == 1 and area.max() >= 8, area                 # single pixels and larger components
    excl = np.zeros((H, W), np.uint8)
    r, c = np.argwhere(mask)[len(np.argwhere(mask)) // 2]
    excl[r, c] = 1
    args = dict(open_radius=1, min_area=4, exclude=excl, exclude_buffer_px=2)
    want = {"pred_binary": base["pred_binary"].clone()}
    products.clean(want, **args)
    ref, counts = _clean_ref(mask, **args)
    cleaned = want["pred_binary"].cpu().numpy().astype(np.uint8)
    assert np.array_equal(cleaned, ref) and want["clean"] == counts
    assert 0 < cleaned.sum() < mask.sum()                             # removes something, keeps something
    out = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "b"), clean=args, **kw)
    assert sorted(os.path.basename(p) for p in out["files"]) == names and out["clean"] == counts
    assert np.array_equal(np.squeeze(io_formats.read_tiff(str(tmp_path / "b" / "predbinary.tif"))), cleaned)
    assert np.array_equal(out["pred_binary"].cpu().numpy().astype(np.uint8), cleaned)
    table = plumes.plume_table(cleaned)
    csv = pd.read_csv(str(tmp_path / "b" / "plumes.csv"))
    cols = ["item", "plume_id", "area_px", "row_min", "row_max", "col_min", "col_max"]
    assert len(csv) == len(table) == len(out["plumes"]) >= 1 and csv[cols].astype(np.int64).equals(table[cols].astype(np.int64))
    assert int(csv["area_px"].sum()) == int(cleaned.sum())           # (the exclusion comes after the sieve and may cut a plume)
    assert len(json.load(open(str(tmp_path / "b" / "plumes.geojson")))["features"]) == len(csv)
    assert data("b", "pred.tif") == data("a", "pred.tif") and data("b", "predbinary.tif") != data("a", "predbinary.tif")
    none = pipeline.aviris_scene_predict(model, folder, str(tmp_path / "c"), clean=None, match_tolerance_px=0.0, **kw)
    assert "clean" not in none and sorted(os.listdir(str(tmp_path / "c"))) == names
    for n in names:
        assert data("c", n) == data("a", n), n
    with pytest.raises(ValueError):
        pipeline.aviris_scene_predict(model, folder, clean=dict(radius=1), **kw)
    # the tolerance of the label match reaches burn_and_match: the outlines of the un-cleaned plumes as labels, shifted by 2 pixels
    shifted = {k: [ring + np.array([2 * 5.0, 0.0]) for ring in v] for k, v in base["plume_outlines"].items()}
    strict = pipeline.aviris_scene_predict(model, folder, label_polygons=shifted, **kw)["plume_match"]
    loose = pipeline.aviris_scene_predict(model, folder, label_polygons=shifted, match_tolerance_px=2.0, **kw)["plume_match"]
    assert loose["tp"] == len(loose["pred"]) and loose["fn"] == 0 and loose["tp"] >= strict["tp"] and loose["fp"] <= strict["fp"]
    assert (loose["pred"]["overlap_px"] >= strict["pred"]["overlap_px"]).all()


def test_mosaic_products_and_emit_granule_predict_clean(hip, tmp_path):
    """the other two scene calls: clean= is products.clean of the mask the call would otherwise write, pred.tif keeps its bytes"""
    import mosaic_util as MU
    from starcop_amd import io_formats as io, model_module as mm, pipeline, products, warp
    from test_gpu_mosaic import scene_dicts

    def data(folder, name):
        return open(os.path.join(folder, name), "rb").read()

    def mask_file(folder):
        return np.squeeze(io.read_tiff(os.path.join(folder, "predbinary.tif")))
    outs = scene_dicts()
    folders = []
    for i, o in enumerate(outs):
        folders.append(str(tmp_path / f"scene{i}"))
        products.write_rasters(o, (products.MAG1C, products.PRED, products.PREDBINARY), folders[-1], True,
                               warp.geo_tags(o["geotransform"], o["crs"]), MU.NODATA, {})
    a, b = str(tmp_path / "mosaic_a"), str(tmp_path / "mosaic_b")
    plain = pipeline.mosaic_products(folders, a, crs=32613, resolution=60.0, plumes=True)
    H, W = plain["pred_binary"].shape
    excl = np.zeros((H, W), np.uint8)
    excl[:, :W // 2] = 1
    for args in (dict(min_area=3), dict(open_radius=1, exclude=excl, exclude_buffer_px=1.5)):
        want = products.clean({"pred_binary": plain["pred_binary"].clone()}, **args)
        ref, counts = _clean_ref(plain["pred_binary"].cpu().numpy(), **args)
        res = pipeline.mosaic_products(folders, b, crs=32613, resolution=60.0, plumes=True, clean=args, overwrite=True)
        assert res["clean"] == want["clean"] == counts and np.array_equal(mask_file(b), ref)
        assert torch.equal(res["pred_binary"], want["pred_binary"]) and int(res["plumes"]["area_px"].sum()) == int(ref.sum())
        assert data(b, "pred.tif") == data(a, "pred.tif") and data(b, "mag1c.tif") == data(a, "mag1c.tif")
    none = pipeline.mosaic_products(folders, str(tmp_path / "mosaic_c"), crs=32613, resolution=60.0, plumes=True, clean=None)
    for n in ("pred.tif", "predbinary.tif", "mag1c.tif", "source.tif", "plumes.csv"):
        assert data(str(tmp_path / "mosaic_c"), n) == data(a, n), n
    # the EMIT fixture granule, orthorectified
    nc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "io", "emit_l1b_like_sb0.nc")
    gt = (-110.25, 0.000542232520256367, 0.0, 35.5, 0.0, -0.000542232520256367)
    torch.manual_seed(0)
    model = mm.ModelModule(mm.default_settings(pos_weight=1)).to(DEV).eval()
    kw = dict(column_step=4, georeferenced=True, geotransform=gt, plumes=True)
    plain = pipeline.emit_granule_predict(model, nc, out_folder=str(tmp_path / "emit_a"), **kw)
    args = dict(open_radius=1, min_area=3)
    want = products.clean({"pred_binary": plain["pred_binary"].clone()}, **args)
    ref, counts = _clean_ref(plain["pred_binary"].cpu().numpy(), **args)
    res = pipeline.emit_granule_predict(model, nc, out_folder=str(tmp_path / "emit_b"), clean=args, **kw)
    assert res["clean"] == want["clean"] == counts and np.array_equal(mask_file(str(tmp_path / "emit_b")), ref)
    assert int(res["plumes"]["area_px"].sum()) == int(ref.sum())
    assert data(str(tmp_path / "emit_b"), "pred.tif") == data(str(tmp_path / "emit_a"), "pred.tif")
    assert torch.equal(res["pred_binary_raw"], plain["pred_binary_raw"])                      # the sensor-geometry mask is left alone
    with pytest.raises(ValueError):
        pipeline.emit_granule_predict(model, nc, column_step=4, clean=args)
