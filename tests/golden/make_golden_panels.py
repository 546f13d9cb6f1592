"""Generates tests/golden/g15_panels.npz with matplotlib: what ``Normalize`` + ``viridis(..., bytes=True)`` and
``ScalarMappable.to_rgba(..., bytes=True)`` give for seeded planes, the viridis table, and the names of the reference's
``PLOTTING_FUNCTIONS`` registry.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_panels.py [REFERENCE_CHECKOUT]

Needs matplotlib; the registry names are read from ``starcop/plot.py`` of the reference checkout when one is given (its keys,
``input_products`` and ``tensor`` fields: names only) and kept from the existing fixture otherwise.  Only DATA is written.
tests/test_plot_host.py calls ``expectations()`` again where matplotlib is importable and compares.
"""
import json
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(OUT, "g15_panels.npz")
H, W = 37, 53
RANGES = [(0.0, 2.0), (0.0, 1.0), (0.1, 0.7)]         # + the plane's own finite (min, max)


def planes():
    """the seeded inputs: a float32 plane with NaN, +-inf, values exactly at every vmin / vmax and just outside them, and an RGB
    stack that reaches below 0 and above 1"""
    rng = np.random.default_rng(15)
    x = rng.normal(0.45, 0.55, size=(H, W)).astype(np.float32)
    x[0, :3] = [np.nan, np.inf, -np.inf]
    x[5, 7] = np.nan
    x[36, 52] = np.inf
    edge = []
    for lo, hi in RANGES:
        for v in (lo, hi):
            f = np.float32(v)
            edge += [f, np.nextafter(f, np.float32(-9)), np.nextafter(f, np.float32(9))]
    x[1, :len(edge)] = edge
    x[2, :4] = [-3.0, 3.0, 0.5, 1.0 - 2.0 ** -24]
    rgb = rng.uniform(-0.25, 1.25, size=(3, H, W)).astype(np.float32)
    rgb[:, 3, :4] = np.array([0.0, 1.0, 0.5, 1.0 - 2.0 ** -24], np.float32)
    return x, rgb


def data_range(x):
    fin = x[np.isfinite(x)]
    return float(fin.min()), float(fin.max())


def expectations():
    """matplotlib's bytes: {"band_k": (H, W, 3) for range k, "rgb": (H, W, 3), "viridis8": (256, 3)}"""
    from matplotlib import cm, colormaps
    from matplotlib.colors import Normalize
    x, rgb = planes()
    out = {}
    for k, (lo, hi) in enumerate(RANGES + [data_range(x)]):
        with np.errstate(all="ignore"):
            out[f"band_{k}"] = colormaps["viridis"](Normalize(lo, hi)(x), bytes=True)[..., :3]
    # what imshow does with a float RGB image (after show_3_bands clamped it): to_rgba(bytes=True)
    img = np.clip(np.transpose(rgb, (1, 2, 0)), 0, 1)
    out["rgb"] = cm.ScalarMappable().to_rgba(img, bytes=True)[..., :3]
    out["viridis8"] = (np.asarray(colormaps["viridis"].colors) * 255).astype(np.uint8)
    return out


def registry(reference=None):
    if reference is None:
        return str(np.load(PATH)["registry"])
    sys.dont_write_bytecode = True
    sys.path.insert(0, reference)
    import matplotlib
    matplotlib.use("Agg")
    import starcop.plot as ref
    return json.dumps([[k, v.get("input_products"), v["tensor"]] for k, v in ref.PLOTTING_FUNCTIONS.items()])


def main():
    x, rgb = planes()
    exp = expectations()
    np.savez_compressed(PATH, plane=x, rgb_planes=rgb, ranges=np.array(RANGES + [data_range(x)], np.float64),
                        registry=np.array(registry(sys.argv[1] if len(sys.argv) > 1 else None)), **exp)
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
