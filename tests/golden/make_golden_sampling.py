"""Generates tests/golden/sampling_input.json and sampling_expected.json by RUNNING THE REFERENCE ITSELF
(starcop/data/sampling_dataset.py: permian_mag1c_stats_dataframe, select_non_overlapping, sampling_no_plumes).

Run in the build container only (needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sampling.py

georeader, rasterio, tqdm and the starcop modules that sampling_dataset.py imports but these three functions never call are
stubbed as empty modules.  The stub of ``rasterio.windows`` carries a ``Window`` with the four fields and ``intersect`` with the
rule starcop_amd.sampling.windows_intersect documents: two windows intersect iff their extents overlap with positive area.
The stats table (60 windows of 512 x 512 at stride 256 over three flight lines on two dates, one of them a test date) and the plume
table are seeded; permian_mag1c_stats_dataframe reads its CSV from a module-level path, which is pointed at a temporary file.
Five ids of the reference's hard-coded list of unlabelled plumes are windows of the table; the other ten are absent, for which
the reference's ``.loc`` assignment creates empty rows -- those rows (no folder) are not recorded.  Only DATA is written.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import pandas as pd

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)


class Window:
    def __init__(self, col_off, row_off, width, height):
        self.col_off, self.row_off, self.width, self.height = col_off, row_off, width, height


def intersect(a, b):
    return (min(a.row_off + a.height, b.row_off + b.height) > max(a.row_off, b.row_off) and
            min(a.col_off + a.width, b.col_off + b.width) > max(a.col_off, b.col_off))


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


_stub("georeader", window_utils=_stub("georeader.window_utils"))
_stub("georeader.rasterio_reader", RasterioReader=object)
_stub("georeader.geotensor", GeoTensor=object)
_stub("georeader.save_cog", save_cog=None)
_stub("rasterio", windows=_stub("rasterio.windows", Window=Window, intersect=intersect))
_stub("tqdm", tqdm=lambda x, **kw: x)
_stub("starcop.utils")
_stub("starcop.data.aviris")
_stub("starcop.data.mask_creation")

from starcop.data import sampling_dataset as ref  # noqa: E402

ROOT = "/data/permian/"
LINES = (("ang20191018t183859", 11), ("ang20190926t172904", 10), ("ang20190927t110000", 9))      # name, window rows


def stats_table():
    rng = np.random.default_rng(20191018)
    rows = []
    for k, (name, nrows) in enumerate(LINES):
        folder = ROOT + name + ("/" if k == 1 else "")        # both spellings of a folder occur in the table
        for r in range(nrows):
            for c in (0, 256):
                count = int(rng.integers(0.55 * 512 * 512, 512 * 512 + 1))
                mean = float(rng.integers(200, 9000)) / 8
                rows.append({"window_col_off": c, "window_row_off": 256 * r, "window_width": 512, "window_height": 512,
                             "folder": folder, "max": 10000.0, "min": 0.0, "mean": mean, "percentile01": mean / 8,
                             "percentile05": mean / 4, "median": mean / 2, "percentile95": mean * 2, "percentile99": mean * 3,
                             "sum": mean * count, "count": count})
    return pd.DataFrame(rows)


# labelled plumes: folder, row_off, col_off, height, width.  The second only shares the edge row 512 with the windows above it,
# the fourth lies in a folder the stats table does not hold.
PLUMES = [[ROOT + "ang20191018t183859/", 700, 100, 151, 151],
          [ROOT + "ang20190926t172904/", 2048, 256, 151, 151],
          [ROOT + "ang20190927t110000/", 1300, 600, 151, 151],
          [ROOT + "ang20190101t000000/", 0, 0, 151, 151]]
SAMPLING = [{"n_hard": 2, "n_random": 2, "percentage_valids": .8, "seed": 42},
            {"n_hard": 1, "n_random": 3, "percentage_valids": .7, "seed": 7},
            {"n_hard": 3, "n_random": 1, "percentage_valids": .9, "seed": 123}]


def main():
    table = stats_table()
    plumes = pd.DataFrame({"folder": [p[0] for p in PLUMES],
                           "window": [Window(col_off=p[2], row_off=p[1], width=p[4], height=p[3]) for p in PLUMES]})
    with tempfile.TemporaryDirectory() as tmp:
        ref.PERMIAN_MAG1C_STATS_DATAFRAME = os.path.join(tmp, "stats_mag1c.csv")
        table.to_csv(ref.PERMIAN_MAG1C_STATS_DATAFRAME, index=False)
        full = ref.permian_mag1c_stats_dataframe(plumes)
    full = full[full["folder"].notna()]
    assert full.shape[0] == table.shape[0]
    expected = {"frame": {"id": list(full.index), "name": list(full["name"]), "folder": list(full["folder"]),
                          "date": [d.strftime("%Y-%m-%d") for d in full["date"]],
                          "datetime": [d.isoformat() for d in full["datetime"]],
                          "percentage_valids": [float(v) for v in full["percentage_valids"]],
                          "has_plume": [bool(v) for v in full["has_plume"]], "subset": list(full["subset"]),
                          "window": [[int(w.row_off), int(w.col_off), int(w.height), int(w.width)] for w in full["window"]]}}
    no_plumes = full[~full["has_plume"].astype(bool)]
    expected["sampling"] = []
    for kw in SAMPLING:
        sel = ref.sampling_no_plumes(no_plumes, **kw)
        expected["sampling"].append({"args": kw, "id": list(sel.index), "difficulty": list(sel["difficulty"]),
                                     "qplume": [int(v) for v in sel["qplume"]], "candidate_id": list(sel["candidate_id"]),
                                     "label_path": list(sel["label_path"]), "columns": list(sel.columns)})
    expected["select"] = []
    for name, _ in LINES:
        line = no_plumes[no_plumes["name"] == name].sort_values(by="mean", ascending=False)
        for n in (1, 3, 50):
            expected["select"].append({"name": name, "n": n, "id": list(ref.select_non_overlapping(line, n=n))})
        first = [line.index[-1]]
        expected["select"].append({"name": name, "n": 4, "idxs": first, "id": list(ref.select_non_overlapping(line, n=4, idxs=first))})
    with open(os.path.join(OUT, "sampling_input.json"), "w") as f:
        json.dump({"stats": table.to_dict(orient="list"), "plumes": PLUMES}, f, indent=0)
    with open(os.path.join(OUT, "sampling_expected.json"), "w") as f:
        json.dump(expected, f, indent=0)
    n_sel = [len(s["id"]) for s in expected["sampling"]]
    print(f"{full.shape[0]} windows, {int(full['has_plume'].sum())} with plume, selected {n_sel}")


if __name__ == "__main__":
    main()
