"""Host side of the mag1c window statistics and the no-plume window sampling (starcop_amd.sampling): exports and argument checks
of sc_window_stats, the window intersection rule, and select_non_overlapping / sampling_no_plumes / mag1c_stats_dataframe against
what the reference's own functions returned (tests/golden/sampling_*.json, written by tests/golden/make_golden_sampling.py).
No GPU."""
import ctypes
import json
import os
import shutil
import subprocess
from collections import namedtuple

import numpy as np
import pandas as pd
import pytest

import winstats_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    from starcop_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "sampling_input.json")) as f:
        inp = json.load(f)
    with open(os.path.join(GOLDEN, "sampling_expected.json")) as f:
        exp = json.load(f)
    stats = pd.DataFrame(inp["stats"])
    plumes = pd.DataFrame({"folder": [p[0] for p in inp["plumes"]], "window": [tuple(p[1:]) for p in inp["plumes"]]})
    return stats, plumes, exp


@pytest.fixture(scope="module")
def frame(golden):
    from starcop_amd import sampling
    stats, plumes, _ = golden
    return sampling.mag1c_stats_dataframe(stats, plumes)


def test_window_stats_symbols_are_exported(lib):
    from starcop_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sc_window_stats", "sc_window_stats_workspace_bytes"):
        assert hasattr(raw, name), f"{name} is not exported by libstarcop_hip.so"
        assert name in _lib.SIGNATURES
    assert lib.sc_window_stats_workspace_bytes(0) == 0
    one, many = lib.sc_window_stats_workspace_bytes(1), lib.sc_window_stats_workspace_bytes(200)
    assert 0 < one < many


def test_winstats_args_layout_matches_the_c_compiler(tmp_path):
    from starcop_amd import _lib
    assert shutil.which("gcc") is not None, "gcc is needed to lay out sc_winstats_args as the C compiler does"
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(sc_winstats_args), offsetof(sc_winstats_args, has_fill), '
                   'offsetof(sc_winstats_args, clip_max), offsetof(sc_winstats_args, windows), '
                   'offsetof(sc_winstats_args, windows_host), offsetof(sc_winstats_args, stats));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = _lib.sc_winstats_args
    assert got == [ctypes.sizeof(A), A.has_fill.offset, A.clip_max.offset, A.windows.offset, A.windows_host.offset, A.stats.offset]


def _args(wins, H=64, W=48):
    """arguments whose device pointers are never dereferenced: every case below is rejected on the host"""
    from starcop_amd import _lib
    wins = np.ascontiguousarray(wins, dtype=np.int32).reshape(-1, 4)
    a = _lib.sc_winstats_args()
    a.x, a.row_stride, a.H, a.W = 4096, W, H, W
    a.has_fill, a.fill, a.clip_max, a.n_win = 1, -9999.0, 10_000.0, wins.shape[0]
    a.windows, a.windows_host = 4096, wins.ctypes.data
    a.count = a.sum_mean = a.stats = 4096
    return a, wins


@pytest.mark.parametrize("case", ["n_win_zero", "n_win_negative", "row_outside", "col_outside", "negative_offset", "empty_window",
                                  "second_window_outside", "short_workspace", "null_workspace", "narrow_stride", "nan_clip"])
def test_argument_errors_return_a_negative_code(lib, case):
    wins = [[0, 0, 32, 32]]
    if case == "row_outside":
        wins = [[40, 0, 32, 32]]
    elif case == "col_outside":
        wins = [[0, 17, 32, 32]]
    elif case == "negative_offset":
        wins = [[-1, 0, 32, 32]]
    elif case == "empty_window":
        wins = [[0, 0, 0, 32]]
    elif case == "second_window_outside":
        wins = [[0, 0, 32, 32], [63, 47, 1, 1], [63, 47, 2, 1]]
    a, keep = _args(wins)
    wb = lib.sc_window_stats_workspace_bytes(max(a.n_win, 1))
    work = ctypes.c_void_p(4096)
    if case == "n_win_zero":
        a.n_win = 0
    elif case == "n_win_negative":
        a.n_win = -3
    elif case == "short_workspace":
        wb -= 1
    elif case == "null_workspace":
        work = None
    elif case == "narrow_stride":
        a.row_stride = a.W - 1
    elif case == "nan_clip":
        a.clip_max = float("nan")
    rc = lib.sc_window_stats(ctypes.byref(a), work, wb, None)
    assert rc < 0
    msg = lib.sc_last_error().decode()
    assert msg.startswith("sc_window_stats"), msg
    del keep


Win = namedtuple("Win", ["col_off", "row_off", "width", "height"])


def test_windows_intersect():
    from starcop_amd.sampling import windows_intersect
    a = (0, 0, 512, 512)
    assert windows_intersect(a, a)
    assert windows_intersect(a, (256, 256, 512, 512)) and windows_intersect((256, 256, 512, 512), a)
    assert windows_intersect(a, (511, 511, 512, 512))                       # one shared pixel
    assert not windows_intersect(a, (512, 0, 512, 512))                     # share the edge row 512
    assert not windows_intersect(a, (0, 512, 512, 512))                     # share the edge column 512
    assert not windows_intersect(a, (512, 512, 512, 512))                   # share a corner
    assert not windows_intersect(a, (0, 600, 512, 512)) and not windows_intersect(a, (900, 0, 10, 10))
    assert windows_intersect(a, (100, 100, 151, 151)) and windows_intersect((100, 100, 151, 151), a)      # containment
    assert windows_intersect((10, 0, 5, 1000), (0, 10, 1000, 5))            # a cross: no corner of one inside the other
    # objects with the four attributes (rasterio.windows.Window's field names) mix with tuples
    assert windows_intersect(Win(col_off=0, row_off=0, width=512, height=512), (511, 0, 1, 1))
    assert not windows_intersect(Win(col_off=0, row_off=0, width=512, height=512), Win(col_off=512, row_off=0, width=4, height=4))


def test_mag1c_stats_dataframe_matches_the_reference(golden, frame):
    stats, plumes, exp = golden
    want = exp["frame"]
    assert list(frame.index) == want["id"] and frame.index.name == "id"
    assert frame.shape[0] == stats.shape[0]                                 # listed ids that are absent create no rows
    for col in ("name", "folder", "subset"):
        assert list(frame[col]) == want[col], col
    assert [bool(v) for v in frame["has_plume"]] == want["has_plume"]
    assert any(want["has_plume"]) and not all(want["has_plume"]) and {"train", "test"} == set(want["subset"])
    assert [d.strftime("%Y-%m-%d") for d in frame["date"]] == want["date"]
    assert [d.isoformat() for d in frame["datetime"]] == want["datetime"]
    assert np.array_equal(frame["percentage_valids"].to_numpy(), np.array(want["percentage_valids"]))
    assert [list(w) for w in frame["window"]] == want["window"]


def test_unlabeled_ids_and_test_dates_are_parameters(golden):
    from starcop_amd import sampling
    stats, plumes, _ = golden
    none = sampling.mag1c_stats_dataframe(stats, plumes.iloc[:0], unlabeled_plume_ids=[], test_dates=[])
    assert not none["has_plume"].any() and set(none["subset"]) == {"train"}
    uid = none.index[7]
    one = sampling.mag1c_stats_dataframe(stats, plumes.iloc[:0], unlabeled_plume_ids=[uid, "ang20000101t000000_r0_c0_w512_h512"],
                                         test_dates=["2019-09-26"])
    hit = [i for i in one.index if one.loc[i, "has_plume"]]
    assert uid in hit and all(one.loc[i, "folder"] == one.loc[uid, "folder"] and
                              sampling.windows_intersect(one.loc[i, "window"], one.loc[uid, "window"]) for i in hit)
    assert len(hit) > 1 and one.shape[0] == stats.shape[0]
    assert set(one.loc[one["subset"] == "test", "name"]) == {"ang20190926t172904"}


def test_select_non_overlapping_matches_the_reference(golden, frame):
    from starcop_amd import sampling
    exp = golden[2]
    no_plumes = frame[~frame["has_plume"]]
    assert len(exp["select"]) >= 12
    for case in exp["select"]:
        line = no_plumes[no_plumes["name"] == case["name"]].sort_values(by="mean", ascending=False)
        got = sampling.select_non_overlapping(line, n=case["n"], idxs=case.get("idxs"))
        assert got == case["id"], case
        for i, a in enumerate(got):
            for b in got[i + 1:]:
                assert not sampling.windows_intersect(line.loc[a, "window"], line.loc[b, "window"])
    with pytest.raises(AssertionError):
        sampling.select_non_overlapping(no_plumes, n=0)
    with pytest.raises(AssertionError):
        sampling.select_non_overlapping(no_plumes, n=2, idxs=list(no_plumes.index[:2]))


def test_sampling_no_plumes_matches_the_reference(golden, frame):
    from starcop_amd import sampling
    exp = golden[2]
    no_plumes = frame[~frame["has_plume"]]
    assert len(exp["sampling"]) == 3 and any("random" in case["difficulty"] for case in exp["sampling"])
    for case in exp["sampling"]:
        sel = sampling.sampling_no_plumes(no_plumes, **case["args"])
        assert list(sel.index) == case["id"], case["args"]
        assert list(sel["difficulty"]) == case["difficulty"]
        assert "hard" in case["difficulty"]
        assert [int(v) for v in sel["qplume"]] == case["qplume"]
        assert list(sel["candidate_id"]) == case["candidate_id"] and list(sel["label_path"]) == case["label_path"]
        # the reference's frame holds rasterio windows and ours tuples; every other column is the same, in the same order
        assert list(sel.columns) == case["columns"]
        assert (sel["percentage_valids"] >= case["args"]["percentage_valids"]).all()


def test_oracle_follows_the_reference_loop():
    """the oracle on a scene small enough to check by hand: masking, clip, dropped empty window, column names"""
    s = np.array([[-9999., 1., 2., 20000.], [np.nan, -3., -0., np.inf], [-9999., -9999., -1., np.nan]], dtype=np.float32)
    rows = U.oracle_rows(s, [(0, 0, 2, 4), (2, 0, 1, 4), (0, 0, 3, 1)], fill=-9999.)
    assert len(rows) == 1                                           # the second and third windows hold nothing valid
    r = rows[0]
    assert r["count"] == 5 and r["max"] == 10000. and r["min"] == 0. and r["sum64"] == 20003. and r["median"] == 2.
    assert all(isinstance(r[c], np.float32) for c in U.F32_COLUMNS)
    assert set(U.COLUMNS) - {"sum", "mean"} <= set(r)
    assert U.oracle_rows(s, [(0, 0, 3, 1)], fill=None) == []        # -9999 and NaN fail v >= 0 whatever the fill


def test_pairwise_bound_holds_for_numpy():
    """numpy's float32 sum stays inside the bound derived in winstats_util.pairwise_depth, on sizes around its blocking"""
    rng = np.random.default_rng(5)
    for n in (1, 7, 8, 9, 127, 128, 129, 1000, 4099, 65536, 262144, 300001):
        x = (rng.random(n, dtype=np.float32) * np.float32(10000)).astype(np.float32)
        exact = float(np.sum(x.astype(np.float64)))
        _, b32 = U.sum_bounds(n)
        assert abs(float(np.sum(x)) - exact) <= b32 * exact * (1 + 1e-9) + n * 2.0 ** -53 * exact
