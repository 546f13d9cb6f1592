"""The feature registry (starcop/data/feature_extration.py:193-246) and the host side of the MLR ratio: no GPU needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_registry_keys_and_inputs_match_the_reference():
    from starcop_amd import features
    g = np.load(os.path.join(G, "g12_mlr.npz"))
    assert list(features.FEATURES) == [str(k) for k in g["registry_keys"]]
    for k, inputs in zip(g["registry_keys"], g["registry_inputs"]):
        e = features.FEATURES[str(k)]
        assert e["inputs"] == str(inputs).split(","), k
        assert e["fill_value_default"] is None and callable(e["function"])
    assert features.FEATURES["ratio_wv3_B8_B8MLR_SanchezGarcia22_sum_c_out"]["function"] is features.ratio_MLR_local_5IN
    assert features.FEATURES["ratio_wv3_B7_B7MLR_fromS2_9bands_sum_c_out"]["function"] is features.ratio_MLR_local_9IN
    assert features.FEATURES["ratio_wv3_B7_B7MLR_SanchezGarcia22_simplediv"]["function"] is features.ratio_MLR_local_5IN_simplediv


def test_unreachable_and_unknown_divisions_raise():
    from starcop_amd import features
    for div in ("simple", "nope"):
        with pytest.raises(ValueError):
            features.ratio_MLR_local([np.zeros((4, 4), np.float32)], np.zeros((4, 4), np.float32), division=div)
    with pytest.raises(NotImplementedError):
        features.FEATURES["ratio_lrn_bands2band8only_60ep_512_l1"]["function"]()
    with pytest.raises(KeyError):
        features.extract_features(["not_a_product"], {"folder": []})


def test_mlr_struct_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof of sc_mlr_args as gcc lays it out == the ctypes mirror in _lib.py"""
    from starcop_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = ["base", "band_off", "k", "tile_stride", "target", "target_tile_stride", "B", "n"]
    src = tmp_path / "mlr.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "starcop_hip.h"\nint main(void){printf("%zu", sizeof(sc_mlr_args));'
                   + "".join(f'printf(" %zu", offsetof(sc_mlr_args, {f}));' for f in fields)
                   + 'printf(" %d %d %d\\n", SC_MLR_C_MATCHED, SC_MLR_SIMPLE_PLUS, SC_MLR_RESIDUAL);return 0;}\n')
    exe = tmp_path / "mlr"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_lib.sc_mlr_args)] + [getattr(_lib.sc_mlr_args, f).offset for f in fields] + \
           [_lib.MLR_C_MATCHED, _lib.MLR_SIMPLE_PLUS, _lib.MLR_RESIDUAL]
    assert got == want
