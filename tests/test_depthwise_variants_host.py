"""The GPU case tables of tests/test_gpu_depthwise_variants.py reach EVERY kernel variant the depthwise dispatchers can select (no GPU).

The four depthwise launchers dispatch on the function behind the host-only query sc_dw_variant.  Here the query is swept over the
shapes each entry point accepts, and the set of codes it returns must EQUAL the set of codes of that op's case table: deleting a case,
or a dispatcher gaining a branch without a case, fails this test; so does a table entry whose shape no longer selects the code written
next to it, and a table that loses one of the edges it is there for."""
import pytest

from test_gpu_depthwise_variants import (DW_BWD_CASES, DW_CASES, DW_DGRAD_CASES, DW_FWD_CASES, DW_WGRAD_CASES, OP_BWD,
                                         OP_DGRAD, OP_FWD, OP_WGRAD, chain_tile, chain_wgrad, dw_code, dw_tile, dw_tiled_plane, dw_tiles,
                                         wgrad_tiles_per_group)

TILE_CODES = {1000 * s + 10 * tw for s in (1, 2) for tw in (64, 32, 16)}
STAGED_CODES = {c + v4 for c in TILE_CODES for v4 in (0, 1)} | {9016}
WANT = {OP_FWD: STAGED_CODES, OP_DGRAD: TILE_CODES, OP_WGRAD: TILE_CODES, OP_BWD: STAGED_CODES}


def _flags(case):
    return set(case[7].split())


def _aligned(case):
    return "offset" not in _flags(case)


def _sweep(op):
    got = {dw_code(op, 1, nc, H, W, s, al) for s in (1, 2) for H in range(1, 81) for W in range(1, 81) for nc in (4, 6) for al in (False, True)}
    got.discard(-1)
    return got


@pytest.mark.parametrize("op", [OP_FWD, OP_DGRAD, OP_WGRAD, OP_BWD])
def test_case_table_reaches_every_variant(op):
    cases = DW_CASES[op]
    for case in cases:
        code, N, C_, H, W, stride = case[:6]
        assert dw_code(op, N, C_, H, W, stride, _aligned(case)) == code, case
        if "loop" not in _flags(case):
            assert N <= 3 and C_ <= 12 and H <= 40 and W <= 72, case
    assert _sweep(op) == {c[0] for c in cases} == WANT[op]
    assert len(WANT[op]) == (13 if op in (OP_FWD, OP_BWD) else 6)
    # the query does not depend on how the N C planes split into images and channels
    assert all(dw_code(op, 2, 3, H, W, s, True) == dw_code(op, 1, 6, H, W, s, True) for s in (1, 2) for H in (8, 16, 37) for W in (16, 33, 70))


@pytest.mark.parametrize("op", [OP_FWD, OP_DGRAD, OP_WGRAD, OP_BWD])
def test_every_variant_has_a_plain_and_a_ragged_case(op):
    cases = DW_CASES[op]
    for code in sorted(WANT[op]):
        mine = [c for c in cases if c[0] == code]
        assert any(not _flags(c) for c in mine), (op, code, "no plain case")
        ragged = [c for c in mine if "ragged" in _flags(c)]
        assert ragged, (op, code, "no ragged case")
        for c in ragged:
            assert (c[1] * c[2]) % 8 != 0, c                # the padded grid's surplus planes return early
        if code >= 9000:
            continue
        tw, th, _ = dw_tile(code)
        for c in ragged:                                    # both axes off the tile
            ph, pw = dw_tiled_plane(op, c[3], c[4], c[5])
            assert ph % th != 0 and pw % tw != 0, c
        if op in (OP_FWD, OP_BWD) and code % 10 == 0:       # the element-wise forms: rows that are no whole float4s
            assert any(c[4] % 4 != 0 for c in ragged), (op, code)
    # two tiles along an axis on every tile width
    for tw in (64, 32, 16):
        assert any(c[0] < 9000 and dw_tile(c[0])[0] == tw and dw_tiles(op, c[0], c[3], c[4], c[5]) >= 2 for c in cases), (op, tw)
    # float4 staging above 64 columns: the last tile column is partly outside the plane
    v4_wide = {OP_FWD: (1641,), OP_BWD: (1641, 2641)}.get(op, ())
    for code in v4_wide:
        assert any(c[0] == code and dw_tiled_plane(op, c[3], c[4], c[5])[1] > 64 and dw_tiled_plane(op, c[3], c[4], c[5])[1] % 64 != 0
                   for c in cases), (op, code)
    # the narrowest plane that takes the 64-wide tile
    assert any(dw_tile(c[0])[0] == 64 and dw_tiled_plane(op, c[3], c[4], c[5])[1] == 33 for c in cases if c[0] < 9000), op


def test_required_edge_cases_are_present():
    # stride 2 from odd planes
    for cases in (DW_FWD_CASES, DW_DGRAD_CASES, DW_WGRAD_CASES):
        odd = [c for c in cases if c[5] == 2 and c[3] % 2 and c[4] % 2]
        assert any(c[4] > 32 for c in odd) and any(c[4] <= 16 for c in odd), "stride 2 with odd H and odd W, a wide and a narrow plane"
    # accumulation onto a pre-filled dx, at both strides
    assert {c[5] for c in DW_DGRAD_CASES if "accum" in _flags(c)} == {1, 2}
    # dy through the BatchNorm-backward prologue (ReLU6 mask) and through the affine one
    assert {"raw", "affine", "bnbwd6"} == {c[6] for c in DW_DGRAD_CASES} == {c[6][0] for c in DW_WGRAD_CASES} == {c[6][0] for c in DW_BWD_CASES}
    # inputs: RAW without activation, AFFINE with ReLU and with ReLU6
    assert {"raw", "affine_relu", "affine6"} == {c[6] for c in DW_FWD_CASES} == {c[6][1] for c in DW_WGRAD_CASES} == {c[6][1] for c in DW_BWD_CASES}
    # tensors offset by one float: a shape that is float4-eligible when aligned must answer the element-wise code, for every such code
    for op, cases in ((OP_FWD, DW_FWD_CASES), (OP_BWD, DW_BWD_CASES)):
        off = [c for c in cases if "offset" in _flags(c)]
        for c in off:
            aligned = dw_code(op, *c[1:6], True)
            assert c[0] % 10 == 0 and (aligned == c[0] + 1 or aligned == 9016), c
            assert any(d[0] == aligned and d[1:6] == c[1:6] for d in cases), (c, "the same shape also runs aligned")
        assert {c[0] for c in off} == {c for c in TILE_CODES}, op
        # the wave-per-plane kernel needs N C % 4 == 0: 16 x 16 planes fall back to the float4 16-wide tile
        fb = [c for c in cases if "plane_fallback" in _flags(c)]
        assert fb and all(c[0] == 1161 and c[3:6] == (16, 16, 1) and (c[1] * c[2]) % 4 for c in fb)
        assert any(c[0] == 9016 and (c[1] * c[2]) % 8 for c in cases)
    # the grid-stride loop of the filter-gradient kernel: a work-group stages at least two tiles, at each stride
    loops = [c for c in DW_WGRAD_CASES if "loop" in _flags(c)]
    assert {c[5] for c in loops} == {1, 2}
    for code, N, C_, H, W, stride, _, _ in loops:
        assert N * dw_tiles(OP_WGRAD, code, H, W, stride) > 4096 // C_ and wgrad_tiles_per_group(code, N, C_, H, W, stride) >= 2
    assert all(wgrad_tiles_per_group(*c[:6]) == 1 for c in DW_WGRAD_CASES if "loop" not in _flags(c))
    # the fused backward without the BatchNorm-backward sums, and with them on every variant
    assert any("nosums" in _flags(c) for c in DW_BWD_CASES)
    assert all("nosums" in _flags(c) for c in DW_BWD_CASES if c[6][1] == "raw")
    assert {c[0] for c in DW_BWD_CASES if "nosums" not in _flags(c)} == STAGED_CODES
    # 32 x 32 planes take the tile kernels (the plane kernels are for 16 x 16 only)
    assert all(dw_code(op, 2, 4, 32, 32, 1, True) == 1321 for op in (OP_FWD, OP_BWD))


def test_rejected_arguments():
    for op in (OP_FWD, OP_DGRAD, OP_WGRAD, OP_BWD):
        assert dw_code(op, 1, 8, 16, 16, 0) == -1 and dw_code(op, 1, 8, 16, 16, 3) == -1
    assert dw_code(4, 1, 8, 16, 16, 1) == -1 and dw_code(-1, 1, 8, 16, 16, 1) == -1
    # the fused backward owns 2 x 2 blocks of the input at stride 2
    for H, W in ((15, 16), (16, 15), (9, 13), (39, 37)):
        assert dw_code(OP_BWD, 1, 8, H, W, 2) == -1 and dw_code(OP_BWD, 1, 8, H, W, 1) > 0
        assert all(dw_code(op, 1, 8, H, W, 2) > 0 for op in (OP_FWD, OP_DGRAD, OP_WGRAD))


def test_chain_counts():
    """the fp32 chain lengths the GPU bounds use, written out for the cases that matter"""
    assert chain_wgrad(1640, 1, 8, 32, 64, 1) == 8 + 9 + 3 and chain_wgrad(1160, 8, 960, 8, 8, 1) == 2 * 1 + 9 + 3
    assert wgrad_tiles_per_group(2160, 8, 960, 16, 16, 2) == 2
    assert chain_tile(1641) == 8 + 9 + 3 and chain_tile(2161, 2) == 4 + 9 + 3 and chain_tile(2641, 2) == 8 + 9 + 3
    assert chain_tile(9016) == 4 + 6 + 3
