"""The GPU case tables of tests/test_gpu_dispatch_variants.py reach EVERY kernel variant the pointwise dispatchers can select (no GPU).

Each dispatcher asks a host-only query which template instantiation a shape gets (sc_conv1x1_pw3_variant, sc_wgrad_pw3_variant,
sc_irb_variant, sc_pw_stream_variant) and launches what the query says.  Here each query is swept over the shapes its entry point
accepts, and the set of codes it returns must EQUAL the set of codes of the case table: deleting a case, or a dispatcher gaining a
branch without a case, fails this test; so does a table entry whose shape no longer selects the code written next to it."""
from test_gpu_dispatch_variants import (IRB_RESIDUAL_ACT_CASES, IRB_VARIANT_CASES, PW3_VARIANT_CASES, PW3_WGRAD_VARIANT_CASES,
                                        PWS_DGRAD_VARIANT_CASES, PWS_VARIANT_CASES, irb_code, pw3_code, pw3_wgrad_code, pws_code)


def test_pw3_case_table_reaches_every_variant():
    swept = {pw3_code(1, 1, nhw, cout) for cout in range(8, 1281, 8) for nhw in range(1, 2 ** 17 + 1, 31)}
    swept |= {pw3_code(1, 1, nhw, cout) for cout in (8, 40, 96, 136, 384, 1280) for nhw in (2 ** 17 - 1, 2 ** 17)}
    for ncb, K, M, N, H, W in PW3_VARIANT_CASES:
        assert pw3_code(N, H, W, M) == ncb, (ncb, K, M, N, H, W)
    assert swept == {c[0] for c in PW3_VARIANT_CASES} == {1, 2, 4}
    # the edges the table is there for, per variant: a ragged last 32-pixel block with H W % 4 != 0, and a last cout group with
    # fewer than ncb valid blocks
    for ncb in (1, 2, 4):
        mine = [c for c in PW3_VARIANT_CASES if c[0] == ncb]
        assert any((N * H * W) % 32 and (H * W) % 4 for _, K, M, N, H, W in mine), ncb
        assert ncb == 1 or any(-(-M // 32) % ncb for _, K, M, N, H, W in mine), ncb
    assert pw3_code(0, 4, 4, 8) == -1 and pw3_code(1, 4, 4, 0) == -1


def test_pw3_wgrad_case_table_reaches_every_variant():
    swept = {pw3_wgrad_code(n, 4, 6, cout, cin) for n in (1, 2, 64) for cout in range(8, 129, 8) for cin in range(8, 129, 8)}
    for code, cin, cout, N, H, W in PW3_WGRAD_VARIANT_CASES:
        assert pw3_wgrad_code(N, H, W, cout, cin) == code and (H * W) % 8 == 0, (code, cin, cout, N, H, W)
    assert swept == {c[0] for c in PW3_WGRAD_VARIANT_CASES} == {11, 12, 21, 22}
    assert pw3_wgrad_code(1, 4, 6, 0, 8) == -1


def test_irb_case_table_reaches_every_variant():
    swept = {irb_code(cin, hid, cout, s) for cin in range(8, 161, 8) for hid in range(32, 961, 32) for cout in range(8, 385, 8) for s in (1, 2)}
    swept.discard(-1)
    for case in IRB_VARIANT_CASES:
        code, (N, cin, hid, cout, H, W) = case[0], case[1:7]
        assert irb_code(cin, hid, cout, case[9] if len(case) > 9 else 1) == code, case
        assert N <= 2 and H <= 16 and W <= 16, case
    assert swept == {c[0] for c in IRB_VARIANT_CASES}
    assert len(swept) == 30 and not any(c // 10000 == 2 for c in swept)      # tiling C: behind the development knob only
    for tiling in (0, 1, 3):          # a plane off the tile with W % 4 != 0 on every tiling
        assert any(c[0] // 10000 == tiling and c[5] % 4 and c[6] % 4 for c in IRB_VARIANT_CASES), tiling
    assert any(c[0] % 1000 // 10 == 10 and c[2] % 16 for c in IRB_VARIANT_CASES)      # Cin % 16 != 0 at NKE 10
    for code, N, C_, hid, H, W, act in IRB_RESIDUAL_ACT_CASES:
        assert irb_code(C_, hid, C_, 1) == code and act != 0
    assert {c[5] % 4 == 0 for c in IRB_RESIDUAL_ACT_CASES} == {True, False}      # both store paths of the epilogue
    assert irb_code(320, 1280, 64, 1) == -1 and irb_code(160, 960, 320, 2) == -1 and irb_code(64, 100, 64, 1) == -1


def test_streaming_case_tables_reach_every_variant():
    swept = {(bnb, pws_code(1, K, M, 64, 64, bnb)) for bnb in (False, True) for K in (16, 24, 32) for M in range(8, 193, 8)}
    fwd, bwd = {c for b, c in swept if not b and c >= 0}, {c for b, c in swept if b and c >= 0}
    for code, N, cin, cout, H, W, mode in PWS_VARIANT_CASES:
        assert pws_code(N, cin, cout, H, W, False, stats=True) == code, (code, N, cin, cout, H, W, mode)
    for code, N, cin, cout, H, W, act in PWS_DGRAD_VARIANT_CASES:
        assert pws_code(N, cout, cin, H, W, True) == code, (code, N, cin, cout, H, W, act)
    assert fwd == {c[0] for c in PWS_VARIANT_CASES} and len(fwd) == 8
    assert bwd == {c[0] for c in PWS_DGRAD_VARIANT_CASES} and len(bwd) == 12
    # just past a block-count edge: most of the wave's 16-channel output blocks are padding
    assert any(c[0] // 10 == 5 and c[3] == 40 for c in PWS_VARIANT_CASES) and any(c[0] // 10 == 13 and c[2] == 33 for c in PWS_DGRAD_VARIANT_CASES)
    # what the streaming kernel does not take
    assert pws_code(1, 16, 16, 64, 64, False) == -1          # forward: 24 or 32 input channels only
    assert pws_code(1, 32, 200, 64, 64, False) == -1 and pws_code(1, 32, 16, 32, 32, False) == -1 and pws_code(1, 32, 16, 72, 72, False) == -1
    assert pws_code(1, 24, 96, 64, 64, True, stats=True) == -1      # no statistics epilogue behind a BatchNorm-backward source
    assert pws_code(1, 24, 96, 64, 64, True, base=(1 << 20) + 4) == -1
