"""Host test of the kernel choice of a 1x1 layer (dense_route / dense_launch, egonn_amd/csrc/dense.hip) through
egonn_debug_dense_route, which makes no device call: which of the five kernels a (rows, cin, cout, form) gets, its grid, its
dynamic LDS bytes and the column block of the persistent LDS kernel, on both sides of every threshold of the rule.  The expected
values are literals worked out by hand from the rule as DESIGN.md states it ("Host side of a 1x1 layer"), not computed by a copy
of it; the value tests (tests/test_gpu_dense_routes.py, tests/test_gpu_dense_stream.py) cannot see a moved threshold, this one
does.  Runs with EGONN_NO_DENSE_STREAM unset (the switch moves the streaming shapes to the persistent kernel)."""
import os

import pytest


@pytest.fixture(scope="module")
def route():
    assert "EGONN_NO_DENSE_STREAM" not in os.environ, "the expected routes are those of the product rule"
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    return _lib.debug_dense_route


# (rows, cin, cout, form) -> (route, grid x, grid y, LDS bytes, colblk); None = not pinned
CASES = [
    ((8192, 32, 64, -1), ("stream", 128, 1, 8964, 0)),
    ((8191, 32, 64, -1), ("small", 128, 1, 0, 0)),
    ((8192, 128, 128, -1), ("lds", 128, 1, 67072, 128)),          # 64 KB of weights: above the streaming form's 32 KB
    ((8192, 128, 64, 0), ("lds", 128, 1, 33536, 64)),
    ((8192, 128, 64, 1), ("stream", 128, 1, 33540, 0)),
    ((8192, 128, 64, -1), ("stream", 128, 1, 33540, 0)),
    ((2048, 192, 256, -1), ("lds", 32, 2, 99840, 128)),           # 192 KB: two column blocks of 96 KB, from 2048 rows on
    ((2047, 192, 256, -1), ("tile", 32, 4, 0, 0)),
    ((2048, 256, 256, -1), ("lds", 32, 3, 99456, 96)),            # 256 KB: three blocks of 96 columns, the last one ragged (64)
    ((8192, 96, 256, -1), ("lds", 128, 1, 101376, 256)),          # exactly 96 KB: one block
    ((4096, 96, 256, -1), ("small", 64, 4, 0, 0)),
    ((4096, 256, 64, -1), ("tile", 64, 1, 0, 0)),                 # below 8192 rows, but the small kernel stops at cin 128
    ((8192, 64, 100, -1), ("tile", 128, 2, 0, 0)),                # cout not a multiple of 16: no staged weights
    ((8191, 64, 100, -1), ("small", 128, 2, 0, 0)),
    ((8192, 64, 3, -1), ("tile", 128, 1, 0, 0)),
    ((5000, 48, 16, -1), ("plain", 313, 1, 0, 0)),                # no MFMA plan for cin 48: 80 000 outputs / 256 threads
    ((0, 32, 64, -1), ("none", 0, 0, 0, 0)),
    ((0, 128, 64, 1), ("none", 0, 0, 0, 0)),
    # the persistent grid is capped: 512 workgroups up to 72 KB per block, 256 above, divided among the column blocks
    ((1 << 20, 128, 128, -1), ("lds", 512, 1, 67072, 128)),
    ((1 << 20, 96, 256, -1), ("lds", 256, 1, 101376, 256)),
    ((1 << 20, 192, 256, -1), ("lds", 128, 2, 99840, 128)),
    ((1 << 20, 32, 64, -1), ("stream", 16384, 1, 8964, 0)),       # the streaming grid is not: one tile per wave
]


@pytest.mark.parametrize("shape,want", CASES, ids=[f"{s[0]}x{s[1]}-{s[2]}-form{s[3]}" for s, _ in CASES])
def test_route_grid_and_lds(route, shape, want):
    assert route(*shape) == want


@pytest.mark.parametrize("shape", [(8191, 128, 64, 1), (8192, 128, 128, 1), (8192, 96, 64, 1), (8192, 32, 32, 1)])
def test_streaming_form_on_another_shape_is_an_error(route, shape):
    from egonn_amd._lib import EgonnError
    with pytest.raises(EgonnError, match="no streaming form") as e:
        route(*shape)
    assert e.value.code == 1


def test_gate_scans_add_their_offsets_to_the_streaming_lds(route):
    plain, gated = route(8192, 32, 64), route(8192, 32, 64, gate_scans=16)
    assert gated[0] == plain[0] == "stream" and gated[3] == plain[3] + 64 and gated[:3] == plain[:3]
    # the persistent kernel reads the offsets from memory
    assert route(8192, 32, 64, form=0, gate_scans=16) == route(8192, 32, 64, form=0) == ("lds", 128, 1, 8960, 64)


# (cin, cout) whose gated ECA tail can be fused at 8192 rows: cout a multiple of 16 and cin * cout * 4 <= 96 KB
FUSABLE_AT_8192 = {(ci, 16) for ci in (32, 64, 96, 128, 192, 256)} | {(ci, 64) for ci in (32, 64, 96, 128, 192, 256)} | \
                  {(ci, 128) for ci in (32, 64, 96, 128, 192)} | {(32, 256), (64, 256), (96, 256)}


def test_gate_fusable_is_the_single_block_persistent_route(route):
    """dense_gate_fusable (what a gated call is checked against, and what the forward asks before it fuses a block tail): true
    exactly where form 0 gives the persistent LDS kernel with one column block"""
    from egonn_amd._lib import EgonnError
    for n in (8191, 8192):
        for cin in (32, 64, 96, 128, 192, 256):
            for cout in (16, 64, 100, 128, 256):
                want = n == 8192 and (cin, cout) in FUSABLE_AT_8192
                r = route(n, cin, cout, form=0)
                assert (r[0] == "lds" and r[2] == 1) == want, (n, cin, cout, r)
                try:
                    route(n, cin, cout, form=0, gate_scans=2)
                    fusable = True
                except EgonnError as e:
                    assert e.code == 1 and "fused gated residual needs the LDS-staged kernel" in str(e)
                    fusable = False
                assert fusable == want, (n, cin, cout)


def test_bad_arguments(route):
    from egonn_amd._lib import EgonnError
    for args in ((-1, 32, 64), (8192, 0, 64), (8192, 32, 0), (8192, 32, 64, 2), (8192, 32, 64, -2)):
        with pytest.raises(EgonnError, match="debug_dense_route: bad arguments"):
            route(*args)
