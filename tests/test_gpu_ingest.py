"""GPU tests of the device scan filter (egonn_amd/csrc/ingest.hip) where its three kernels change behaviour: the block
(1024 rows) and scan-pass (1024 blocks = 1 048 576 rows) boundaries, scan boundaries on and next to a block boundary,
`n` as a capacity, both strides, both switches, and values next to the two thresholds.  The filter only copies floats,
so every comparison is np.array_equal against oracle/ingest_ref.preprocess per scan: no tolerance anywhere."""
import numpy as np
import pytest
import torch

from tests import ends_data as E

pytestmark = pytest.mark.gpu
FILL = -777.25                       # what the tests put into the outputs first; nothing the filter could write there
EGONN_ERR_INVALID = 1


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    return _lib


def _call(lib, raw, offsets, ds="mulran", rz=True, rg=True, n=None, scratch_ints=None, stride=None):
    """egonn_filter_points through the C ABI on pre-filled outputs -> (rc, out (cap,3), new_off (B+1,)) as numpy"""
    from oracle.ingest_ref import GROUND_PLANE_LEVEL
    L = lib.load()
    dev = lib.require_gpu()
    n = len(raw) if n is None else n
    stride = raw.shape[1] if stride is None else stride
    d_raw = torch.from_numpy(raw).to(dev) if raw.size else torch.zeros(4, device=dev)
    d_off = torch.tensor(offsets, dtype=torch.int64, device=dev)
    cap = max(min(n, len(raw)), 1)
    out = torch.full((cap, 3), FILL, dtype=torch.float32, device=dev)
    new_off = torch.full((len(offsets),), -5, dtype=torch.int64, device=dev)
    ints = L.egonn_filter_points_scratch_ints(min(n, 1 << 24)) if scratch_ints is None else scratch_ints
    scratch = torch.zeros(max(ints, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = L.egonn_filter_points(d_raw.data_ptr(), n, stride, d_off.data_ptr(), len(offsets) - 1, int(rz), int(rg),
                                   float(GROUND_PLANE_LEVEL[ds]), out.data_ptr(), new_off.data_ptr(), scratch.data_ptr(),
                                   ints, lib._stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), new_off.cpu().numpy()


def _check(lib, raw, offsets, ds="mulran", rz=True, rg=True, n=None, what=None):
    from oracle import ingest_ref as I
    rc, out, new_off = _call(lib, raw, offsets, ds, rz, rg, n)
    assert rc == 0, what
    want, woff = I.filter_batch(raw, offsets, ds, rz, rg)
    assert new_off.tolist() == woff, what
    assert np.array_equal(out[:woff[-1]], want, equal_nan=True), what
    assert (out[woff[-1]:] == np.float32(FILL)).all(), what           # nothing written behind the survivors
    return woff[-1]


@pytest.mark.parametrize("total", [0, 1, 63, 64, 255, 256, 1023, 1024, 1025, 4096, 1024 * 1024 - 1, 1024 * 1024,
                                   1024 * 1024 + 1, 2 * 1024 * 1024 + 1029])
def test_row_counts_across_block_and_pass_boundaries(lib, total):
    """one scan, and the same rows cut into five scans at random places: survivors and offsets bit-exact.  From
    1 048 577 rows on the one-workgroup scan of the block counts runs a second pass and its carry decides where every
    later row lands."""
    raw, off = E.ingest_batch(total, 1, seed=total % 97)
    kept = _check(lib, raw, off, "kitti", what=("one scan", total))
    assert total < 64 or 0.2 * total < kept < 0.8 * total            # an irregular mask
    raw, off = E.ingest_batch(total, 5, seed=total % 89 + 1)
    _check(lib, raw, off, "mulran", what=("five scans", total))


def test_batch_shaped_like_config2(lib):
    """BASELINE.json configs[2]: 64 scans of about 50 k returns staged as one batch, 3.2 M rows = four scan passes"""
    rng = np.random.default_rng(64)
    sizes = rng.integers(48_000, 52_000, 64)
    off = [0] + np.cumsum(sizes).tolist()
    raw, off = E.ingest_batch(off[-1], 64, seed=64, offsets=off)
    assert off[-1] > 3 * 1024 * 1024
    _check(lib, raw, off, "mulran", what="configs[2]")


@pytest.mark.parametrize("offsets", [
    [0, 1024, 2048, 3072],                       # every boundary and the batch end on a block boundary
    [0, 1023, 2049, 3071],                       # one row before / after
    [0, 0, 1024, 1024, 1024, 3072, 3072],        # empty scans first, last and adjacent
    [0, 2048],                                   # a batch of one scan ending on a block boundary
    [0, 1],
    [0, 0],                                      # one empty scan
    [0, 0, 0, 0],
    [0, 1024 * 1024, 1024 * 1024 + 1024],        # a boundary on the scan-pass boundary
])
def test_scan_boundaries(lib, offsets):
    raw, off = E.ingest_batch(offsets[-1], len(offsets) - 1, seed=len(offsets), offsets=offsets)
    for ds in ("mulran", "southbay"):
        _check(lib, raw, off, ds, what=(offsets, ds))


def test_all_dropped_and_nothing_dropped(lib):
    raw, off = E.ingest_batch(5000, 4, seed=3)
    low = raw.copy()
    low[:, 2] = -50.0                                                # every point under the ground plane
    assert _check(lib, low, off, "kitti") == 0
    zero = np.zeros_like(raw)
    zero[:, 3] = 1.0                                                 # the reflectance is not a coordinate
    assert _check(lib, zero, off, "kitti", rg=False) == 0
    high = np.abs(np.nan_to_num(raw)) + np.float32(1.0)
    assert _check(lib, high, off, "kitti") == 5000
    assert _check(lib, raw, off, "kitti", rz=False, rg=False) == 5000   # both switches off: a copy, NaN rows included


@pytest.mark.parametrize("extra", [1, 1024, 1024 * 1024 + 5])
def test_capacity_rows_behind_the_end_are_never_read(lib, extra):
    """n is a capacity: the rows behind scan_offsets[B] hold points that every setting would keep; none may appear, the
    offsets must not count them and the output behind the survivors stays as it was"""
    for total, offsets in ((5000, None), (2048, [0, 1024, 2048]), (0, [0, 0])):
        raw, off = E.ingest_batch(total, 3, seed=extra % 7, extra=extra, offsets=offsets)
        assert len(raw) == total + extra and (raw[total:, :3] == 5.0).all()
        kept = _check(lib, raw, off, "mulran", n=total + extra, what=(total, extra))
        assert kept <= total


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("rz", [True, False])
@pytest.mark.parametrize("rg", [True, False])
def test_strides_switches_and_levels(lib, stride, rz, rg):
    from oracle.ingest_ref import GROUND_PLANE_LEVEL
    raw, off = E.ingest_batch(7001, 3, seed=11, stride=stride)
    counts = set()
    for ds in GROUND_PLANE_LEVEL:
        counts.add(_check(lib, raw, off, ds, rz, rg, what=(stride, rz, rg, ds)))
    assert len(counts) == (3 if rg else 1)                           # the three levels cut differently


@pytest.mark.parametrize("ds", ["mulran", "kitti", "southbay"])
def test_threshold_values(lib, ds):
    """values placed by hand on, and one float32 step to either side of, |v| <= 1e-8 and z > level; +-0, subnormals,
    NaN and +-inf in every coordinate: the expected mask is numpy's (np.isclose / >, the reference's lines), and the host
    suite checks that restatement against a plain loop over the rows"""
    from oracle import ingest_ref as I
    raw = E.threshold_scan(ds)
    for rz in (True, False):
        for rg in (True, False):
            kept = _check(lib, raw, [0, len(raw)], ds, rz, rg, what=(ds, rz, rg))
            assert kept == int(I.keep_loop(raw, ds, rz, rg).sum())
    _check(lib, np.ascontiguousarray(raw[:, :3]), [0, 700, len(raw)], ds, what=(ds, "stride 3"))


def test_error_paths_leave_the_outputs_untouched(lib):
    raw, off = E.ingest_batch(3000, 2, seed=5)
    L = lib.load()
    need = L.egonn_filter_points_scratch_ints(3000)
    assert need == 3 + 2                                             # 3 blocks, the total, one spare
    for kw in (dict(stride=2), dict(stride=5), dict(scratch_ints=need - 1), dict(n=1 << 31), dict(n=-1)):
        rc, out, new_off = _call(lib, raw, off, **kw)
        assert rc == EGONN_ERR_INVALID, kw
        assert (out == np.float32(FILL)).all() and (new_off == -5).all(), kw
    assert _call(lib, raw, off, scratch_ints=need)[0] == 0


def test_wrapper_on_empty_and_large_batches(lib):
    """ScanIngest (pinned staging + the C call): a batch whose scans are all empty, and one above a scan pass"""
    from egonn_amd.ingest import ScanIngest
    from oracle import ingest_ref as I
    dev = lib.require_gpu()
    ing = ScanIngest("kitti", dev)
    pts, off = ing([np.zeros((0, 4), np.float32)] * 3)
    assert off == [0, 0, 0, 0] and pts.shape == (0, 3)
    raw, roff = E.ingest_batch(1024 * 1024 + 3000, 3, seed=21)
    pts, off = ing([raw[lo:hi] for lo, hi in zip(roff[:-1], roff[1:])])
    want, woff = I.filter_batch(raw, roff, "kitti")
    assert off == woff and np.array_equal(pts.cpu().numpy(), want, equal_nan=True)
    pts, off = ing([raw[:5000]])                                     # the staging buffer is reused: nothing of the big batch
    want, woff = I.filter_batch(raw[:5000], [0, 5000], "kitti")
    assert off == woff and np.array_equal(pts.cpu().numpy(), want, equal_nan=True)
