"""GPU tests of the coordinate plan at the sizes where the loops of its sort (egonn_amd/csrc/sort.hip) wrap — a sibling of
tests/test_gpu_maps.py, whose geometries stay below 8 500 rows (4 tiles of the sort).  What is compared, with np.array_equal:
the level-0 coordinates IN PLAN ORDER (the unique rows ordered by (batch, Morton code)), the row of the caller's input every
plan row names (the FIRST occurrence of a duplicated row or voxel: the sort is stable) and the batch offsets.

  coords_set   73 000 rows (70 000 distinct, 3 000 repeated) at coord_bits = 12, B = 3, scans of 20 000 / 45 000 / 5 000 rows:
               36 tiles = a second supertile of the flat sort, 38 key bits = 5 passes
  voxelize     65 535 and 65 536 points at coord_bits = 16: below 2^16 points the plan sorts packed elements (48 Morton bits
               << 16 | index inside the scan), from 2^16 on (key, value) pairs; eager and reserved (voxelize_device) plans.
               The 65 536th point is the last of the last scan and sits in a voxel of its own: apart from that voxel's row the
               two plans must be the same.

The Morton code, restated: bit 3 k of the code is bit k of x + 2^(coord_bits - 1), bit 3 k + 1 that of y, bit 3 k + 2 that of z."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as entry
    entry.build()
    import egonn_amd
    from egonn_amd import _lib
    egonn_amd._lib = _lib
    return egonn_amd


def morton(xyz, cb):
    u = (np.asarray(xyz, dtype=np.int64) + (1 << (cb - 1))).astype(np.uint64)
    assert (u < (1 << cb)).all()
    code = np.zeros(len(u), dtype=np.uint64)
    for k in range(cb):
        for axis in range(3):                                    # x in bit 0, y in bit 1, z in bit 2
            code |= ((u[:, axis] >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k + axis)
    return code


def plan_reference(c4, cb, B):
    """(b, x, y, z) rows in the caller's order -> (unique rows in plan order, index of each one's first occurrence, offsets)"""
    key = (c4[:, 0].astype(np.uint64) << np.uint64(3 * cb)) | morton(c4[:, 1:], cb)
    _, first = np.unique(key, return_index=True)                 # ascending key; the FIRST index of every key
    rows = c4[first]
    off = [int((rows[:, 0] < b).sum()) for b in range(B + 1)]
    return rows, first, off


def _check_plan(ctx, rows, index, off, what):
    assert ctx.level_count(0) == len(rows), (what, ctx.level_count(0), len(rows))
    got = ctx.level_coords(0).cpu().numpy()
    if not np.array_equal(got, rows):
        bad = np.flatnonzero((got != rows).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {len(rows)} level-0 rows differ from the (batch, Morton) order, first at "
                             f"{bad[:5].tolist()}: got {got[bad[0]].tolist()}, want {rows[bad[0]].tolist()}")
    idx = ctx.input_index().cpu().numpy()
    if not np.array_equal(idx, index):
        bad = np.flatnonzero(idx != index)
        raise AssertionError(f"{what}: input_index differs in {len(bad)} rows, first at {bad[:5].tolist()}: got "
                             f"{idx[bad[:5]].tolist()}, want the first occurrences {index[bad[:5]].tolist()}")
    assert ctx.level_batch_offsets(0) == off, (what, ctx.level_batch_offsets(0), off)
    ctx.plan_status()


def _distinct_cells(rng, n, lo, hi):
    c = np.unique(rng.integers(lo, hi, size=(n + n // 4, 3)), axis=0)
    assert len(c) >= n
    return c[rng.permutation(len(c))[:n]].astype(np.int32)


@pytest.mark.gpu
def test_coords_set_order_beyond_one_supertile(gpu):
    cb, B, sizes = 12, 3, (20000, 45000, 5000)
    rng = np.random.default_rng(70000)
    c4 = np.concatenate([np.column_stack([np.full(n, b, dtype=np.int32), _distinct_cells(rng, n, -2048, 2048)])
                         for b, n in enumerate(sizes)])
    rows_in = np.concatenate([c4, c4[rng.integers(0, len(c4), size=3000)]])
    rows_in = np.ascontiguousarray(rows_in[rng.permutation(len(rows_in))], dtype=np.int32)
    assert len(rows_in) == 73000 and len(np.unique(rows_in, axis=0)) == 70000 and max(sizes) > 16384
    rows, first, off = plan_reference(rows_in, cb, B)
    assert off == [0, 20000, 65000, 70000]
    ctx = gpu._lib.Context(coord_bits=cb)
    ctx.coords_set(torch.from_numpy(rows_in).cuda(), B)
    _check_plan(ctx, rows, first, off, "coords_set")


def _points(n_total):
    """B = 3 scans of voxel-centre points at step 1, several points per voxel; the first 65 535 points are the same whatever
    n_total is, a 65 536th is the last point of the last scan, alone in its voxel"""
    rng = np.random.default_rng(65535)
    sizes = (30000, 20000, 15535)
    scans = []
    for n in sizes:
        cells = _distinct_cells(rng, n // 2, -30000, 30000)                      # near the +-32768 range of coord_bits = 16
        scans.append(cells[rng.integers(0, len(cells), size=n)])
    if n_total == 65536:
        scans[2] = np.concatenate([scans[2], np.array([[32767, -32768, 32767]], dtype=np.int32)])
    assert sum(len(s) for s in scans) == n_total
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
    c4 = np.concatenate([np.column_stack([np.full(len(s), b, dtype=np.int32), s]) for b, s in enumerate(scans)])
    return c4, off


def _plan_from_points(gpu, way, c4, off):
    pts = torch.from_numpy(c4[:, 1:].astype(np.float32) + np.float32(0.5)).cuda()        # exact: |c| + 0.5 < 2^16
    ctx = gpu._lib.Context(coord_bits=16)
    if way == "voxelize":
        ctx.voxelize(pts, off.tolist(), 0, [1.0])
    else:
        ctx.reserve(len(pts), 3)            # the buffer holds exactly the points: its row count decides packed elements / pairs
        ctx.voxelize_device(pts, torch.from_numpy(off).cuda(), 3, 0, [1.0])
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("way", ["voxelize", "reserved"])
def test_plan_from_points_on_either_side_of_the_packed_sort(gpu, way):
    plans = {}
    for n_total in (65535, 65536):
        c4, off = _points(n_total)
        rows, first, boff = plan_reference(c4, 16, 3)
        index = first - off[rows[:, 0]]                                          # relative to each scan's first point
        assert index.min() == 0 and len(rows) < 0.6 * n_total                    # several points per voxel
        ctx = _plan_from_points(gpu, way, c4, off)
        _check_plan(ctx, rows, index, boff, f"{way} {n_total} points")
        plans[n_total] = (ctx.level_coords(0).cpu().numpy(), ctx.input_index().cpu().numpy())
    (ca, ia), (cb_, ib) = plans[65535], plans[65536]
    extra = np.flatnonzero((cb_ == [2, 32767, -32768, 32767]).all(axis=1))
    assert len(extra) == 1 and len(cb_) == len(ca) + 1 and ib[extra[0]] == 15535
    keep = np.arange(len(cb_)) != extra[0]
    assert np.array_equal(cb_[keep], ca) and np.array_equal(ib[keep], ia)
