"""GPU tests of the voxel map (run with -m gpu on an MI355X): csrc/voxel_map.hip and egonn_amd/mapping.py against the numpy
restatement tests/voxel_map_ref.py, bit for bit: integrate at the wave and tile edges, on voxel faces, at the ends of the
index range, with dropped points, bad picks and short capacities; merge of disjoint, identical, interleaved and empty record
sets; insertion in batches and in reversed order; select with filters, faces, overlapping boxes and overflow; eager against a
replayed graph; and the seam to the ICP: scan-to-map refinement moves a perturbed pose towards the planted one."""
import ctypes

import numpy as np
import pytest
import torch

from tests import voxel_map_ref as ref

pytestmark = pytest.mark.gpu

VOXEL = 0.25
ORIGIN = np.array([0.5, -1.25, 0.125])
CANARY = 5                                   # rows behind every output buffer that no call may touch
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


@pytest.fixture(scope="module")
def scene():
    return ref.random_scene()


def _np(t):
    return t.detach().cpu().numpy()


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _c3(v):
    return (ctypes.c_double * 3)(*[float(x) for x in v])


def _scratch(nbytes):
    assert nbytes > 0
    s = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device="cuda")
    assert s.data_ptr() % 256 == 0
    return s


def _alloc(rows):
    """record buffers of `rows` rows + CANARY rows, every byte a pattern"""
    r = {"keys": torch.full((rows + CANARY,), FILL, dtype=torch.int64, device="cuda"),
         "sums": torch.full((rows + CANARY, 3), FILL, dtype=torch.int64, device="cuda"),
         "count": torch.full((rows + CANARY,), FILL, dtype=torch.int32, device="cuda"),
         "obs": torch.full((rows + CANARY,), FILL, dtype=torch.int32, device="cuda"),
         "n": torch.full((), -7, dtype=torch.int64, device="cuda"), "rows": rows}
    return r


def _ptrs(r):
    return r["keys"].data_ptr(), r["sums"].data_ptr(), r["count"].data_ptr(), r["obs"].data_ptr()


def _upload(rec, rows=None):
    n = len(rec["keys"])
    r = _alloc(n if rows is None else rows)
    r["keys"][:n] = _cu(rec["keys"].astype(np.int64))
    r["sums"][:n] = _cu(rec["sums"])
    r["count"][:n] = _cu(rec["count"])
    r["obs"][:n] = _cu(rec["obs"])
    r["n"].fill_(n)
    return r


def _download(r, status=0):
    n = int(r["n"])
    assert 0 <= n <= r["rows"]
    out = {"keys": _np(r["keys"][:n]).astype(np.uint64), "sums": _np(r["sums"][:n]), "count": _np(r["count"][:n]),
           "obs": _np(r["obs"][:n]), "status": int(status)}
    return out


def _untouched(r, start):
    """rows from `start` on still hold the pattern"""
    return all(bool((r[f][start:] == FILL).all()) for f in ref.FIELDS)


def _integrate(pts, off, pick, poses, origin=ORIGIN, voxel=VOXEL, points_capacity=None, capacity=None):
    from egonn_amd import _lib
    lib = _lib.load()
    pts, off = np.asarray(pts, np.float64).reshape(-1, 3), np.asarray(off, np.int64)
    if points_capacity is None:
        points_capacity = int(sum(off[p + 1] - off[p] for p in pick if 0 <= p < len(off) - 1))
    capacity = points_capacity if capacity is None else capacity
    out = _alloc(capacity)
    status = torch.zeros((), dtype=torch.int32, device="cuda")
    bank, offs, pk, ps = _cu(pts), _cu(off), _cu(np.asarray(pick, np.int32)), _cu(np.asarray(poses, np.float64))
    s = _scratch(lib.egonn_voxel_map_integrate_scratch_bytes(points_capacity, len(pick)))
    _lib.call(bank.device, lib.egonn_voxel_map_integrate, bank.data_ptr() if len(pts) else None, len(pts), offs.data_ptr(),
              len(off) - 1, pk.data_ptr(), ps.data_ptr(), len(pick), _c3(origin), float(voxel), points_capacity, *_ptrs(out), capacity,
              out["n"].data_ptr(), status.data_ptr(), s.data_ptr(), s.numel() * 8)
    torch.cuda.synchronize()
    got = _download(out, status)
    assert _untouched(out, max(len(got["keys"]), 0) if got["status"] & ref.CAPACITY else capacity), "rows behind the capacity were written"
    return got, out


def _check_integrate(pts, off, pick, poses, origin=ORIGIN, voxel=VOXEL):
    got, _ = _integrate(pts, off, pick, poses, origin, voxel)
    want = ref.integrate(pts, off, pick, poses, origin, voxel)
    assert got["status"] == want["status"], (got["status"], want["status"])
    assert ref.same(got, want)
    return want


def _split(n, parts):
    """offsets of `parts` clouds that hold n points together (uneven, some may be empty)"""
    cuts = sorted(np.random.default_rng(n).integers(0, n + 1, size=parts - 1).tolist())
    return np.array([0] + cuts + [n], np.int64)


def _shifts(parts, step=0.0):
    poses = np.tile(np.eye(4), (parts, 1, 1))
    poses[:, 0, 3] = step * np.arange(parts)
    return poses


# ------------------------------------------------------------------ integrate
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025, 65536, 65537])
def test_integrate_at_the_wave_and_tile_edges(gpu, n):
    """n points in three clouds: every point in its own voxel, all points in one voxel, and a clustered mix.  65 536 and 65 537
    points are 256 and 257 workgroups: in the one-workgroup scan of their head counts a thread owns one counter, then two"""
    rng = np.random.default_rng(n)
    off, poses = _split(n, 3), _shifts(3)
    side = max(40, int(np.ceil(np.sqrt(n))))                     # side * side >= n cells
    cells = rng.permutation(side * side)[:n]
    own = np.stack([cells // side - side // 2, cells % side - side // 2, rng.integers(-3, 3, n)], axis=1) * VOXEL \
        + rng.uniform(0.01, 0.24, (n, 3)) + ORIGIN
    want = _check_integrate(own, off, [0, 1, 2], poses)
    assert len(want["keys"]) == n and (want["count"] == 1).all()
    one = ORIGIN + np.array([-3, 2, 5]) * VOXEL + rng.uniform(0.0, VOXEL * 0.999, (n, 3))
    want = _check_integrate(one, off, [0, 1, 2], poses)
    assert len(want["keys"]) == 1 and want["count"][0] == n and want["obs"][0] == (np.diff(off) > 0).sum()
    mix = rng.uniform(-2, 2, (12, 3))[rng.integers(0, 12, n)] + rng.normal(0, 0.2, (n, 3))
    want = _check_integrate(mix, off, [2, 0, 1], _shifts(3, 0.07))
    assert want["count"].sum() == n


def test_integrate_runs_across_tiles(gpu):
    """a voxel of 300 points between single-point voxels (its run crosses a wave and a 256-point boundary wherever it starts),
    and runs that begin on the last lane of a wave (sorted position 63) and of a 256-point tile (position 255)"""
    rng = np.random.default_rng(3)
    inside = lambda m: rng.uniform(0.0, VOXEL * 0.999, (m, 3))                 # noqa: E731
    singles = lambda m, x0: np.stack([np.arange(m) + x0, np.zeros(m), np.zeros(m)], axis=1) * VOXEL + inside(m)   # noqa: E731
    for lead in (0, 10, 63, 200, 255):
        pts = np.concatenate([singles(lead, -400), np.array([1, 0, 0]) * VOXEL + inside(300), singles(17, 50)]) + ORIGIN
        pts = pts[rng.permutation(len(pts))]
        want = _check_integrate(pts, _split(len(pts), 4), [0, 1, 2, 3], _shifts(4))
        assert want["count"].max() == 300 and len(want["keys"]) == lead + 18
    for lead, run in ((63, 5), (255, 5), (63, 200), (255, 700), (127, 2)):
        pts = np.concatenate([singles(lead, -400), np.array([1, 0, 0]) * VOXEL + inside(run)]) + ORIGIN
        want = _check_integrate(pts[rng.permutation(len(pts))], _split(len(pts), 2), [0, 1], _shifts(2))
        assert want["count"][-1] == run and len(want["keys"]) == lead + 1


def test_integrate_on_faces_and_signs(gpu):
    """coordinates exactly on voxel faces (k * voxel), negative ones, -0.0, and s = -1e-20, which floors to -1 with a residual
    that rounds to 1.0 and is clamped to 2^30 - 1"""
    k = np.arange(-6, 7, dtype=np.float64)
    faces = np.stack(np.meshgrid(k, k[:3], k[-2:], indexing="ij"), axis=-1).reshape(-1, 3) * VOXEL
    odd = np.array([[-0.0, 0.0, -0.0], [-1e-20 * VOXEL, -1e-20 * VOXEL, 1e-20], [-VOXEL, -2 * VOXEL, -1e-300], [1e-310, -1e-310, 0.0]])
    pts = np.concatenate([faces, odd, -faces[:20] - 1e-9, faces[:20] + 1e-9])
    zero = np.zeros(3)
    want = _check_integrate(pts, [0, 40, len(pts)], [0, 1], _shifts(2), origin=zero)
    key, q, valid = ref.point_keys(odd[1:2], np.eye(4), zero, VOXEL)
    assert ref.indices(key).tolist() == [[-1, -1, 0]] and q[0, :2].tolist() == [ref.ONE - 1] * 2 and key[0] in want["keys"]
    c = ref.centroids(want, zero, VOXEL)
    assert (c >= ref.indices(want["keys"]) * VOXEL).all() and (c < (ref.indices(want["keys"]) + 1) * VOXEL).all()


def test_integrate_at_utm_sized_poses(gpu, scene):
    bank, off, poses = scene
    org = np.array([3e5, 4e6, 50.0])
    far = poses.copy()
    far[:, :3, 3] += org + np.array([123.456, -789.012, 3.3])
    want = _check_integrate(bank, off, np.arange(7), far, origin=org, voxel=0.2)
    assert len(want["keys"]) > 100 and (want["obs"] > 2).any()


def test_integrate_index_range_and_dropped_points(gpu):
    """voxel = 1: index 2^20 - 1 is kept and 2^20 dropped, -2^20 kept and -2^20 - 1 dropped, on every axis; NaN and inf are
    dropped; RANGE is set and every other record is what it is without the dropped points"""
    rng = np.random.default_rng(8)
    good = rng.uniform(-50, 50, (200, 3))
    hi, lo = float(2 ** 20), -float(2 ** 20)
    edge = []
    for a in range(3):
        for v in (hi - 0.5, hi, hi + 0.25, lo, lo + 0.5, lo - 1e-9, lo - 1.0):
            p = [1.5, 2.5, 3.5]
            p[a] = v
            edge.append(p)
    bad = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [1e300, 0, 0]]
    pts = np.concatenate([good[:100], edge, good[100:], bad])
    pts = pts[rng.permutation(len(pts))]
    zero = np.zeros(3)
    want = _check_integrate(pts, [0, 90, len(pts)], [0, 1], _shifts(2), origin=zero, voxel=1.0)
    assert want["status"] == ref.RANGE
    idx = ref.indices(want["keys"])
    assert idx.max() == 2 ** 20 - 1 and idx.min() == -(2 ** 20) and want["count"].sum() == 200 + 3 * 3
    keep = np.isfinite(pts).all(axis=1) & (np.floor(pts) >= lo).all(axis=1) & (np.floor(pts) < hi).all(axis=1)
    clean = ref.integrate(pts[keep], [0, int(keep[:90].sum()), int(keep.sum())], [0, 1], _shifts(2), zero, 1.0)
    assert clean["status"] == 0 and ref.same(clean, want)


def test_integrate_picks_and_observations(gpu, scene):
    bank, off, poses = scene
    # a pick outside the bank contributes nothing
    got, _ = _integrate(bank, off, [0, 7, 1, -1], poses[[0, 1, 1, 2]])
    want = ref.integrate(bank, off, [0, 7, 1, -1], poses[[0, 1, 1, 2]], ORIGIN, VOXEL)
    assert got["status"] == want["status"] == ref.BAD_INDEX and ref.same(got, want)
    assert ref.same(got, ref.integrate(bank, off, [0, 1], poses[[0, 1]], ORIGIN, VOXEL))
    # the same cloud twice under the same pose: two observations of every voxel, twice the points
    once, twice = _check_integrate(bank, off, [2], poses[[2]]), _check_integrate(bank, off, [2, 2], poses[[2, 2]])
    assert np.array_equal(once["keys"], twice["keys"]) and (once["obs"] == 1).all() and (twice["obs"] == 2).all()
    assert np.array_equal(twice["sums"], 2 * once["sums"]) and np.array_equal(twice["count"], 2 * once["count"])
    # a voxel seen by observations 0 and 2 only (observation 1 is elsewhere; 3 is the empty cloud)
    v = ORIGIN + np.array([4, 4, 4]) * VOXEL
    pts = np.concatenate([v + [[0.01, 0.02, 0.03], [0.2, 0.1, 0.1]], v + 40.0 + np.zeros((3, 3)), v + [[0.1, 0.1, 0.1]] * 4])
    want = _check_integrate(pts, [0, 2, 5, 9, 9], [0, 1, 2, 3], _shifts(4))
    assert want["count"].tolist() == [6, 3] and want["obs"].tolist() == [2, 1]


def test_integrate_capacity_one_short(gpu, scene):
    bank, off, poses = scene
    want = ref.integrate(bank, off, np.arange(7), poses, ORIGIN, VOXEL)
    n, total = len(want["keys"]), int(off[-1])
    got, buf = _integrate(bank, off, np.arange(7), poses, capacity=n)
    assert got["status"] == 0 and ref.same(got, want)
    got, buf = _integrate(bank, off, np.arange(7), poses, capacity=n - 1)                 # one voxel too many
    assert got["status"] == ref.CAPACITY and int(buf["n"]) == 0 and _untouched(buf, 0), "nothing is written"
    got, buf = _integrate(bank, off, np.arange(7), poses, points_capacity=total - 1, capacity=total)      # one point too many
    assert got["status"] == ref.CAPACITY and int(buf["n"]) == 0 and _untouched(buf, 0)
    short = ref.integrate(bank, off, np.arange(7), poses, ORIGIN, VOXEL, points_capacity=total - 1)
    assert short["status"] == ref.CAPACITY and len(short["keys"]) == 0


# ------------------------------------------------------------------ merge
def _random_records(rng, keys):
    keys = np.sort(np.asarray(keys, np.uint64))
    n = len(keys)
    count = rng.integers(1, 5000, n).astype(np.int32)
    return {"keys": keys, "sums": rng.integers(0, ref.ONE, (n, 3)) * count[:, None].astype(np.int64), "count": count,
            "obs": rng.integers(1, 40, n).astype(np.int32), "status": 0}


def _merge(A, B, capacity_out=None, rows_a=None, rows_b=None):
    from egonn_amd import _lib
    lib = _lib.load()
    a, b = _upload(A, rows_a), _upload(B, rows_b)
    capacity_out = a["rows"] + b["rows"] if capacity_out is None else capacity_out
    out = _alloc(capacity_out)
    status = torch.zeros((), dtype=torch.int32, device="cuda")
    s = _scratch(lib.egonn_voxel_map_merge_scratch_bytes(a["rows"], b["rows"], capacity_out))
    _lib.call(out["keys"].device, lib.egonn_voxel_map_merge, *_ptrs(a), a["n"].data_ptr(), a["rows"], *_ptrs(b), b["n"].data_ptr(),
              b["rows"], *_ptrs(out), capacity_out, out["n"].data_ptr(), status.data_ptr(), s.data_ptr(), s.numel() * 8)
    torch.cuda.synchronize()
    assert _untouched(out, capacity_out) and _untouched(a, len(A["keys"])) and _untouched(b, len(B["keys"]))
    assert ref.same(_download(a), A) and ref.same(_download(b), B), "the inputs are read only"
    return _download(out, status), out


@pytest.mark.parametrize("n", [1, 64, 65, 256, 257, 65537])
def test_merge_key_sets(gpu, n):
    """65 537 rows are 257 workgroups: the scan of the B-only counts and the ranks behind it with two counters per thread"""
    rng = np.random.default_rng(n)
    pool = np.unique(rng.integers(0, 2 ** 63 - 1, 4 * n + 8, dtype=np.int64).astype(np.uint64))
    pool = pool[rng.permutation(len(pool))]
    A = _random_records(rng, pool[:n])
    cases = {"disjoint": _random_records(rng, pool[n: 2 * n]), "identical": _random_records(rng, pool[:n]),
             "interleaved": _random_records(rng, np.concatenate([pool[: n // 2 + 1], pool[2 * n: 3 * n]])),
             "below": _random_records(rng, np.arange(n, dtype=np.uint64)), "empty": ref.empty()}
    for name, B in cases.items():
        for X, Y in ((A, B), (B, A)):
            got, _ = _merge(X, Y)
            want = ref.merge(X, Y)
            assert got["status"] == 0 and ref.same(got, want), name
            got, _ = _merge(X, Y, capacity_out=len(want["keys"]), rows_a=len(X["keys"]), rows_b=len(Y["keys"]) + 3)
            assert got["status"] == 0 and ref.same(got, want), name                        # exactly full


def test_merge_overflow_keeps_a(gpu):
    rng = np.random.default_rng(2)
    pool = np.unique(rng.integers(0, 2 ** 63 - 1, 1000, dtype=np.int64).astype(np.uint64))
    A, B = _random_records(rng, pool[:300]), _random_records(rng, pool[250:520])
    union = len(np.union1d(A["keys"], B["keys"]))
    got, out = _merge(A, B, capacity_out=union - 1)
    assert got["status"] == ref.CAPACITY and ref.same(got, A) and _untouched(out, len(A["keys"]))
    got, _ = _merge(A, B, capacity_out=union)
    assert got["status"] == 0 and ref.same(got, ref.merge(A, B))


def _bank_of(gpu, pts, off):
    bank = gpu.CloudBank()
    bank.points = _cu(np.asarray(pts, np.float64).reshape(-1, 3))
    bank.host_offsets = [int(v) for v in off]
    return bank


def _map_records(vm):
    R = vm.records
    n = int(R["n"])
    return {"keys": _np(R["keys"][:n]).astype(np.uint64), "sums": _np(R["sums"][:n]), "count": _np(R["count"][:n]),
            "obs": _np(R["obs"][:n]), "status": vm.status}


@pytest.mark.parametrize("reserved", [False, True])
def test_insert_in_batches_and_reversed(gpu, scene, reserved):
    """VoxelMap.insert in 1, 2 and 5 batches, forwards and backwards, and in chunks forced by a small point budget: the records
    of one call, bit for bit, which are the restatement's"""
    bank_np, off, poses = scene
    bank = _bank_of(gpu, bank_np, off)
    pick = np.array([0, 1, 2, 3, 4, 5, 6, 2, 0])
    ps = poses[pick]
    want = ref.integrate(bank_np, off, pick, ps, ORIGIN, VOXEL)
    kw = dict(voxel_size=VOXEL, origin=ORIGIN, capacity=len(want["keys"]) + 9 if reserved else None)
    one = _map_records(gpu.VoxelMap(**kw).insert(bank, ps, pick))
    assert one["status"] == 0 and ref.same(one, want)
    for batches in (2, 5):
        for order in (np.arange(len(pick)), np.arange(len(pick))[::-1]):
            vm = gpu.VoxelMap(**kw)
            for part in np.array_split(order, batches):
                vm.insert(bank, ps[part], pick[part])
            assert ref.same(_map_records(vm), want) and vm.n_voxels == len(want["keys"]), (batches, order[0])
    vm = gpu.VoxelMap(chunk_points=400, **kw).insert(bank, ps, pick)
    assert ref.same(_map_records(vm), want)
    if reserved:                                                    # a chunk that does not fit is dropped whole, the map keeps its records
        small = gpu.VoxelMap(VOXEL, ORIGIN, capacity=len(want["keys"]) - 1)
        small.insert(bank, ps[:4], pick[:4])
        held = _map_records(small)
        assert held["status"] == 0 and ref.same(held, ref.integrate(bank_np, off, pick[:4], ps[:4], ORIGIN, VOXEL))
        small.insert(bank, ps[4:], pick[4:])
        assert small.status == ref.CAPACITY and ref.same(_map_records(small), held)
    else:
        assert ref.same(_map_records(gpu.build_map(bank, poses, VOXEL, origin=ORIGIN)), ref.integrate(bank_np, off, np.arange(7), poses, ORIGIN, VOXEL))


@pytest.mark.parametrize("n_obs", [257, 513])
def test_insert_more_observations_than_scan_threads(gpu, n_obs):
    """one call with 257 and 513 observations of a handful of points each, every seventh cloud empty and some clouds picked
    twice: the one-workgroup scan of the clouds' sizes gives a thread two, then three observations"""
    rng = np.random.default_rng(n_obs)
    sizes = rng.integers(1, 9, n_obs)
    sizes[::7] = 0
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pts = rng.uniform(-3, 3, (int(off[-1]), 3)) + ORIGIN
    pick = np.arange(n_obs)
    pick[5::50] = 3
    poses = _shifts(n_obs, 0.013)
    want = ref.integrate(pts, off, pick, poses, ORIGIN, VOXEL)
    assert want["status"] == 0 and want["count"].sum() == sizes[pick].sum() and want["obs"].max() > 1
    got = _map_records(gpu.VoxelMap(VOXEL, ORIGIN).insert(_bank_of(gpu, pts, off), poses, pick))
    assert got["status"] == 0 and ref.same(got, want)
    _check_integrate(pts, off, pick, poses)                            # the entry point itself, its buffers exactly full


# ------------------------------------------------------------------ select
def _scene_map(gpu, scene):
    bank_np, off, poses = scene
    pick = np.array([0, 1, 2, 4, 5, 6, 2])
    want = ref.integrate(bank_np, off, pick, poses[pick], ORIGIN, VOXEL)
    vm = gpu.VoxelMap(VOXEL, ORIGIN).insert(_bank_of(gpu, bank_np, off), poses[pick], pick)
    return vm, want


def _same_points(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def test_select_filters_boxes_and_offsets(gpu, scene):
    vm, rec = _scene_map(gpu, scene)
    c = ref.centroids(rec, ORIGIN, VOXEL)
    for mc, mo in ((1, 1), (2, 1), (1, 2), (3, 3), (10 ** 6, 1)):
        got = vm.points(mc, mo)
        want = ref.select(rec, ORIGIN, VOXEL, mc, mo)
        assert _same_points(_np(got["points"]), want["points"]) and np.array_equal(_np(got["count"]), want["count"])
        assert np.array_equal(_np(got["observations"]), want["obs"])
    assert len(ref.select(rec, ORIGIN, VOXEL, 2, 1)["points"]) not in (0, len(c)) and len(ref.select(rec, ORIGIN, VOXEL, 1, 2)["points"]) not in (0, len(c))
    # boxes: two that overlap, one outside the map, one with per-axis half extents applied through three numbers
    centers = np.array([[0.0, 0.0, 0.0], [1.5, 0.5, 0.0], [900.0, 0.0, 0.0], [-3.0, 2.0, 1.0], [c[:, 0].min(), 0.0, 0.0]])
    for half in (3.0, (2.0, 4.0, 1.0)):
        boxes = np.concatenate([centers, np.broadcast_to(np.asarray(half, np.float64), (len(centers), 3))], axis=1)
        for relative in (True, False):
            for mc in (1, 2):
                got = vm.submaps(centers, half, min_count=mc, relative=relative)
                want = ref.select(rec, ORIGIN, VOXEL, mc, 1, boxes, relative)
                assert _np(got["offsets"]).tolist() == want["offsets"].tolist() and int(got["status"]) == 0
                assert _same_points(_np(got["points"]), want["points"]), (half, relative, mc)
        n0, n1 = np.diff(want["offsets"])[:2]
        assert n0 > 5 and n1 > 5 and want["offsets"][3] == want["offsets"][2], "two filled boxes, an empty one"
    # a reserved output: exact fit, then one short
    total = int(want["offsets"][-1])
    fit = vm.submaps(centers, half, min_count=2, relative=False, capacity=total)
    assert _np(fit["offsets"]).tolist() == want["offsets"].tolist() and _same_points(_np(fit["points"]), want["points"])
    short = vm.submaps(centers, half, min_count=2, relative=False, capacity=total - 1)
    assert int(short["status"]) == ref.CAPACITY and _np(short["offsets"]).tolist() == [0] * (len(centers) + 1)


def test_select_many_boxes_of_a_sliced_map(gpu):
    """a map of 4 097 records (three slices per box) and 200 boxes: 600 slice counters, two or three per thread of the scan"""
    rng = np.random.default_rng(4097)
    cells = rng.permutation(70 * 70)[:4097]
    pts = np.stack([cells // 70 - 35, cells % 70 - 35, rng.integers(-2, 2, 4097)], axis=1) * VOXEL + rng.uniform(0.01, 0.24, (4097, 3)) + ORIGIN
    off = _split(4097, 3)
    rec = ref.integrate(pts, off, [0, 1, 2], _shifts(3), ORIGIN, VOXEL)
    assert len(rec["keys"]) == 4097
    vm = gpu.VoxelMap(VOXEL, ORIGIN, capacity=4097).insert(_bank_of(gpu, pts, off), _shifts(3))
    assert ref.same(_map_records(vm), rec) and 4096 < vm.records["keys"].shape[0] <= 6144, "three slices of 2048 records"
    centers = np.concatenate([rng.uniform(-9, 9, (199, 2)), np.zeros((199, 1))], axis=1) + ORIGIN
    centers = np.concatenate([centers, [[500.0, 0.0, 0.0]]])                                  # the last box is empty
    half = (1.5, 2.5, 1.0)
    boxes = np.concatenate([centers, np.broadcast_to(np.asarray(half), (200, 3))], axis=1)
    for relative in (True, False):
        got = vm.submaps(centers, half, relative=relative)
        want = ref.select(rec, ORIGIN, VOXEL, 1, 1, boxes, relative)
        assert int(got["status"]) == 0 and _np(got["offsets"]).tolist() == want["offsets"].tolist()
        assert _same_points(_np(got["points"]), want["points"]), relative
    sizes = np.diff(want["offsets"])
    assert sizes[-1] == 0 and (sizes[:-1] > 0).sum() > 150 and sizes.sum() > 4097, "filled boxes that overlap"


def test_select_faces(gpu):
    """voxel 0.25, origin 0: the only point of its voxel at 1.125 gives the centroid (4 + 0.5) * 0.25 = 1.125 exactly.  A box
    whose lower face is 1.125 keeps it (centre - half <= c), a box whose upper face is 1.125 drops it (c < centre + half)"""
    pts = np.array([[1.125, 1.125, 1.125], [-10.375, 0.625, 0.125]])
    bank = _bank_of(gpu, pts, [0, 2])
    vm = gpu.VoxelMap(0.25, np.zeros(3)).insert(bank, np.eye(4)[None])
    rec = ref.integrate(pts, [0, 2], [0], np.eye(4)[None], np.zeros(3), 0.25)
    assert np.array_equal(ref.centroids(rec, np.zeros(3), 0.25), pts[[1, 0]])
    for a in range(3):
        lower, upper = np.full(3, 1.125), np.full(3, 1.125)
        lower[a], upper[a] = 2.125, 0.125
        centers = np.stack([lower, upper, np.full(3, 1.125)])
        got = vm.submaps(centers, 1.0, relative=False)
        want = ref.select(rec, np.zeros(3), 0.25, boxes=np.concatenate([centers, np.ones((3, 3))], axis=1))
        assert _np(got["offsets"]).tolist() == want["offsets"].tolist() == [0, 1, 1, 2], a
        assert _same_points(_np(got["points"]), want["points"]) and np.array_equal(_np(got["points"]), pts[[0, 0]])


def test_save_and_load(gpu, scene, tmp_path):
    vm, rec = _scene_map(gpu, scene)
    path = str(tmp_path / "map.npz")
    vm.save(path)
    for capacity in (None, len(rec["keys"]) + 100):
        back = gpu.VoxelMap.load(path, capacity=capacity)
        assert back.voxel_size == VOXEL and np.array_equal(back.origin, ORIGIN) and ref.same(_map_records(back), rec)
        assert _same_points(_np(back.points()["points"]), ref.centroids(rec, ORIGIN, VOXEL))


# ------------------------------------------------------------------ determinism and capture
def _capture(lib, _lib, st, fn):
    g = ctypes.c_void_p()
    _lib.check(lib.egonn_graph_begin(st.cuda_stream))
    try:
        fn()
    finally:
        rc = lib.egonn_graph_end(st.cuda_stream, ctypes.byref(g))
    _lib.check(rc)
    return g


def test_eager_and_replayed_graph_are_bit_equal(gpu, scene):
    """reserved capacity, device picks and poses: two inserts into an emptied map, eager and replayed from a captured graph, give
    the same records; between the replays the buffers are overwritten"""
    from egonn_amd import _lib
    lib = _lib.load()
    bank_np, off, poses = scene
    bank = _bank_of(gpu, bank_np, off)
    picks = [np.array([0, 1, 2, 2], np.int32), np.array([6, 5, 4, 3, 0], np.int32)]
    want = ref.integrate(bank_np, off, np.concatenate(picks), poses[np.concatenate(picks)], ORIGIN, VOXEL)
    dev = [(_cu(p), _cu(poses[p]), int(sum(off[i + 1] - off[i] for i in p))) for p in picks]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        vm = gpu.VoxelMap(VOXEL, ORIGIN, capacity=len(want["keys"]) + 50)
        run = lambda: [vm.insert(bank, ps, pk, points_capacity=cap) for pk, ps, cap in dev]          # noqa: E731
        run()                                                                   # eager once: every buffer exists now
        st.synchronize()
        eager = _map_records(vm)
        assert eager["status"] == 0 and ref.same(eager, want)
        vm.clear()
        st.synchronize()
        g = _capture(lib, _lib, st, run)
        for rep in range(2):
            for R in vm._buf:                                                   # both record buffers overwritten, then the map emptied
                for f in ref.FIELDS:
                    R[f].fill_(-3)
                R["n"].fill_(-3)
            vm.clear()
            _lib.check(lib.egonn_graph_launch(g, st.cuda_stream))
            st.synchronize()
            assert ref.same(_map_records(vm), want), rep
    lib.egonn_graph_destroy(g)
    torch.cuda.current_stream().wait_stream(st)


# ------------------------------------------------------------------ the seam to the ICP
def test_scan_to_map_refinement_moves_towards_the_planted_pose(gpu):
    """The six scans of planted_sequence() in a CloudBank.  The map at the planted poses has fewer voxels than the map at the
    perturbed "GPS" poses.  Every scan k, started at gps[k] against the map of the other five scans at their planted poses, ends
    nearer to planted[k] than it started (Frobenius norm of the pose difference).  The condition was confirmed on the CPU for the
    restatements alone (icp_f64 / downsample_f64 of tests/test_icp_host.py against the numpy map): see DESIGN.md §3.19."""
    from tests import tuples_data as D
    raws, planted, gps = D.planted_sequence()
    bank = gpu.CloudBank().add(raws)
    n_planted, n_gps = gpu.build_map(bank, planted).n_voxels, gpu.build_map(bank, gps).n_voxels
    print(f"[voxel map] voxels at 0.2 m: planted {n_planted}, gps {n_gps}")
    assert 0 < n_planted < n_gps
    for k in range(6):
        others = [j for j in range(6) if j != k]
        vm = gpu.VoxelMap(0.2, origin=planted[0, :3, 3]).insert(bank, planted[others], others)
        assert vm.status == 0
        r = gpu.refine_against_map(vm, bank, [k], gps[k: k + 1], half_extent=30.0)
        pose = _np(r["poses"])[0]
        d_init, d_ref = np.linalg.norm(gps[k] - planted[k]), np.linalg.norm(pose - planted[k])
        print(f"[voxel map] scan {k}: |gps - planted| {d_init:.4f}, |refined - planted| {d_ref:.4f}, fitness {float(r['fitness'][0]):.3f}, "
              f"status {int(r['status'][0])}")
        assert d_ref < d_init, k
