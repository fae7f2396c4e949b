"""GPU tests of the map update (run with -m gpu on an MI355X): csrc/voxel_map.hip (integrate_moments, merge_moments, subtract)
and egonn_amd/mapping.py (remove, repose, the ledger, NDTMap.from_map / update, build_ndt_map(moments=True)) against the numpy
restatement tests/map_update_ref.py and against the untouched entry points (integrate, ndt_accumulate, build_ndt_map), bit for
bit: no tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

from tests import map_update_ref as ref
from tests import voxel_map_ref as vref

pytestmark = pytest.mark.gpu

VOXEL = 0.25
ORIGIN = np.array([0.5, -1.25, 0.125])
CANARY = 5                                   # rows behind every output buffer that no call may touch
FILL = 0x5A5A5A5A
WIDTH = {"keys": (), "sums": (3,), "count": (), "obs": (), "s1": (3,), "s2": (6,)}
DTYPE = {"keys": torch.int64, "sums": torch.int64, "count": torch.int32, "obs": torch.int32, "s1": torch.int64, "s2": torch.int64}
PICK = np.array([0, 1, 2, 3, 4, 5, 6, 2, 0])


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


@pytest.fixture(scope="module")
def scene():
    return vref.random_scene()


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


def _names(moments):
    return ref.ALL if moments else ref.FIELDS


def _alloc(rows, moments=True):
    """record buffers of `rows` rows + CANARY rows, every byte a pattern"""
    r = {f: torch.full((rows + CANARY,) + WIDTH[f], FILL, dtype=DTYPE[f], device="cuda") for f in _names(moments)}
    r.update(n=torch.full((), -7, dtype=torch.int64, device="cuda"), rows=rows, moments=moments)
    return r


def _ptrs(r):
    """the six record pointers of the `_moments` entry points and subtract (s1 / s2 null without moments)"""
    return tuple(r[f].data_ptr() if f in r else None for f in ref.ALL)


def _upload(rec, rows=None):
    n, moments = len(rec["keys"]), ref.has_moments(rec)
    r = _alloc(n if rows is None else rows, moments)
    for f in _names(moments):
        r[f][:n] = _cu(rec[f].astype(np.int64) if f == "keys" else rec[f])
    r["n"].fill_(n)
    return r


def _download(r, status=0):
    n = int(r["n"])
    assert 0 <= n <= r["rows"]
    out = {f: _np(r[f][:n]) for f in _names(r["moments"])}
    out["keys"] = out["keys"].astype(np.uint64)
    out["status"] = int(status)
    return out


def _untouched(r, start):
    """rows from `start` on still hold the pattern"""
    return all(bool((r[f][start:] == FILL).all()) for f in _names(r["moments"]))


def _bank_of(gpu, pts, off):
    bank = gpu.CloudBank()
    bank.points = _cu(np.asarray(pts, np.float64).reshape(-1, 3))
    bank.host_offsets = [int(v) for v in off]
    return bank


def _map_records(vm):
    R = vm.records
    n = int(R["n"])
    out = {f: _np(R[f][:n]) for f in _names(vm.moments)}
    out["keys"] = out["keys"].astype(np.uint64)
    out["status"] = vm.status
    return out


# ------------------------------------------------------------------ integrate_moments
def _integrate_moments(pts, off, pick, poses, origin=ORIGIN, voxel=VOXEL, points_capacity=None, capacity=None, against=True):
    """the entry point on exactly full buffers; with `against` also egonn_voxel_map_integrate and egonn_ndt_accumulate on the
    device, whose outputs it must repeat"""
    from egonn_amd import _lib
    lib = _lib.load()
    pts, off = np.asarray(pts, np.float64).reshape(-1, 3), np.asarray(off, np.int64)
    if points_capacity is None:
        points_capacity = int(sum(off[p + 1] - off[p] for p in pick if 0 <= p < len(off) - 1))
    capacity = points_capacity if capacity is None else capacity
    out = _alloc(capacity)
    status = torch.zeros((), dtype=torch.int32, device="cuda")
    bank, offs, pk, ps = _cu(pts), _cu(off), _cu(np.asarray(pick, np.int32)), _cu(np.asarray(poses, np.float64))
    s = _scratch(lib.egonn_voxel_map_integrate_moments_scratch_bytes(points_capacity, len(pick)))
    head = (bank.data_ptr() if len(pts) else None, len(pts), offs.data_ptr(), len(off) - 1, pk.data_ptr(), ps.data_ptr(), len(pick),
            _c3(origin), float(voxel), points_capacity)
    _lib.call(bank.device, lib.egonn_voxel_map_integrate_moments, *head, *_ptrs(out), capacity, out["n"].data_ptr(), status.data_ptr(),
              s.data_ptr(), s.numel() * 8)
    torch.cuda.synchronize()
    got = _download(out, status)
    assert _untouched(out, len(got["keys"]) if got["status"] & ref.CAPACITY else capacity), "rows behind the capacity were written"
    if against:
        plain, st2 = _alloc(capacity, moments=False), torch.zeros((), dtype=torch.int32, device="cuda")
        _lib.call(bank.device, lib.egonn_voxel_map_integrate, *head, *_ptrs(plain)[:4], capacity, plain["n"].data_ptr(), st2.data_ptr(),
                  s.data_ptr(), s.numel() * 8)
        n = int(plain["n"])
        assert n == len(got["keys"]) and int(st2) == got["status"]
        for f in ref.FIELDS:
            assert torch.equal(plain[f][:n], out[f][:n]), f
        rows = max(n, 1)
        cnt, s1, s2 = (torch.zeros((rows,) + w, dtype=d, device="cuda") for w, d in (((), torch.int32), ((3,), torch.int64), ((6,), torch.int64)))
        missed, st3 = torch.zeros((), dtype=torch.int64, device="cuda"), torch.zeros((), dtype=torch.int32, device="cuda")
        s_acc = _scratch(lib.egonn_ndt_accumulate_scratch_bytes(points_capacity, len(pick)))
        _lib.call(bank.device, lib.egonn_ndt_accumulate, *head, out["keys"].data_ptr(), out["n"].data_ptr(), rows, cnt.data_ptr(),
                  s1.data_ptr(), s2.data_ptr(), missed.data_ptr(), st3.data_ptr(), s_acc.data_ptr(), s_acc.numel() * 8)
        torch.cuda.synchronize()
        assert int(missed) == 0 and torch.equal(cnt[:n], out["count"][:n])
        assert torch.equal(s1[:n], out["s1"][:n]) and torch.equal(s2[:n], out["s2"][:n]), "the moments of egonn_ndt_accumulate"
    return got, out


def _check_integrate(pts, off, pick, poses, origin=ORIGIN, voxel=VOXEL):
    got, _ = _integrate_moments(pts, off, pick, poses, origin, voxel)
    want = ref.integrate_moments(pts, off, pick, poses, origin, voxel)
    assert got["status"] == want["status"], (got["status"], want["status"])
    assert ref.same(got, want)
    return want


def _split(n, parts):
    cuts = sorted(np.random.default_rng(n).integers(0, n + 1, size=parts - 1).tolist())
    return np.array([0] + cuts + [n], np.int64)


def _shifts(parts, step=0.0):
    poses = np.tile(np.eye(4), (parts, 1, 1))
    poses[:, 0, 3] = step * np.arange(parts)
    return poses


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_integrate_moments_at_the_wave_and_tile_edges(gpu, n):
    """n points in three clouds: every point in its own voxel, all points in one voxel, and a clustered mix"""
    rng = np.random.default_rng(n)
    off, poses = _split(n, 3), _shifts(3)
    side = max(40, int(np.ceil(np.sqrt(n))))
    cells = rng.permutation(side * side)[:n]
    own = np.stack([cells // side - side // 2, cells % side - side // 2, rng.integers(-3, 3, n)], axis=1) * VOXEL \
        + rng.uniform(0.01, 0.24, (n, 3)) + ORIGIN
    want = _check_integrate(own, off, [0, 1, 2], poses)
    assert len(want["keys"]) == n and (want["count"] == 1).all() and (want["s2"][:, 0] == want["s1"][:, 0] ** 2).all()
    one = ORIGIN + np.array([-3, 2, 5]) * VOXEL + rng.uniform(0.0, VOXEL * 0.999, (n, 3))
    want = _check_integrate(one, off, [0, 1, 2], poses)
    assert len(want["keys"]) == 1 and want["count"][0] == n
    mix = rng.uniform(-2, 2, (12, 3))[rng.integers(0, 12, n)] + rng.normal(0, 0.2, (n, 3))
    want = _check_integrate(mix, off, [2, 0, 1], _shifts(3, 0.07))
    assert want["count"].sum() == n


def test_integrate_moments_runs_across_waves_and_workgroups(gpu):
    """a voxel of 300 points between single-point voxels, at five starts: its run crosses a wave and a 256-point boundary
    wherever it starts, so its moments are added with the 64-bit integer atomics"""
    rng = np.random.default_rng(3)
    inside = lambda m: rng.uniform(0.0, VOXEL * 0.999, (m, 3))                 # noqa: E731
    singles = lambda m, x0: np.stack([np.arange(m) + x0, np.zeros(m), np.zeros(m)], axis=1) * VOXEL + inside(m)   # noqa: E731
    for lead in (0, 10, 63, 200, 255):
        pts = np.concatenate([singles(lead, -400), np.array([1, 0, 0]) * VOXEL + inside(300), singles(17, 50)]) + ORIGIN
        pts = pts[rng.permutation(len(pts))]
        want = _check_integrate(pts, _split(len(pts), 4), [0, 1, 2, 3], _shifts(4))
        assert want["count"].max() == 300 and len(want["keys"]) == lead + 18


def test_integrate_moments_on_faces_signs_and_the_clamp(gpu):
    """coordinates on voxel faces, negative ones, -0.0 and s = -1e-20 (floors to -1, the residual clamps to 2^30 - 1: m = 2^20 - 1)"""
    k = np.arange(-6, 7, dtype=np.float64)
    faces = np.stack(np.meshgrid(k, k[:3], k[-2:], indexing="ij"), axis=-1).reshape(-1, 3) * VOXEL
    odd = np.array([[-0.0, 0.0, -0.0], [-1e-20 * VOXEL, -1e-20 * VOXEL, 1e-20], [-VOXEL, -2 * VOXEL, -1e-300], [1e-310, -1e-310, 0.0]])
    pts = np.concatenate([faces, odd, -faces[:20] - 1e-9, faces[:20] + 1e-9])
    zero = np.zeros(3)
    want = _check_integrate(pts, [0, 40, len(pts)], [0, 1], _shifts(2), origin=zero)
    key, _, _ = vref.point_keys(odd[1:2], np.eye(4), zero, VOXEL)
    row = int(np.searchsorted(want["keys"], key[0]))
    assert want["keys"][row] == key[0] and want["count"][row] == 1 and want["s1"][row, :2].tolist() == [(1 << 20) - 1] * 2
    assert want["s2"][row, 0] == ((1 << 20) - 1) ** 2
    bad = np.concatenate([pts[:30], [[np.nan, 0, 0], [0, np.inf, 0]], pts[30:60]])
    assert _check_integrate(bad, [0, 20, len(bad)], [0, 1], _shifts(2), origin=zero)["status"] == ref.RANGE


def test_integrate_moments_capacity_one_short(gpu, scene):
    bank, off, poses = scene
    want = ref.integrate_moments(bank, off, np.arange(7), poses, ORIGIN, VOXEL)
    n, total = len(want["keys"]), int(off[-1])
    got, buf = _integrate_moments(bank, off, np.arange(7), poses, capacity=n)
    assert got["status"] == 0 and ref.same(got, want) and _untouched(buf, n)
    got, buf = _integrate_moments(bank, off, np.arange(7), poses, capacity=n - 1, against=False)          # one voxel too many
    assert got["status"] == ref.CAPACITY and int(buf["n"]) == 0 and _untouched(buf, 0), "nothing is written, the moments included"
    got, buf = _integrate_moments(bank, off, np.arange(7), poses, points_capacity=total - 1, capacity=total, against=False)
    assert got["status"] == ref.CAPACITY and int(buf["n"]) == 0 and _untouched(buf, 0)


# ------------------------------------------------------------------ merge_moments, subtract
def _random_records(rng, keys, moments=True, low=1):
    keys = np.sort(np.asarray(keys, np.uint64))
    n = len(keys)
    count = rng.integers(low, 5000, n).astype(np.int32)
    out = {"keys": keys, "sums": rng.integers(0, vref.ONE, (n, 3)) * count[:, None].astype(np.int64), "count": count,
           "obs": rng.integers(low, 40, n).astype(np.int32), "status": 0}
    if moments:
        out.update(s1=rng.integers(0, 1 << 20, (n, 3)) * count[:, None].astype(np.int64),
                   s2=rng.integers(0, 1 << 40, (n, 6)) * count[:, None].astype(np.int64))
    return out


def _binary(name, A, B, capacity_out=None, rows_a=None, rows_b=None):
    """egonn_voxel_map_merge_moments / egonn_voxel_map_subtract on uploaded records -> (records, the out buffers)"""
    from egonn_amd import _lib
    lib = _lib.load()
    a, b = _upload(A, rows_a), _upload(B, rows_b)
    if capacity_out is None:
        capacity_out = a["rows"] + (b["rows"] if name == "merge_moments" else 0)
    out = _alloc(capacity_out, a["moments"])
    status = torch.zeros((), dtype=torch.int32, device="cuda")
    s = _scratch(getattr(lib, f"egonn_voxel_map_{name}_scratch_bytes")(a["rows"], b["rows"], capacity_out))
    _lib.call(out["keys"].device, getattr(lib, f"egonn_voxel_map_{name}"), *_ptrs(a), a["n"].data_ptr(), a["rows"], *_ptrs(b),
              b["n"].data_ptr(), b["rows"], *_ptrs(out), capacity_out, out["n"].data_ptr(), status.data_ptr(), s.data_ptr(), s.numel() * 8)
    torch.cuda.synchronize()
    assert _untouched(a, len(A["keys"])) and _untouched(b, len(B["keys"]))
    assert ref.same(_download(a), A) and ref.same(_download(b), B), "the inputs are read only"
    got = _download(out, status)
    assert _untouched(out, len(got["keys"])), "rows from n_out on were written"
    return got, out


@pytest.mark.parametrize("n", [1, 64, 65, 256, 257])
def test_merge_moments_key_sets(gpu, n):
    rng = np.random.default_rng(n)
    pool = np.unique(rng.integers(0, 2 ** 63 - 1, 4 * n + 8, dtype=np.int64).astype(np.uint64))
    pool = pool[rng.permutation(len(pool))]
    A = _random_records(rng, pool[:n])
    cases = {"disjoint": _random_records(rng, pool[n: 2 * n]), "identical": _random_records(rng, pool[:n]),
             "interleaved": _random_records(rng, np.concatenate([pool[: n // 2 + 1], pool[2 * n: 3 * n]])), "empty": ref.empty()}
    for name, B in cases.items():
        for X, Y in ((A, B), (B, A)):
            got, _ = _binary("merge_moments", X, Y)
            want = ref.merge_moments(X, Y)
            assert got["status"] == 0 and ref.same(got, want), name
            got, _ = _binary("merge_moments", X, Y, capacity_out=len(want["keys"]), rows_a=len(X["keys"]), rows_b=len(Y["keys"]) + 3)
            assert got["status"] == 0 and ref.same(got, want), name                        # exactly full
    # without moments the call is egonn_voxel_map_merge
    plain = lambda R: {f: R[f] for f in ref.FIELDS + ("status",)}             # noqa: E731
    got, _ = _binary("merge_moments", plain(A), plain(cases["interleaved"]))
    assert got["status"] == 0 and ref.same(got, vref.merge(A, cases["interleaved"]))


def test_merge_moments_overflow_keeps_a_with_its_moments(gpu):
    rng = np.random.default_rng(2)
    pool = np.unique(rng.integers(0, 2 ** 63 - 1, 1000, dtype=np.int64).astype(np.uint64))
    A, B = _random_records(rng, pool[:300]), _random_records(rng, pool[250:520])
    union = len(np.union1d(A["keys"], B["keys"]))
    got, out = _binary("merge_moments", A, B, capacity_out=union - 1)
    assert got["status"] == ref.CAPACITY and ref.same(got, A) and _untouched(out, len(A["keys"]))
    got, _ = _binary("merge_moments", A, B, capacity_out=union)
    assert got["status"] == 0 and ref.same(got, ref.merge_moments(A, B))


def _rows_of(R, rows):
    out = {f: R[f][rows] for f in ref.fields(R)}
    out["status"] = 0
    return out


def _part_of(R, rows, rng):
    """legal B rows that leave a remainder: one point of one observation with a part of the sums"""
    out = _rows_of(R, rows)
    out["count"], out["obs"] = np.ones(len(rows), np.int32), np.ones(len(rows), np.int32)
    for f in ("sums", "s1", "s2"):
        if f in out:
            out[f] = out[f] // rng.integers(2, 9, out[f].shape)
    return out


@pytest.mark.parametrize("moments", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_subtract_drops_at_the_wave_and_tile_edges(gpu, n, moments):
    """A of n rows (every count and obs >= 2).  B takes whole rows out (none, the first, the last, every row, every other row, rows
    62-66, rows 254-258) and a part of every third remaining row, which stays with its remainder"""
    rng = np.random.default_rng(n)
    keys = np.unique(rng.integers(0, 2 ** 63 - 1, n + 8, dtype=np.int64).astype(np.uint64))[:n]
    A = _random_records(rng, keys, moments, low=2)
    every = np.arange(n)
    drops = {"none": every[:0], "first": every[:1], "last": every[-1:], "every": every, "every other": every[::2],
             "62-66": every[62:67], "254-258": every[254:259]}
    for name, gone in drops.items():
        part = np.setdiff1d(every, gone)[::3]
        rows = np.sort(np.concatenate([gone, part]))
        B = _rows_of(A, rows)
        P = _part_of(A, part, rng)
        at = np.searchsorted(rows, part)
        for f in ref.fields(A):
            B[f][at] = P[f]
        want = ref.subtract(A, B)
        assert want["status"] == 0 and len(want["keys"]) == n - len(gone)
        got, out = _binary("subtract", A, B, rows_b=len(rows) + 2)
        assert got["status"] == 0 and ref.same(got, want), name
        got, _ = _binary("subtract", A, B, capacity_out=n + 7, rows_a=n)
        assert got["status"] == 0 and ref.same(got, want), name
    got, _ = _binary("subtract", A, ref.empty(moments))
    assert got["status"] == 0 and ref.same(got, A), "B empty: out = A"
    got, _ = _binary("subtract", ref.empty(moments), ref.empty(moments))
    assert got["status"] == 0 and len(got["keys"]) == 0


@pytest.mark.parametrize("moments", [True, False])
def test_subtract_illegal_rows_leave_a(gpu, moments):
    """each of the five kinds in one row of an otherwise legal B: out == A bit for bit, n_out = n_a, MISMATCH and no other bit,
    canary rows from n_a on untouched; the row sits in the first and in the third workgroup"""
    rng = np.random.default_rng(77)
    n = 600
    keys = np.unique(rng.integers(0, 2 ** 63 - 1, n + 8, dtype=np.int64).astype(np.uint64))[:n]
    A = _random_records(rng, keys, True, low=2)
    legal = np.arange(n)[5::7]
    B = _rows_of(A, legal)
    P = _part_of(A, legal[::2], rng)
    for f in ref.ALL:
        B[f][::2] = P[f]
    strip = (lambda R: {f: R[f] for f in ref.FIELDS + ("status",)}) if not moments else (lambda R: R)       # noqa: E731
    assert ref.subtract(strip(A), strip(B))["status"] == 0
    for row in (17, 599, 530):
        for name, bad in ref.illegal_rows(A, row).items():
            for Bx in (ref.with_row(B, bad), bad):
                got, out = _binary("subtract", strip(A), strip(Bx), capacity_out=n + 3)
                assert got["status"] == ref.MISMATCH, (name, row)
                assert ref.same(got, strip(A)) and int(out["n"]) == n and _untouched(out, n), (name, row)
    if moments:                                   # a remainder in the moments alone
        bad = _rows_of(A, np.array([300]))
        bad["s2"] = bad["s2"] - 1
        got, _ = _binary("subtract", A, bad)
        assert got["status"] == ref.MISMATCH and ref.same(got, A)


# ------------------------------------------------------------------ Python: remove, repose, files, capture
@pytest.mark.parametrize("reserved", [False, True])
@pytest.mark.parametrize("moments", [True, False])
def test_insert_then_remove_equals_a_build_of_the_rest(gpu, scene, reserved, moments):
    bank_np, off, poses = scene
    bank = _bank_of(gpu, bank_np, off)
    ps = poses[PICK]
    gone = np.array([8, 1, 4, 7, 3])
    stay = np.array([k for k in range(9) if k not in gone])
    whole = ref.integrate(bank_np, off, PICK, ps, ORIGIN, VOXEL, moments)
    want = ref.integrate(bank_np, off, PICK[stay], ps[stay], ORIGIN, VOXEL, moments)
    kw = dict(voxel_size=VOXEL, origin=ORIGIN, capacity=len(whole["keys"]) + 9 if reserved else None, moments=moments, track=moments)
    for batches in (1, 2, 5):
        for order in (gone, gone[::-1]):
            vm = gpu.VoxelMap(**kw).insert(bank, ps, PICK)
            assert ref.same(_map_records(vm), whole)
            for part in np.array_split(order, batches):
                vm.remove(bank, ps[part], PICK[part])
            got = _map_records(vm)
            assert got["status"] == 0 and ref.same(got, want) and vm.n_voxels == len(want["keys"]), (batches, order[0])
            if moments:
                assert sorted(vm.ledger[0].tolist()) == sorted(PICK[stay].tolist()) and np.array_equal(vm.ledger[1], poses[vm.ledger[0]])
    vm = gpu.VoxelMap(chunk_points=400, **kw).insert(bank, ps, PICK).remove(bank, ps[gone], PICK[gone])      # chunks forced by a point budget
    assert ref.same(_map_records(vm), want)
    vm.remove(bank, ps[stay], PICK[stay])
    assert vm.n_voxels == 0 and vm.status == 0
    # what the map does not hold: MISMATCH, the map as it was
    vm = gpu.VoxelMap(**dict(kw, track=False)).insert(bank, ps[stay], PICK[stay])
    far = ps[gone[:1]].copy()
    far[0, :3, 3] += 40.0
    vm.remove(bank, far, PICK[gone[:1]])
    assert vm.status == ref.MISMATCH and ref.same(_map_records(vm), dict(want, status=ref.MISMATCH))


def test_a_cloud_inserted_twice_and_removed_once(gpu, scene):
    bank_np, off, poses = scene
    bank = _bank_of(gpu, bank_np, off)
    vm = gpu.VoxelMap(VOXEL, ORIGIN, moments=True, track=True).insert(bank, poses[[2, 5, 2]], [2, 5, 2])
    held = _map_records(vm)
    for pk, ps in (([4], poses[[4]]), ([2], poses[[5]]), ([2, 2, 2], poses[[2, 2, 2]]), ([5], poses[[5]] + 1e-16)):
        with pytest.raises(ValueError, match="not in the ledger"):
            vm.remove(bank, ps, pk)
    assert ref.same(_map_records(vm), held) and vm.ledger[0].tolist() == [2, 5, 2], "a refused remove launches nothing"
    vm.remove(bank, poses[[2]], [2])
    assert vm.ledger[0].tolist() == [5, 2]
    assert ref.same(_map_records(vm), ref.integrate_moments(bank_np, off, [5, 2], poses[[5, 2]], ORIGIN, VOXEL))
    vm.remove(bank, poses[[2]], [2])
    assert vm.ledger[0].tolist() == [5] and ref.same(_map_records(vm), ref.integrate_moments(bank_np, off, [5], poses[[5]], ORIGIN, VOXEL))
    with pytest.raises(ValueError, match="not in the ledger"):
        vm.remove(bank, poses[[2]], [2])
    with pytest.raises(ValueError, match="host picks and host poses"):
        vm.insert(bank, _cu(poses[[2]]), _cu(np.array([2], np.int32)), points_capacity=1000)


def test_the_ledger_of_a_reserved_map_holds_only_what_the_map_took(gpu, scene):
    """a chunk that a reserved map drops for STATUS_CAPACITY does not enter the ledger, in `insert` and in the re-insert of
    `repose`; the status bits of earlier calls survive the per-chunk read"""
    bank_np, off, poses = scene
    bank = _bank_of(gpu, bank_np, off)
    first = ref.integrate_moments(bank_np, off, [0, 1], poses[[0, 1]], ORIGIN, VOXEL)
    vm = gpu.VoxelMap(VOXEL, ORIGIN, capacity=len(first["keys"]) + 3, moments=True, track=True, chunk_points=300)
    vm.insert(bank, poses[[0, 1]], [0, 1])                                     # one chunk: it fits
    assert vm.status == 0 and vm.ledger[0].tolist() == [0, 1]
    vm.insert(bank, poses[[2, 4]], [2, 4])                                     # two chunks (a point budget of 300), neither fits
    assert vm.status == ref.CAPACITY and vm.ledger[0].tolist() == [0, 1] and ref.same(_map_records(vm), first)
    vm.remove(bank, poses[[1]], [1])
    only = ref.integrate_moments(bank_np, off, [0], poses[[0]], ORIGIN, VOXEL)
    assert vm.status == ref.CAPACITY and vm.ledger[0].tolist() == [0] and ref.same(_map_records(vm), only)
    # repose: the remove goes through, the re-insert at a pose far away does not fit any more
    tight = gpu.VoxelMap(VOXEL, ORIGIN, capacity=len(first["keys"]), moments=True, track=True).insert(bank, poses[[0, 1]], [0, 1])
    far = poses[[0, 1]].copy()
    far[1, :3, 3] += 40.0
    assert tight.repose(bank, far) == 1
    assert tight.status == ref.CAPACITY and tight.ledger[0].tolist() == [0] and ref.same(_map_records(tight), only)
    assert np.array_equal(tight.ledger[1], poses[[0]])


@pytest.fixture(scope="module")
def planted(gpu):
    bank, off, good, gps = vref.planted_bank()
    return {"bank": _bank_of(gpu, bank, off), "np": bank, "off": off, "planted": good, "gps": gps, "org": good[0, :3, 3],
            "at_planted": ref.integrate_moments(bank, off, np.arange(6), good, good[0, :3, 3], 0.2)}


def test_repose_from_the_perturbed_to_the_planted_poses(gpu, planted):
    P = planted
    vm = gpu.VoxelMap(0.2, P["org"], moments=True, track=True).insert(P["bank"], P["gps"])
    assert vm.n_voxels == 18869
    assert vm.repose(P["bank"], P["planted"]) == 6
    got = _map_records(vm)
    assert got["status"] == 0 and vm.n_voxels == 7881 and ref.same(got, P["at_planted"])
    assert np.array_equal(vm.ledger[1], P["planted"]) and vm.ledger[0].tolist() == list(range(6))
    assert vm.repose(P["bank"], P["planted"]) == 0 and ref.same(_map_records(vm), P["at_planted"])
    built = gpu.build_map(P["bank"], P["planted"], 0.2, origin=P["org"])             # the remedy without repose, untouched
    for f in ref.FIELDS:
        assert torch.equal(built.records[f][:7881], vm.records[f][:7881]), f
    plain = gpu.VoxelMap(0.2, P["org"], track=True).insert(P["bank"], P["gps"])
    assert plain.repose(P["bank"], P["planted"]) == 6 and vref.same(_map_records(plain), P["at_planted"])
    with pytest.raises(ValueError, match="track=True"):
        built.repose(P["bank"], P["planted"])


def test_repose_with_tolerances_moves_a_strict_subset(gpu, planted):
    P = planted
    d = np.abs(P["planted"] - P["gps"])
    dr, dt = d[:, :3, :3].reshape(6, -1).max(axis=1), d[:, :3, 3].max(axis=1)
    rot_tol, trans_tol = float(np.sort(dr)[2] + np.sort(dr)[3]) / 2, float(np.sort(dt)[2] + np.sort(dt)[3]) / 2
    moved = (dr > rot_tol) | (dt > trans_tol)
    assert 0 < moved.sum() < 6
    mixed = np.where(moved[:, None, None], P["planted"], P["gps"])
    vm = gpu.VoxelMap(0.2, P["org"], moments=True, track=True, capacity=20000).insert(P["bank"], P["gps"])
    assert vm.repose(P["bank"], P["planted"], rot_tol, trans_tol) == moved.sum()
    want = ref.integrate_moments(P["np"], P["off"], np.arange(6), mixed, P["org"], 0.2)
    assert vm.status == 0 and ref.same(_map_records(vm), want) and np.array_equal(vm.ledger[1], mixed)


def test_save_and_load_with_moments_and_ledger(gpu, scene, tmp_path):
    bank_np, off, poses = scene
    bank = _bank_of(gpu, bank_np, off)
    pick = np.array([0, 1, 2, 4, 5, 6, 2])
    vm = gpu.VoxelMap(VOXEL, ORIGIN, moments=True, track=True).insert(bank, poses[pick], pick)
    rec = ref.integrate_moments(bank_np, off, pick, poses[pick], ORIGIN, VOXEL)
    path, old = str(tmp_path / "map.npz"), str(tmp_path / "old.npz")
    vm.save(path)
    for capacity in (None, len(rec["keys"]) + 100):
        back = gpu.VoxelMap.load(path, capacity=capacity)
        assert back.moments and back.track and ref.same(_map_records(back), rec)
        assert back.ledger[0].tolist() == pick.tolist() and np.array_equal(back.ledger[1], poses[pick])
        back.remove(bank, poses[pick[:3]], pick[:3])                          # the loaded ledger is good for a remove
        assert ref.same(_map_records(back), ref.integrate_moments(bank_np, off, pick[3:], poses[pick[3:]], ORIGIN, VOXEL))
    assert gpu.VoxelMap.load(path, track=False).ledger[0].size == 0
    with pytest.raises(ValueError, match="with moments does not load into a map without"):
        gpu.VoxelMap.load(path, moments=False)
    # a file without them, as the maps before this one wrote it
    gpu.VoxelMap(VOXEL, ORIGIN).insert(bank, poses[pick], pick).save(old)
    with np.load(old) as z:
        assert sorted(z.files) == sorted(ref.FIELDS + ("voxel_size", "origin", "status"))
    back = gpu.VoxelMap.load(old)
    assert not back.moments and not back.track and vref.same(_map_records(back), rec) and "s1" not in back.records
    with pytest.raises(ValueError, match="without moments does not load into a map with"):
        gpu.VoxelMap.load(old, moments=True)


def _capture(lib, _lib, st, fn):
    g = ctypes.c_void_p()
    _lib.check(lib.egonn_graph_begin(st.cuda_stream))
    try:
        fn()
    finally:
        rc = lib.egonn_graph_end(st.cuda_stream, ctypes.byref(g))
    _lib.check(rc)
    return g


def test_captured_remove_equals_eager(gpu, scene):
    """reserved capacity, device picks and poses: two removes, eager and replayed twice from a captured graph into a restored
    map, give the same records; between the replays both record buffers are overwritten"""
    from egonn_amd import _lib
    lib = _lib.load()
    bank_np, off, poses = scene
    bank = _bank_of(gpu, bank_np, off)
    ps = poses[PICK]
    gone = [np.array([7, 1]), np.array([4, 8, 3])]
    stay = np.array([0, 2, 5, 6])
    whole = ref.integrate_moments(bank_np, off, PICK, ps, ORIGIN, VOXEL)
    want = ref.integrate_moments(bank_np, off, PICK[stay], ps[stay], ORIGIN, VOXEL)
    dev = [(_cu(PICK[g].astype(np.int32)), _cu(ps[g]), int(sum(off[i + 1] - off[i] for i in PICK[g]))) for g in gone]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        vm = gpu.VoxelMap(VOXEL, ORIGIN, capacity=len(whole["keys"]) + 50, moments=True).insert(bank, ps, PICK)
        st.synchronize()
        start = vm._cur
        saved = {f: vm._buf[start][f].clone() for f in ref.ALL + ("n",)}

        def restore():
            for R in vm._buf:
                for f in ref.ALL + ("n",):
                    R[f].fill_(-3)
            for f in ref.ALL + ("n",):
                vm._buf[start][f].copy_(saved[f])

        run = lambda: [vm.remove(bank, p, k, points_capacity=cap) for k, p, cap in dev]          # noqa: E731
        run()                                                                   # eager once: every buffer exists now
        st.synchronize()
        eager = _map_records(vm)
        assert eager["status"] == 0 and ref.same(eager, want) and vm._cur == start, "two chunks: back in the first buffer"
        restore()
        st.synchronize()
        g = _capture(lib, _lib, st, run)
        for rep in range(2):
            restore()
            _lib.check(lib.egonn_graph_launch(g, st.cuda_stream))
            st.synchronize()
            assert ref.same(_map_records(vm), want), rep
    lib.egonn_graph_destroy(g)
    torch.cuda.current_stream().wait_stream(st)


# ------------------------------------------------------------------ the NDT seam
GAUSS = ("mean", "info", "eigenvalues", "normal", "valid", "n_valid")
REGISTER = ("poses", "fitness", "score", "iterations", "status")


def _same_layer(a, b, n):
    for f in ("keys", "cnt", "s1", "s2"):
        assert torch.equal(getattr(a, f)[:n], getattr(b, f)[:n]), f
    for f in GAUSS:
        x, y = a.gaussians[f], b.gaussians[f]
        assert torch.equal(x if x.dim() == 0 else x[:n], y if y.dim() == 0 else y[:n]), f
        assert np.array_equal(_bits(_np(x if x.dim() == 0 else x[:n])), _bits(_np(y if y.dim() == 0 else y[:n]))), f


def _same_register(a, b, src, poses):
    for nb in (1, 7):
        ra, rb = (m.register(src["points"], src["offsets"], poses, neighbors=nb) for m in (a, b))
        for f in REGISTER:
            assert torch.equal(ra[f], rb[f]) and np.array_equal(_bits(_np(ra[f])), _bits(_np(rb[f]))), (f, nb)
        assert int((rb["iterations"] > 0).sum()) > 0, "the registration moved"


def test_ndt_layer_follows_a_map_that_grows_and_shrinks(gpu):
    """A moments map grown in three inserts (one scan once too often, at its perturbed pose), shrunk by one remove and followed
    with NDTMap.update is the layer build_ndt_map (two passes over the points, untouched) builds over the final set: keys,
    moments, Gaussians and register outputs, bit for bit; so is build_ndt_map(moments=True), and a layer over a reserved map"""
    from tests import tuples_data as D
    raws, pl, gps = D.planted_sequence()
    bank = gpu.CloudBank().add(raws)
    two_pass = gpu.build_ndt_map(bank, pl)
    n = two_pass.n_voxels
    assert n > 150 and two_pass.missed == 0 and not hasattr(two_pass, "vmap")
    src = bank.gather([0, 3, 5])
    for capacity in (None, n + 500):
        vm = gpu.VoxelMap(1.0, origin=pl[0, :3, 3], capacity=capacity, moments=True, track=True)
        vm.insert(bank, pl[:2], [0, 1])
        ndt = gpu.NDTMap.from_map(vm)
        assert ndt.missed == 0 and ndt.gaussians is None
        ndt.finalize()
        vm.insert(bank, np.stack([pl[2], gps[4], pl[3]]), [2, 4, 3]).insert(bank, pl[4:], [4, 5])
        grown = vm.n_voxels
        vm.remove(bank, gps[4:5], [4])
        assert vm.status == 0 and vm.n_voxels == n <= grown
        assert ndt.update(vm) is ndt and ndt.gaussians is None
        with pytest.raises(ValueError, match="finalize"):
            ndt.register(src["points"], src["offsets"], gps[[0, 3, 5]])
        ndt.finalize()
        assert ndt.n_voxels == n and ndt.missed == 0 and ndt.status == 0
        _same_layer(ndt, two_pass, n)
        _same_register(ndt, two_pass, src, gps[[0, 3, 5]])
        if capacity is not None:
            assert ndt.keys.shape[0] == capacity and not bool(ndt._layer["valid"][n:].any()), "rows behind the live count stay invalid"
    one_pass = gpu.build_ndt_map(bank, pl, moments=True)
    assert one_pass.vmap.moments and one_pass.vmap.n_voxels == n and one_pass.n_voxels == n
    _same_layer(one_pass, two_pass, n)
    _same_register(one_pass, two_pass, src, gps[[0, 3, 5]])
    with pytest.raises(ValueError, match="carries no moments"):
        gpu.NDTMap.from_map(gpu.build_map(bank, pl, 1.0))
