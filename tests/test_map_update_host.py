"""CPU tests of the map update (csrc/voxel_map.hip: integrate_moments, merge_moments, subtract; egonn_amd/mapping.py: remove,
repose, the ledger, NDTMap.from_map / update): the restatement tests/map_update_ref.py against a dict of Python ints that is
simply built from the surviving observations; insert-then-remove against a build of the rest; every kind of illegal row; the
moments against tests/ndt_ref.py; repose of the planted sequence from the perturbed to the planted poses; the ledger rules;
the new C entry points declared, exported and refusing bad arguments before any launch; the Python surface refusing them
before it asks for a device.  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import map_update_ref as ref
from tests import ndt_ref as nref
from tests import voxel_map_ref as vref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["egonn_voxel_map_integrate_moments", "egonn_voxel_map_integrate_moments_scratch_bytes", "egonn_voxel_map_merge_moments",
               "egonn_voxel_map_merge_moments_scratch_bytes", "egonn_voxel_map_subtract", "egonn_voxel_map_subtract_scratch_bytes"]
VOXEL = 0.25
ORIGIN = (0.5, -1.25, 0.125)
PICK = np.array([0, 1, 2, 3, 4, 5, 6, 2, 0])                  # an empty cloud (3), two clouds twice


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def scene():
    return vref.random_scene()


@pytest.fixture(scope="module")
def planted():
    """the six scans of planted_sequence() and their two builds at 0.2 m"""
    bank, off, good, gps = vref.planted_bank()
    org = good[0, :3, 3]
    return {"bank": bank, "off": off, "planted": good, "gps": gps, "org": org,
            "at_planted": ref.integrate_moments(bank, off, np.arange(6), good, org, 0.2),
            "at_gps": ref.integrate_moments(bank, off, np.arange(6), gps, org, 0.2)}


# ----------------------------------------------------------------------------- the restatements
def test_integrate_moments_restated(scene):
    """the four arrays are vref.integrate's, the moments nref.accumulate's over the same keys, and both the naive map's"""
    bank, off, poses = scene
    ps = poses[PICK]
    a = ref.integrate_moments(bank, off, PICK, ps, ORIGIN, VOXEL)
    assert vref.same(a, vref.integrate(bank, off, PICK, ps, ORIGIN, VOXEL)) and a["status"] == 0
    acc = nref.accumulate(a["keys"], bank, off, PICK, ps, ORIGIN, VOXEL)
    assert acc["missed"] == 0 and np.array_equal(acc["cnt"], a["count"])
    assert np.array_equal(acc["s1"], a["s1"]) and np.array_equal(acc["s2"], a["s2"]) and a["s1"].dtype == a["s2"].dtype == np.int64
    assert (a["s2"][:, [0, 3, 5]] > 0).any() and a["s1"].max() < a["count"].max() * (1 << 20)
    assert ref.same(a, ref.NaiveMap(VOXEL, ORIGIN).insert(bank, off, PICK, ps).records())
    # a bad pick, a dropped point and the two capacities follow vref.integrate
    b = ref.integrate_moments(bank, off, [0, 9, 1], poses[[0, 1, 1]], ORIGIN, VOXEL)
    assert b["status"] == ref.BAD_INDEX and ref.same(b, ref.integrate_moments(bank, off, [0, 1], poses[[0, 1]], ORIGIN, VOXEL))
    short = ref.integrate_moments(bank, off, PICK, ps, ORIGIN, VOXEL, capacity=len(a["keys"]) - 1)
    assert short["status"] == ref.CAPACITY and len(short["keys"]) == 0 and short["s2"].shape == (0, 6)


def test_merge_moments_restated(scene):
    bank, off, poses = scene
    a = ref.integrate_moments(bank, off, [0, 1, 2], poses[:3], ORIGIN, VOXEL)
    b = ref.integrate_moments(bank, off, [4, 5], poses[4:6], ORIGIN, VOXEL)
    u = ref.merge_moments(a, b)
    assert vref.same(u, vref.merge(a, b)) and ref.same(u, ref.merge_moments(b, a))
    assert ref.same(u, ref.integrate_moments(bank, off, [0, 1, 2, 4, 5], poses[[0, 1, 2, 4, 5]], ORIGIN, VOXEL))
    over = ref.merge_moments(a, b, capacity_out=len(u["keys"]) - 1)
    assert over["status"] == ref.CAPACITY and ref.same(over, a)
    assert ref.same(ref.merge_moments(a, ref.empty()), a) and ref.same(ref.merge_moments(ref.empty(), a), a)


@pytest.mark.parametrize("moments", [True, False])
def test_subtract_against_a_map_built_from_the_survivors(scene, moments):
    bank, off, poses = scene
    ps = poses[PICK]
    whole = ref.integrate(bank, off, PICK, ps, ORIGIN, VOXEL, moments)
    for gone in ([7], [0, 8], [1, 2, 4], list(range(9)), [3]):
        stay = [k for k in range(9) if k not in gone]
        got = ref.subtract(whole, ref.integrate(bank, off, PICK[gone], ps[gone], ORIGIN, VOXEL, moments))
        naive = ref.NaiveMap(VOXEL, ORIGIN).insert(bank, off, PICK[stay], ps[stay]).records(moments)
        assert got["status"] == 0 and ref.same(got, naive), gone
        assert len(got["keys"]) <= len(whole["keys"]) and (got["count"] > 0).all() and (got["obs"] > 0).all()
    assert len(ref.subtract(whole, whole)["keys"]) == 0 and ref.subtract(whole, whole)["status"] == 0
    assert ref.same(ref.subtract(whole, ref.empty(moments)), whole)
    assert len(ref.subtract(whole, ref.integrate(bank, off, PICK[[1, 2, 4]], ps[[1, 2, 4]], ORIGIN, VOXEL, moments))["keys"]) < len(whole["keys"])


@pytest.mark.parametrize("batches", [1, 2, 5])
def test_insert_then_remove_equals_insert_of_the_rest(scene, batches):
    bank, off, poses = scene
    ps = poses[PICK]
    gone = np.array([8, 1, 4, 7, 3])
    stay = np.array([k for k in range(9) if k not in gone])
    want = ref.integrate_moments(bank, off, PICK[stay], ps[stay], ORIGIN, VOXEL)
    for order in (gone, gone[::-1]):
        m = ref.Map(VOXEL, ORIGIN).insert(bank, off, PICK, ps)
        for part in np.array_split(order, batches):
            m.remove(bank, off, PICK[part], ps[part])
        assert m.rec["status"] == 0 and ref.same(m.rec, want), (batches, order[0])
        # identical (pick, pose) entries cannot be told apart: the first one leaves
        assert sorted(m.ledger[0].tolist()) == sorted(PICK[stay].tolist()) and np.array_equal(m.ledger[1], poses[m.ledger[0]])


def test_every_kind_of_illegal_row_leaves_a(scene):
    bank, off, poses = scene
    ps = poses[PICK]
    A = ref.integrate_moments(bank, off, PICK, ps, ORIGIN, VOXEL)
    B = ref.integrate_moments(bank, off, PICK[[1, 5]], ps[[1, 5]], ORIGIN, VOXEL)
    assert ref.subtract(A, B)["status"] == 0
    row = int(np.flatnonzero((A["count"] >= 2) & (A["obs"] >= 2))[3])
    kinds = ref.illegal_rows(A, row)
    assert len(kinds) == 5
    for name, bad in kinds.items():
        for Bx in (bad, ref.with_row(B, bad)):
            got = ref.subtract(A, Bx)
            assert got["status"] == ref.MISMATCH and ref.same(got, A), name
            plain = ref.subtract({f: A[f] for f in ref.FIELDS}, {f: Bx[f] for f in ref.FIELDS})
            assert plain["status"] == ref.MISMATCH and vref.same(plain, A), name
    # a remainder in the moments alone is caught with moments and cannot be seen without
    only_m = ref.one_voxel(A["keys"][row], A["sums"][row], A["count"][row], A["obs"][row], A["s1"][row], A["s2"][row] - 1)
    assert ref.subtract(A, only_m)["status"] == ref.MISMATCH
    assert ref.subtract({f: A[f] for f in ref.FIELDS}, {f: only_m[f] for f in ref.FIELDS})["status"] == 0
    # what subtract does not prove: a subset of a voxel's points under the wrong sums passes
    wrong = ref.one_voxel(A["keys"][row], A["sums"][row] // 3, 1, 1, A["s1"][row] // 3, A["s2"][row] // 3)
    assert ref.subtract(A, wrong)["status"] == 0


# ----------------------------------------------------------------------------- repose
def test_repose_from_the_perturbed_to_the_planted_poses(planted):
    """18 869 voxels at the perturbed poses, 7 881 at the planted ones, and the re-posed map is the second"""
    P = planted
    assert len(P["at_gps"]["keys"]) == 18869 and len(P["at_planted"]["keys"]) == 7881
    m = ref.Map(0.2, P["org"]).insert(P["bank"], P["off"], np.arange(6), P["gps"])
    assert ref.same(m.rec, P["at_gps"])
    assert m.repose(P["bank"], P["off"], P["planted"]) == 6
    assert m.rec["status"] == 0 and ref.same(m.rec, P["at_planted"]) and np.array_equal(m.ledger[1], P["planted"])
    assert m.repose(P["bank"], P["off"], P["planted"]) == 0 and ref.same(m.rec, P["at_planted"])
    plain = ref.Map(0.2, P["org"], moments=False).insert(P["bank"], P["off"], np.arange(6), P["gps"])
    assert plain.repose(P["bank"], P["off"], P["planted"]) == 6
    assert vref.same(plain.rec, P["at_planted"]) and not ref.has_moments(plain.rec)


def repose_tolerances(gps, good):
    """tolerances strictly between the smallest and the largest change of the sequence -> (rot_tol, trans_tol, moved mask)"""
    d = np.abs(good - gps)
    dr, dt = d[:, :3, :3].reshape(6, -1).max(axis=1), d[:, :3, 3].max(axis=1)
    assert dr.min() < dr.max() and dt.min() < dt.max()
    rot_tol, trans_tol = float(np.sort(dr)[2] + np.sort(dr)[3]) / 2, float(np.sort(dt)[2] + np.sort(dt)[3]) / 2
    moved = (dr > rot_tol) | (dt > trans_tol)
    assert 0 < moved.sum() < 6
    return rot_tol, trans_tol, moved


def test_repose_with_tolerances_moves_a_strict_subset(planted):
    P = planted
    rot_tol, trans_tol, moved = repose_tolerances(P["gps"], P["planted"])
    mixed = np.where(moved[:, None, None], P["planted"], P["gps"])
    m = ref.Map(0.2, P["org"]).insert(P["bank"], P["off"], np.arange(6), P["gps"])
    assert m.repose(P["bank"], P["off"], P["planted"], rot_tol, trans_tol) == moved.sum()
    assert ref.same(m.rec, ref.integrate_moments(P["bank"], P["off"], np.arange(6), mixed, P["org"], 0.2))
    assert np.array_equal(m.ledger[1], mixed) and m.ledger[0].tolist() == list(range(6))
    n = len(m.rec["keys"])
    assert 7881 < n < 18869
    # only a rotation over its tolerance, only a translation over its tolerance
    for rt, tt in ((rot_tol, np.inf), (np.inf, trans_tol)):
        k = ref.Map(0.2, P["org"]).insert(P["bank"], P["off"], np.arange(6), P["gps"]).repose(P["bank"], P["off"], P["planted"], rt, tt)
        assert 0 < k <= moved.sum()


def test_the_ledger_rules(scene):
    bank, off, poses = scene
    m = ref.Map(VOXEL, ORIGIN).insert(bank, off, [2, 5, 2], poses[[2, 5, 2]])
    held = ref.copy(m.rec)
    for pk, ps in (([4], poses[[4]]), ([2], poses[[5]]), ([2, 2, 2], poses[[2, 2, 2]]), ([5], poses[[5]] + 1e-16)):
        with pytest.raises(ValueError, match="ledger"):
            m.remove(bank, off, pk, ps)
        assert ref.same(m.rec, held) and m.ledger[0].tolist() == [2, 5, 2], "a refused remove changes nothing"
    m.remove(bank, off, [2], poses[[2]])                                        # inserted twice: removed once, then again
    assert m.ledger[0].tolist() == [5, 2] and ref.same(m.rec, ref.integrate_moments(bank, off, [5, 2], poses[[5, 2]], ORIGIN, VOXEL))
    m.remove(bank, off, [2], poses[[2]])
    assert m.ledger[0].tolist() == [5]
    with pytest.raises(ValueError, match="ledger"):
        m.remove(bank, off, [2], poses[[2]])
    with pytest.raises(ValueError, match="ledger"):
        ref.Map(VOXEL, ORIGIN, track=False).repose(bank, off, poses[:0])
    # without the ledger a wrong pose is caught only when it shows in the counts
    u = ref.Map(VOXEL, ORIGIN, track=False).insert(bank, off, [2, 5], poses[[2, 5]])
    far = poses[[2]].copy()
    far[0, :3, 3] += 40.0
    u.remove(bank, off, [2], far)
    assert u.rec["status"] == ref.MISMATCH and ref.same(u.rec, ref.integrate_moments(bank, off, [2, 5], poses[[2, 5]], ORIGIN, VOXEL))


def test_voxel_map_ledger_matching_is_the_restatements(scene):
    """VoxelMap's own ledger code (host only): matching by bytes, one entry per match, refusal before any device is asked for"""
    import torch
    from egonn_amd import mapping as M
    _, _, poses = scene
    vm = M.VoxelMap(VOXEL, ORIGIN, moments=True, track=True)
    assert vm.ledger[0].shape == (0,) and vm.ledger[1].shape == (0, 4, 4) and vm.ledger[0].dtype == np.int32
    vm._ledger_pick, vm._ledger_pose = [2, 5, 2], [poses[2].copy(), poses[5].copy(), poses[2].copy()]
    assert vm._ledger_match("t", np.array([2, 2, 5]), poses[[2, 2, 5]]) == [0, 2, 1]
    assert vm._ledger_match("t", np.array([5]), poses[[5]]) == [1]
    for pk, ps in (([4], poses[[4]]), ([2], poses[[5]]), ([2, 2, 2], poses[[2, 2, 2]]), ([5], poses[[5]] + 1e-16)):
        with pytest.raises(ValueError, match="not in the ledger"):
            vm.remove(_Bank([5, 0, 7, 3, 3, 3]), ps, pk)
    assert vm.ledger[0].tolist() == [2, 5, 2] and vm._status is None
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="empty"):
            vm.remove(_Bank([5, 0, 7, 3, 3, 3]), poses[[5]], [5])


# ----------------------------------------------------------------------------- the C ABI
def test_symbols_declared_and_exported(lib):
    from egonn_amd import _lib
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert re.search(r"EGONN_VMAP_STATUS_MISMATCH = 8\b", header)
    src = open(os.path.join(REPO, "egonn_amd", "csrc", "voxel_map.hip")).read()
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*(float|double)|unsafeAtomicAdd|atomicAdd_system", src), "integer atomics only"
    from egonn_amd import mapping as M
    assert M.STATUS_MISMATCH == ref.MISMATCH == 8


def _refused(lib, rc, needle):
    assert rc == 1, rc                              # EGONN_STATUS_INVALID: returned before any device work
    assert needle in lib.egonn_last_error().decode(), lib.egonn_last_error()


def _broken(args, at, value):
    out = list(args)
    out[at] = value
    return out


def test_c_entries_refuse_bad_arguments_before_any_launch(lib):
    """one valid-looking argument list per entry point, broken in one place per case; the pointers are never dereferenced (small
    fake addresses) and no GPU is present when this runs"""
    p, s = C.c_void_p(256), C.c_void_p(4096)
    d3 = lambda *v: (C.c_double * 3)(*v)             # noqa: E731
    org, nan, inf = d3(0.0, 0.0, 0.0), float("nan"), float("inf")
    # integrate_moments: bank n_bank off n_clouds pick poses n_obs origin voxel points_capacity keys sums count obs s1 s2 capacity n_out
    # status scratch bytes stream
    need = lib.egonn_voxel_map_integrate_moments_scratch_bytes(1000, 4)
    assert need > 0 and need % 256 == 0 and need == lib.egonn_voxel_map_integrate_scratch_bytes(1000, 4), "no extra per-point storage"
    ok = [p, 1000, p, 4, p, p, 4, org, 0.2, 1000, p, p, p, p, p, p, 1000, p, p, s, need, None]
    f = lib.egonn_voxel_map_integrate_moments
    for at, value, needle in ((6, 0, "n_obs"), (6, 4097, "n_obs"), (1, -1, "bad shape"), (3, -1, "bad shape"), (9, -1, "points_capacity"),
                              (9, 1 << 31, "points_capacity"), (16, -1, "capacity"), (16, 1 << 31, "capacity"), (8, 0.0, "voxel"),
                              (8, nan, "voxel"), (8, inf, "voxel"), (7, d3(0.0, nan, 0.0), "origin"), (7, None, "origin"),
                              (0, None, "null"), (2, None, "null"), (4, None, "null"), (5, None, "null"), (10, None, "null"),
                              (11, None, "null"), (12, None, "null"), (13, None, "null"), (14, None, "all given or all null"),
                              (15, None, "all given or all null"), (17, None, "null"), (18, None, "null"), (19, None, "null"),
                              (19, C.c_void_p(4096 + 8), "256-byte aligned"), (20, need - 1, "scratch needs")):
        _refused(lib, f(*_broken(ok, at, value)), needle)
        assert "voxel_map_integrate_moments" in lib.egonn_last_error().decode()
    assert lib.egonn_voxel_map_integrate_moments_scratch_bytes(-1, 4) == -1 and lib.egonn_voxel_map_integrate_moments_scratch_bytes(10, 0) == -1
    assert lib.egonn_voxel_map_integrate_moments_scratch_bytes(1 << 31, 4) == -1 and lib.egonn_voxel_map_integrate_moments_scratch_bytes(10, 4097) == -1
    assert lib.egonn_voxel_map_integrate_moments_scratch_bytes(0, 1) > 0
    # merge_moments, subtract: A (keys sums count obs s1 s2 n) capacity_a B (...) capacity_b out (keys sums count obs s1 s2) capacity_out
    # n_out status scratch bytes stream
    q, o = C.c_void_p(512), C.c_void_p(768)
    for name in ("merge_moments", "subtract"):
        f, fb = getattr(lib, f"egonn_voxel_map_{name}"), getattr(lib, f"egonn_voxel_map_{name}_scratch_bytes")
        need = fb(100, 50, 150)
        assert need > 0 and need % 256 == 0
        ok = [p, p, p, p, p, p, p, 100, q, q, q, q, q, q, q, 50, o, o, o, o, o, o, 150, p, p, s, need, None]
        for at, value, needle in ((7, -1, "capacity_a"), (15, -1, "capacity_b"), (22, 99, "capacity_out"), (22, 1 << 31, "capacity_out"),
                                  (15, 1 << 31, "capacity_b"), (0, None, "null"), (3, None, "null"), (6, None, "null"), (8, None, "null"),
                                  (14, None, "null"), (16, None, "null"), (19, None, "null"), (23, None, "null"), (24, None, "null"),
                                  (25, None, "null"), (16, p, "must not be A or B"), (16, q, "must not be A or B"),
                                  (4, None, "all given or all null"), (5, None, "all given or all null"),
                                  (12, None, "all given or all null"), (13, None, "all given or all null"),
                                  (20, None, "all given or all null"), (21, None, "all given or all null"),
                                  (25, C.c_void_p(4096 + 128), "256-byte aligned"), (26, need - 1, "scratch needs")):
            _refused(lib, f(*_broken(ok, at, value)), needle)
            assert f"voxel_map_{name}" in lib.egonn_last_error().decode()
        # the moments of one operand given and the others null, and the other way round
        mixed = list(ok)
        for at in (4, 5, 12, 13):
            mixed[at] = None
        _refused(lib, f(*mixed), "all given or all null")
        mixed = list(ok)
        for at in (12, 13, 20, 21):
            mixed[at] = None
        _refused(lib, f(*mixed), "all given or all null")
        assert fb(-1, 5, 5) == -1 and fb(5, -1, 5) == -1 and fb(5, 5, 4) == -1 and fb(1 << 31, 5, 1 << 31) == -1 and fb(0, 0, 0) > 0
    assert lib.egonn_voxel_map_merge_moments_scratch_bytes(100, 50, 150) == lib.egonn_voxel_map_merge_scratch_bytes(100, 50, 150)


# ----------------------------------------------------------------------------- the Python surface
class _Bank:
    """what VoxelMap.insert / remove read of a CloudBank before they ask for a device"""

    def __init__(self, sizes):
        self._sizes = np.asarray(sizes, np.int64)

    def __len__(self):
        return len(self._sizes)

    def sizes(self):
        return self._sizes


def test_python_refuses_bad_arguments_before_asking_for_a_device(lib, monkeypatch):
    import torch
    import egonn_amd
    from egonn_amd import mapping as M
    bank, eye = _Bank([5, 0, 7]), np.tile(np.eye(4), (3, 1, 1))
    vm = M.VoxelMap()
    assert vm.moments is False and vm.track is False and M.VoxelMap(moments=True, track=True).track is True
    # remove mirrors insert's checks
    with pytest.raises(ValueError, match=r"\(3, 4, 4\)"):
        vm.remove(bank, eye[:2])
    with pytest.raises(ValueError, match="pick outside"):
        vm.remove(bank, eye, pick=[0, 1, 3])
    with pytest.raises(ValueError, match="at least one"):
        vm.remove(bank, eye[:0], pick=[])
    with pytest.raises(ValueError, match="empty"):
        vm.remove(bank, eye)
    with pytest.raises(ValueError, match="track=True"):
        vm.repose(bank, eye[:0])
    tr = M.VoxelMap(track=True)
    with pytest.raises(ValueError, match="not in the ledger"):
        tr.remove(bank, eye)
    with pytest.raises(ValueError, match=r"\(0, 4, 4\)"):
        tr.repose(bank, eye)
    with pytest.raises(ValueError, match="at least 0"):
        tr.repose(bank, eye[:0], rot_tol=-1.0)
    with pytest.raises(ValueError, match="at least 0"):
        tr.repose(bank, eye[:0], trans_tol=float("nan"))
    assert tr.repose(bank, eye[:0]) == 0, "an empty ledger has nothing to move"

    class _DevicePick:                       # stands in for a device tensor: the check reads is_cuda before anything else
        is_cuda = True

        def __len__(self):
            return 3

    real_is_tensor = torch.is_tensor
    monkeypatch.setattr(torch, "is_tensor", lambda x: isinstance(x, _DevicePick) or real_is_tensor(x))
    for call in (tr.insert, tr.remove):
        with pytest.raises(ValueError, match="host picks and host poses"):
            call(bank, eye, pick=_DevicePick(), points_capacity=12)
    with pytest.raises(ValueError, match="points_capacity"):
        vm.remove(bank, eye, pick=_DevicePick())
    monkeypatch.undo()
    # the NDT layer from a map
    with pytest.raises(ValueError, match="min_points"):
        M.NDTMap.from_map(vm, min_points=2)
    with pytest.raises(ValueError, match="empty"):
        M.NDTMap.from_map(vm)
    with pytest.raises(ValueError, match="min_eig_ratio"):
        M.build_ndt_map(bank, eye, min_eig_ratio=0.0, moments=True)
    assert vm.n_voxels == 0 and vm.status == 0 and vm.origin is None and tr.ledger[0].size == 0
    assert egonn_amd.VoxelMap is M.VoxelMap
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            M.VoxelMap(moments=True, track=True).insert(bank, eye)


def test_load_refuses_a_map_of_the_other_kind(tmp_path):
    from egonn_amd import VoxelMap
    plain, withm = str(tmp_path / "plain.npz"), str(tmp_path / "moments.npz")
    base = dict(keys=np.zeros(2, np.int64), sums=np.zeros((2, 3), np.int64), count=np.ones(2, np.int32), obs=np.ones(2, np.int32),
                voxel_size=np.float64(0.2), origin=np.zeros(3))
    np.savez(plain, **base)
    np.savez(withm, s1=np.zeros((2, 3), np.int64), s2=np.zeros((2, 6), np.int64), **base)
    with pytest.raises(ValueError, match="with moments does not load into a map without"):
        VoxelMap.load(withm, moments=False)
    with pytest.raises(ValueError, match="without moments does not load into a map with"):
        VoxelMap.load(plain, moments=True)
    with pytest.raises(ValueError, match="without a ledger"):
        VoxelMap.load(plain, track=True)
