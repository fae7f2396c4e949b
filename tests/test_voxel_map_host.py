"""CPU tests of the voxel map (egonn_amd/mapping.py, csrc/voxel_map.hip): the two restatements of tests/voxel_map_ref.py agree
bit for bit, the properties the GPU tests rely on hold for them (batching, order, the residual clamp, centroids inside their
voxel, a consistent trajectory fills fewer voxels), the three C entries and their scratch functions are declared, exported and
refuse bad arguments before any launch, and the Python surface refuses them before it asks for a device.  Nothing here needs
a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import voxel_map_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["egonn_voxel_map_integrate", "egonn_voxel_map_integrate_scratch_bytes", "egonn_voxel_map_merge",
               "egonn_voxel_map_merge_scratch_bytes", "egonn_voxel_map_select", "egonn_voxel_map_select_scratch_bytes"]
VOXEL = 0.25
ORIGIN = (0.5, -1.25, 0.125)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def scene():
    return ref.random_scene()


# ----------------------------------------------------------------------------- the two restatements
def test_the_two_restatements_agree(scene):
    bank, off, poses = scene
    pick = [0, 1, 2, 3, 4, 5, 6, 2]                           # an empty cloud (3) and a cloud picked twice (2)
    ps = poses[pick]
    a = ref.integrate(bank, off, pick, ps, ORIGIN, VOXEL)
    naive = ref.NaiveMap(VOXEL, ORIGIN).insert(bank, off, pick, ps)
    b = naive.records()
    assert ref.same(a, b) and a["status"] == b["status"] == 0
    assert len(a["keys"]) > 100 and (np.diff(a["keys"].astype(np.int64)) > 0).all() and not (a["keys"] >> np.uint64(63)).any()
    assert a["count"].sum() == sum(off[p + 1] - off[p] for p in pick) and a["obs"].max() >= 3 and (a["obs"] <= a["count"]).all()
    assert (a["count"] > 1).sum() > 20, "the scene must fuse points"
    assert np.array_equal(ref.centroids(a, ORIGIN, VOXEL).view(np.uint64), naive.centroids().view(np.uint64))
    # a bad pick contributes nothing and is reported by both
    c = ref.integrate(bank, off, [0, 9, 1], poses[[0, 1, 1]], ORIGIN, VOXEL)
    d = ref.NaiveMap(VOXEL, ORIGIN).insert(bank, off, [0, 9, 1], poses[[0, 1, 1]]).records()
    assert ref.same(c, d) and c["status"] == d["status"] == ref.BAD_INDEX
    assert ref.same(c, ref.integrate(bank, off, [0, 1], poses[[0, 1]], ORIGIN, VOXEL))


@pytest.mark.parametrize("batches", [1, 2, 5])
def test_incremental_equals_one_shot(scene, batches):
    bank, off, poses = scene
    pick = np.array([0, 1, 2, 3, 4, 5, 6, 2, 0])
    ps = poses[pick]
    one = ref.integrate(bank, off, pick, ps, ORIGIN, VOXEL)
    for order in (np.arange(len(pick)), np.arange(len(pick))[::-1]):
        rec, naive = ref.empty(), ref.NaiveMap(VOXEL, ORIGIN)
        for part in np.array_split(order, batches):
            rec = ref.insert(rec, bank, off, pick[part], ps[part], ORIGIN, VOXEL)
            naive.insert(bank, off, pick[part], ps[part])
        assert ref.same(rec, one) and ref.same(naive.records(), one)


def test_residual_clamp_and_voxel_faces():
    """s = -1e-20 floors to -1 and s - (-1) rounds to exactly 1.0: without the clamp q would be 2^30, one past the voxel"""
    pts = np.array([[-1e-20 * VOXEL, 0.0, -0.0], [3 * VOXEL, -2 * VOXEL, VOXEL], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]])
    off = np.array([0, len(pts)])
    eye = np.eye(4)[None]
    assert (-1e-20 * VOXEL) / VOXEL == -1e-20
    key, q, valid = ref.point_keys(pts, eye[0], (0, 0, 0), VOXEL)
    assert valid.tolist() == [True, True, False, False]
    assert ref.indices(key[:2]).tolist() == [[-1, 0, 0], [3, -2, 1]] and q[:2].tolist() == [[ref.ONE - 1, 0, 0], [0, 0, 0]]
    a = ref.integrate(pts, off, [0], eye, (0, 0, 0), VOXEL)
    b = ref.NaiveMap(VOXEL, (0, 0, 0)).insert(pts, off, [0], eye).records()
    assert ref.same(a, b) and a["status"] == b["status"] == ref.RANGE and a["count"].tolist() == [1, 1]
    c = ref.centroids(a, (0, 0, 0), VOXEL)
    assert -VOXEL <= c[0, 0] < 0.0, "the clamped point stays inside voxel -1"
    # the index range: 2^20 - 1 and -2^20 are kept, 2^20 and -2^20 - 1 are dropped
    edge = np.array([[(2 ** 20 - 1) * 1.0, 0, 0], [2 ** 20 * 1.0, 0, 0], [-(2 ** 20) * 1.0, 0, 0], [-(2 ** 20) - 1.0, 0, 0]])
    key, q, valid = ref.point_keys(edge, eye[0], (0, 0, 0), 1.0)
    assert valid.tolist() == [True, False, True, False] and ref.indices(key[[0, 2]])[:, 0].tolist() == [2 ** 20 - 1, -(2 ** 20)]


def test_centroids_lie_inside_their_voxel(scene):
    bank, off, poses = scene
    org = np.array([3e5, 4e6, 50.0])
    far = poses.copy()
    far[:, :3, 3] += org
    rec = ref.integrate(bank, off, np.arange(7), far, org, VOXEL)
    near = ref.integrate(bank, off, np.arange(7), poses, (0, 0, 0), VOXEL)
    c, i = ref.centroids(near, (0, 0, 0), VOXEL), ref.indices(near["keys"])
    assert (c >= i * VOXEL).all() and (c < (i + 1) * VOXEL).all()
    # t' = t - origin first: at UTM-sized translations the voxel indices are those of the local frame up to the rounding of
    # the poses' translations themselves
    assert len(rec["keys"]) == pytest.approx(len(near["keys"]), rel=0.05)
    frac = rec["sums"] / (rec["count"][:, None] * float(ref.ONE))
    assert (frac >= 0).all() and (frac < 1).all()


def test_consistent_poses_fill_fewer_voxels():
    """the six scans of planted_sequence(), zero-filtered, no crop, at 0.2 m: 7881 occupied voxels at the planted poses, 18869 at
    the perturbed "GPS" poses, for the same 36000 points (origin = the first planted pose's translation)"""
    bank, off, planted, gps = ref.planted_bank()
    assert len(bank) == 36000
    org = planted[0, :3, 3]
    a = ref.integrate(bank, off, np.arange(6), planted, org, 0.2)
    b = ref.integrate(bank, off, np.arange(6), gps, org, 0.2)
    print(f"[voxel map] occupied voxels at 0.2 m: planted {len(a['keys'])}, gps {len(b['keys'])}")
    assert a["count"].sum() == b["count"].sum() == 36000 and a["status"] == b["status"] == 0
    assert len(a["keys"]) < len(b["keys"])


def test_merge_and_select_rules(scene):
    bank, off, poses = scene
    a = ref.integrate(bank, off, [0, 1, 2], poses[:3], ORIGIN, VOXEL)
    b = ref.integrate(bank, off, [4, 5], poses[4:6], ORIGIN, VOXEL)
    u = ref.merge(a, b)
    n_union = len(np.union1d(a["keys"], b["keys"]))
    assert len(u["keys"]) == n_union and 0 < len(np.intersect1d(a["keys"], b["keys"])) < len(b["keys"])
    assert u["count"].sum() == a["count"].sum() + b["count"].sum() and ref.same(u, ref.merge(b, a))
    over = ref.merge(a, b, capacity_out=n_union - 1)
    assert ref.same(over, a) and over["status"] == ref.CAPACITY
    assert ref.same(ref.merge(a, ref.empty()), a) and ref.same(ref.merge(ref.empty(), a), a)
    c = ref.centroids(u, ORIGIN, VOXEL)
    box = np.array([[0.0, 0.0, 0.0, 2.0, 2.0, 2.0], [1.0, 0.0, 0.0, 2.0, 2.0, 2.0], [500.0, 0.0, 0.0, 1.0, 1.0, 1.0]])
    s = ref.select(u, ORIGIN, VOXEL, boxes=box, relative=True)
    inside = (np.abs(c) < 2.0).all(axis=1)
    assert s["offsets"][1] == inside.sum() > 10 and s["offsets"][3] == s["offsets"][2] and s["status"] == 0
    assert np.array_equal(s["points"][: s["offsets"][1]], c[inside]) and np.abs(s["points"]).max() <= 2.0
    assert ref.select(u, ORIGIN, VOXEL, boxes=box, capacity=int(s["offsets"][-1]) - 1)["offsets"].tolist() == [0, 0, 0, 0]
    whole = ref.select(u, ORIGIN, VOXEL, min_count=2, min_obs=2)
    assert whole["offsets"].tolist() == [0, int(((u["count"] >= 2) & (u["obs"] >= 2)).sum())] and 0 < whole["offsets"][1] < len(c)


def test_scan_to_map_condition_holds_for_the_restatements():
    """the condition of the GPU seam test, for the restatements alone: every scan of planted_sequence(), cropped and downsampled
    as the bank does (downsample_f64), started at its "GPS" pose against the numpy map of the other five scans at their planted
    poses (0.2 m, a 30 m box around the start, relative), ends nearer to its planted pose under icp_f64.  Frobenius distances,
    start -> end: 0.125 -> 0.0067, 0.284 -> 0.0079, 0.174 -> 0.0030, 0.182 -> 0.0044, 0.231 -> 0.0045, 0.193 -> 0.0052; fitness
    0.936 to 0.947."""
    from tests import tuples_data as D
    from tests.test_icp_host import downsample_f64, icp_f64
    raws, planted, gps = D.planted_sequence()
    clouds = [downsample_f64(D.zero_filtered(r), 0.1, (-80., 80., -80., 80., -0.9, None))[0] for r in raws]
    off = np.zeros(7, np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    bank, org = np.concatenate(clouds), planted[0, :3, 3]
    for k in range(6):
        others = [j for j in range(6) if j != k]
        rec = ref.integrate(bank, off, others, planted[others], org, 0.2)
        centre = gps[k, :3, 3]
        tgt = ref.select(rec, org, 0.2, boxes=np.concatenate([centre, [30.0] * 3])[None], relative=True)["points"]
        T0 = gps[k].copy()
        T0[:3, 3] = 0.0
        r = icp_f64(clouds[k], tgt, T0, 1.2, 200)
        pose = r["T"].copy()
        pose[:3, 3] += centre
        d_init, d_ref = np.linalg.norm(gps[k] - planted[k]), np.linalg.norm(pose - planted[k])
        print(f"[voxel map] scan {k}: |gps - planted| {d_init:.4f}, |refined - planted| {d_ref:.4f}, fitness {r['fitness']:.3f}")
        assert d_ref < d_init, k


# ----------------------------------------------------------------------------- the C ABI
def test_symbols_declared_and_exported(lib):
    from egonn_amd import _lib
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for bit, value in (("RANGE", 1), ("CAPACITY", 2), ("BAD_INDEX", 4)):
        assert re.search(rf"EGONN_VMAP_STATUS_{bit} = {value}\b", header)
    src = open(os.path.join(REPO, "egonn_amd", "csrc", "voxel_map.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*(float|double)|unsafeAtomicAdd|atomicAdd_system", src), "integer atomics only"


def _refused(lib, rc, needle):
    assert rc == 1, rc                              # EGONN_STATUS_INVALID: returned before any device work
    assert needle in lib.egonn_last_error().decode(), lib.egonn_last_error()


def _broken(args, at, value):
    out = list(args)
    out[at] = value
    return out


def test_c_entries_refuse_bad_arguments_before_any_launch(lib):
    """one valid-looking argument list per entry point, broken in one place per case: every refusal is decided on the host from
    the scalar arguments, the pointers are never dereferenced (small fake addresses, 256-byte aligned where that is asked),
    and no GPU is present when this runs"""
    p, s = C.c_void_p(256), C.c_void_p(4096)
    d3 = lambda *v: (C.c_double * 3)(*v)             # noqa: E731
    org, nan, inf = d3(0.0, 0.0, 0.0), float("nan"), float("inf")
    # integrate: bank n_bank off n_clouds pick poses n_obs origin voxel points_capacity keys sums count obs capacity n_out status scratch bytes stream
    need = lib.egonn_voxel_map_integrate_scratch_bytes(1000, 4)
    assert need > 0 and need % 256 == 0
    ok = [p, 1000, p, 4, p, p, 4, org, 0.2, 1000, p, p, p, p, 1000, p, p, s, need, None]
    f = lib.egonn_voxel_map_integrate
    for at, value, needle in ((6, 0, "n_obs"), (6, 4097, "n_obs"), (1, -1, "bad shape"), (3, -1, "bad shape"), (9, -1, "points_capacity"),
                              (9, 1 << 31, "points_capacity"), (14, -1, "capacity"), (14, 1 << 31, "capacity"), (8, 0.0, "voxel"),
                              (8, -0.2, "voxel"), (8, nan, "voxel"), (8, inf, "voxel"), (7, d3(0.0, nan, 0.0), "origin"),
                              (7, d3(inf, 0.0, 0.0), "origin"), (7, None, "origin"), (0, None, "null"), (2, None, "null"),
                              (4, None, "null"), (5, None, "null"), (10, None, "null"), (11, None, "null"), (12, None, "null"),
                              (13, None, "null"), (15, None, "null"), (16, None, "null"), (17, None, "null"),
                              (17, C.c_void_p(4096 + 8), "256-byte aligned"), (18, need - 1, "scratch needs")):
        _refused(lib, f(*_broken(ok, at, value)), needle)
    assert lib.egonn_voxel_map_integrate_scratch_bytes(-1, 4) == -1 and lib.egonn_voxel_map_integrate_scratch_bytes(1 << 31, 4) == -1
    assert lib.egonn_voxel_map_integrate_scratch_bytes(10, 0) == -1 and lib.egonn_voxel_map_integrate_scratch_bytes(10, 4097) == -1
    assert lib.egonn_voxel_map_integrate_scratch_bytes(0, 1) > 0
    # merge: A (keys sums count obs n) capacity_a B (...) capacity_b out (keys sums count obs) capacity_out n_out status scratch bytes stream
    q, o = C.c_void_p(512), C.c_void_p(768)
    need = lib.egonn_voxel_map_merge_scratch_bytes(100, 50, 150)
    assert need > 0
    ok = [p, p, p, p, p, 100, q, q, q, q, q, 50, o, o, o, o, 150, p, p, s, need, None]
    f = lib.egonn_voxel_map_merge
    for at, value, needle in ((5, -1, "capacity_a"), (11, -1, "capacity_b"), (16, 99, "capacity_out"), (16, 1 << 31, "capacity_out"),
                              (11, 1 << 31, "capacity_b"), (0, None, "null"), (3, None, "null"), (4, None, "null"), (6, None, "null"),
                              (10, None, "null"), (12, None, "null"), (15, None, "null"), (17, None, "null"), (18, None, "null"),
                              (19, None, "null"), (12, p, "must not be A or B"), (12, q, "must not be A or B"),
                              (19, C.c_void_p(4096 + 128), "256-byte aligned"), (20, need - 1, "scratch needs")):
        _refused(lib, f(*_broken(ok, at, value)), needle)
    assert lib.egonn_voxel_map_merge_scratch_bytes(-1, 5, 5) == -1 and lib.egonn_voxel_map_merge_scratch_bytes(5, -1, 5) == -1
    assert lib.egonn_voxel_map_merge_scratch_bytes(5, 5, 4) == -1 and lib.egonn_voxel_map_merge_scratch_bytes(0, 0, 0) > 0
    # select: keys sums count obs n_dev capacity_map origin voxel min_count min_obs boxes n_boxes relative points offsets count obs capacity status scratch bytes stream
    need = lib.egonn_voxel_map_select_scratch_bytes(1000, 8)
    assert need > 0
    ok = [p, p, p, p, p, 1000, org, 0.2, 1, 1, q, 8, 1, o, o, o, o, 500, p, s, need, None]
    f = lib.egonn_voxel_map_select
    for at, value, needle in ((5, -1, "capacity_map"), (5, 1 << 31, "capacity_map"), (11, -1, "n_boxes"), (11, 4097, "n_boxes"),
                              (17, -1, "capacity"), (7, 0.0, "voxel"), (7, nan, "voxel"), (7, inf, "voxel"),
                              (6, d3(nan, 0.0, 0.0), "origin"), (6, None, "origin"), (8, -1, "min_count"), (9, -1, "min_obs"),
                              (10, None, "boxes and n_boxes"), (11, 0, "boxes and n_boxes"), (0, None, "null"), (1, None, "null"),
                              (4, None, "null"), (14, None, "null"), (18, None, "null"), (19, None, "null"), (13, None, "null"),
                              (19, C.c_void_p(4096 + 64), "256-byte aligned"), (20, need - 1, "scratch needs")):
        _refused(lib, f(*_broken(ok, at, value)), needle)
    whole = [p, p, p, p, p, 1000, org, 0.2, 1, 1, None, 0, 1, o, o, o, o, 500, p, s, lib.egonn_voxel_map_select_scratch_bytes(1000, 0), None]
    _refused(lib, f(*whole), "relative needs boxes")
    assert lib.egonn_voxel_map_select_scratch_bytes(-1, 0) == -1 and lib.egonn_voxel_map_select_scratch_bytes(10, 4097) == -1
    assert lib.egonn_voxel_map_select_scratch_bytes(0, 0) > 0


# ----------------------------------------------------------------------------- the Python surface
class _Bank:
    """what VoxelMap.insert reads of a CloudBank before it asks for a device"""

    def __init__(self, sizes):
        self._sizes = np.asarray(sizes, np.int64)

    def __len__(self):
        return len(self._sizes)

    def sizes(self):
        return self._sizes


def test_python_refuses_bad_arguments_before_asking_for_a_device(lib):
    import torch
    import egonn_amd
    from egonn_amd import mapping as M
    assert egonn_amd.VoxelMap is M.VoxelMap and egonn_amd.build_map is M.build_map and egonn_amd.refine_against_map is M.refine_against_map
    for bad in (0.0, -0.2, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            M.VoxelMap(bad)
    for bad in ((0, 0), (0, 0, float("nan")), np.zeros((3, 3))):
        with pytest.raises(ValueError, match="origin"):
            M.VoxelMap(origin=bad)
    for bad in (0, -5, 2 ** 31):
        with pytest.raises(ValueError, match="capacity"):
            M.VoxelMap(capacity=bad)
    with pytest.raises(ValueError, match="chunk_points"):
        M.VoxelMap(chunk_points=0)
    bank, eye = _Bank([5, 0, 7]), np.tile(np.eye(4), (3, 1, 1))
    vm = M.VoxelMap()
    with pytest.raises(ValueError, match=r"\(3, 4, 4\)"):
        vm.insert(bank, eye[:2])
    with pytest.raises(ValueError, match=r"4, 4\)"):
        vm.insert(bank, np.zeros((3, 3, 4)))
    with pytest.raises(ValueError, match="pick outside"):
        vm.insert(bank, eye, pick=[0, 1, 3])
    with pytest.raises(ValueError, match="at least one"):
        vm.insert(bank, eye[:0], pick=[])
    nan_pose = eye.copy()
    nan_pose[0, 1, 3] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        vm.insert(bank, nan_pose)
    with pytest.raises(ValueError, match="min_count"):
        vm.points(min_count=0)
    with pytest.raises(ValueError, match="min_count"):
        vm.submaps(np.zeros((2, 3)), 5.0, min_observations=0)
    with pytest.raises(ValueError, match="centers"):
        vm.submaps(np.zeros((2, 2)), 5.0)
    with pytest.raises(ValueError, match="centers"):
        vm.submaps(np.zeros((0, 3)), 5.0)
    with pytest.raises(ValueError, match="centers"):
        vm.submaps(np.zeros((4097, 3)), 5.0)
    for bad in (0.0, -1.0, float("nan"), (1.0, 2.0), (1.0, 2.0, float("inf"))):
        with pytest.raises(ValueError, match="half_extent"):
            vm.submaps(np.zeros((2, 3)), bad)
    with pytest.raises(ValueError, match="capacity"):
        vm.submaps(np.zeros((2, 3)), 5.0, capacity=-1)
    with pytest.raises(ValueError, match="empty"):
        vm.submaps(np.zeros((2, 3)), 5.0)
    with pytest.raises(ValueError, match="empty"):
        vm.points()
    with pytest.raises(ValueError, match="empty"):
        vm.save("nowhere.npz")
    with pytest.raises(ValueError, match=r"\(2, 4, 4\)"):
        M.refine_against_map(vm, bank, [0, 1], eye)
    assert vm.n_voxels == 0 and vm.status == 0 and vm.origin is None, "nothing above asked for a device or changed the map"
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            vm.insert(bank, eye)


def test_load_refuses_other_files(tmp_path):
    from egonn_amd import VoxelMap
    path = str(tmp_path / "junk.npz")
    np.savez(path, keys=np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="not a voxel map"):
        VoxelMap.load(path)
