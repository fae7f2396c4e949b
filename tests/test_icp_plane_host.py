"""CPU tests of the point-to-plane ICP (egonn_estimate_normals / egonn_icp_plane_pairs): the symbols, the argument checks that
fail before any launch, the Python refusals that need no device, self-checks of the float64 restatement
(tests/icp_plane_ref.py) and the conditioning of the committed cases that tests/test_gpu_icp_plane.py relies on."""
import os
import re

import numpy as np
import pytest
import torch

from egonn_amd.synth import rot_zyx
from tests import icp_plane_ref as R
from tests.test_icp_host import BAND, ICP_CASES, box_displacement, icp_case_result, pose_error

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["egonn_estimate_normals", "egonn_estimate_normals_scratch_bytes", "egonn_icp_plane_pairs",
               "egonn_icp_plane_scratch_bytes"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_new_symbols_declared_and_exported(built):
    from egonn_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    declared = set(re.findall(r"\b(egonn_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for bits in ("EGONN_ICP_STATUS_SINGULAR = 16", "EGONN_NORMALS_STATUS_FEW_POINTS = 1", "EGONN_NORMALS_STATUS_RANGE = 2"):
        assert bits in header
    from egonn_amd import registration as reg
    assert (reg.ICP_SINGULAR, reg.NORMALS_FEW_POINTS, reg.NORMALS_RANGE) == (16, 1, 2) == \
        (R.ICP_SINGULAR, R.NORMALS_FEW_POINTS, R.NORMALS_RANGE)


def test_scratch_sizes(built):
    from egonn_amd import _lib
    lib = _lib.load()
    nb, pb = lib.egonn_estimate_normals_scratch_bytes, lib.egonn_icp_plane_scratch_bytes
    assert nb(50000, 1) > 0 and pb(50000, 50000, 1) > 0
    assert nb(-1, 1) == -1 and nb(1 << 31, 1) == -1 and nb(10, 0) == -1 and nb(10, 1 << 20) == -1
    assert pb(-1, 10, 1) == -1 and pb(10, 1 << 31, 1) == -1 and pb(10, 10, 0) == -1
    assert nb(100000, 1) > nb(50000, 1) and nb(50000, 16) > nb(50000, 1) and nb(0, 1) > 0
    assert pb(100000, 50000, 1) > pb(50000, 50000, 1) and pb(50000, 100000, 1) > pb(50000, 50000, 1)
    assert pb(50000, 50000, 16) > pb(50000, 50000, 1)
    # 29 partials per workgroup instead of 17
    assert pb(50000, 50000, 1) > lib.egonn_icp_scratch_bytes(50000, 50000, 1)


def test_argument_checks_need_no_gpu(built):
    """the up-front checks return the library's invalid status before anything is launched"""
    from egonn_amd import _lib
    lib = _lib.load()
    one = 256       # non-null, aligned, never dereferenced: every call below fails its argument check first
    big = 1 << 40
    nrm = lib.egonn_estimate_normals
    for knn in (2, 33, 0, -1):
        assert nrm(one, 10, one, 1, knn, one, one, None, None, one, big, None) == 1
        assert b"knn" in lib.egonn_last_error()
    assert nrm(one, 10, one, 0, 20, one, one, None, None, one, big, None) == 1
    assert b"n_clouds" in lib.egonn_last_error()
    assert nrm(one, 10, None, 1, 20, one, one, None, None, one, big, None) == 1
    assert nrm(one, 10, one, 1, 20, None, one, None, None, one, big, None) == 1
    assert b"null" in lib.egonn_last_error()
    assert nrm(one, 10, one, 1, 20, one, one, None, None, one, 8, None) == 1
    assert b"scratch" in lib.egonn_last_error()
    assert nrm(one, 10, one, 1, 20, one, one, None, None, one + 8, big, None) == 1
    assert b"scratch" in lib.egonn_last_error()
    plane = lib.egonn_icp_plane_pairs
    args = (one, one, one, one, one, None, None, None)
    assert plane(one, 10, one, one, 10, one, None, 1, None, 1.2, 200, 1e-6, 1e-6, *args, one, big, None) == 1
    assert b"tgt_normals" in lib.egonn_last_error()
    assert plane(one, 10, one, one, 10, one, one, 0, None, 1.2, 200, 1e-6, 1e-6, *args, one, big, None) == 1
    assert plane(one, 10, one, one, 10, one, one, 1, None, 0.0, 200, 1e-6, 1e-6, *args, one, big, None) == 1
    assert plane(one, 10, one, one, 10, one, one, 1, None, 1.2, -1, 1e-6, 1e-6, *args, one, big, None) == 1
    assert b"max_iteration" in lib.egonn_last_error()
    assert plane(one, 10, one, one, 10, one, one, 1, None, 1.2, 200, 1e-6, 1e-6, *args, one, 8, None) == 1
    assert b"scratch" in lib.egonn_last_error()
    assert plane(one, 10, one, one, 10, one, one, 1, None, 1.2, 200, 1e-6, 1e-6, *args, one + 8, big, None) == 1
    # a scratch that suffices for point-to-point is short for the plane call
    short = lib.egonn_icp_scratch_bytes(50000, 50000, 1)
    assert plane(one, 50000, one, one, 50000, one, one, 1, None, 1.2, 200, 1e-6, 1e-6, *args, one, short, None) == 1


def test_public_functions_exist_and_reject_bad_shapes():
    """shape errors are raised before a device is asked for: these pass (by raising) without a GPU"""
    import egonn_amd
    import inspect
    for name in ("estimate_normals", "icp_point_to_plane", "icp_pairs", "refine_pairs"):
        assert callable(getattr(egonn_amd, name)), name
    z = np.zeros
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        egonn_amd.estimate_normals(z((10, 2)), [0, 10])
    with pytest.raises(ValueError, match="offsets"):
        egonn_amd.estimate_normals(z((10, 3)), [10])
    for knn in (2, 33):
        with pytest.raises(ValueError, match="knn"):
            egonn_amd.estimate_normals(z((10, 3)), [0, 10], knn=knn)
        with pytest.raises(ValueError, match="knn"):
            egonn_amd.icp_point_to_plane(z((10, 3)), z((10, 3)), knn=knn)
    with pytest.raises(ValueError, match="tgt_normals"):
        egonn_amd.icp_pairs(z((10, 3)), [0, 10], z((10, 3)), [0, 10], tgt_normals=z((9, 3)))
    with pytest.raises(ValueError, match="tgt_normals"):
        egonn_amd.icp_pairs(z((10, 3)), [0, 10], z((10, 3)), [0, 10], tgt_normals=z((10, 4)))
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        egonn_amd.icp_point_to_plane(z((10,)), z((10, 3)))
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        egonn_amd.icp_point_to_plane(z((10, 3)), z((10, 3)), transform=np.eye(3))
    # icp(point2plane=True) keeps refusing, and says where the estimator lives
    with pytest.raises(NotImplementedError, match="icp_point_to_plane"):
        egonn_amd.icp(z((10, 3)), z((10, 3)), point2plane=True)
    # the pass-through switches exist and default to off
    from egonn_amd import Relocalizer, evaluate_local, generate_training_tuples, refine_pairs
    assert inspect.signature(evaluate_local).parameters["icp_point2plane"].default is False
    assert inspect.signature(generate_training_tuples).parameters["point2plane"].default is False
    assert inspect.signature(Relocalizer.__init__).parameters["icp_point2plane"].default is False
    assert inspect.signature(refine_pairs).parameters["point2plane"].default is False
    assert inspect.signature(refine_pairs).parameters["knn"].default == 20
    assert inspect.signature(egonn_amd.icp_pairs).parameters["tgt_normals"].default is None


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_plane_icp_has_no_cpu_path(built):
    import egonn_amd
    from egonn_amd.synth import planted_scan_pair
    s, t, _, T0 = planted_scan_pair(3, 500)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        egonn_amd.icp_point_to_plane(s, t, T0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        egonn_amd.estimate_normals(t.astype(np.float64), [0, len(t)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        egonn_amd.icp_pairs(s.astype(np.float64), [0, len(s)], t.astype(np.float64), [0, len(t)], tgt_normals=np.zeros((len(t), 3)))


# ------------------------------------------------------------------ the restatement checks itself
def test_vec6_to_T_is_a_proper_rotation():
    rng = np.random.default_rng(4)
    for _ in range(20):
        x = rng.uniform(-1, 1, 6) * np.array([3, 1.5, 3, 10, 10, 10])
        U = R.vec6_to_T(x)
        assert np.abs(U[:3, :3] @ U[:3, :3].T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(U[:3, :3]) - 1.0) < 1e-14
        assert np.array_equal(U[:3, 3], x[3:]) and np.array_equal(U[3], [0, 0, 0, 1])
        assert np.abs(U[:3, :3] - rot_zyx(x[2], x[1], x[0])).max() < 1e-14          # yaw = x2, pitch = x1, roll = x0
    assert np.array_equal(R.vec6_to_T(np.zeros(6)), np.eye(4))
    # first order: a small x0 turns y towards z
    assert R.vec6_to_T([1e-3, 0, 0, 0, 0, 0])[2, 1] > 0 and R.vec6_to_T([0, 0, 1e-3, 0, 0, 0])[1, 0] > 0


def test_one_plane_step_recovers_a_planted_pose():
    """noise-free pair with known correspondences: the residual vanishes at the planted pose whatever the normals are, and one
    Gauss-Newton step from a start 1e-6 rad / 1e-5 m away lands on it up to the second order of that start"""
    rng = np.random.default_rng(5)
    src = rng.uniform(-100, 100, size=(2000, 3)) * np.array([1, 1, 0.1])
    nrm = rng.standard_normal((2000, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    Tp = np.eye(4)
    Tp[:3, :3], Tp[:3, 3] = rot_zyx(0.4, -0.05, 0.02), [3.0, -7.0, 0.5]
    tgt = src @ Tp[:3, :3].T + Tp[:3, 3]
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = rot_zyx(1e-6, -1e-6, 1e-6), [1e-5, -1e-5, 1e-5]
    j = np.arange(2000)
    T1, cond = R.plane_step_f64(src, tgt, nrm, D @ Tp, j)
    assert cond < 1e6 and box_displacement(D @ Tp, Tp) > 1e-5
    assert box_displacement(T1, Tp) <= 1e-9, box_displacement(T1, Tp)
    # rows without a correspondence do not enter
    j2 = j.copy()
    j2[::2] = -1
    assert box_displacement(R.plane_step_f64(src, tgt, nrm, D @ Tp, j2)[0], Tp) <= 1e-9
    # one plane: rank deficient, no step
    flat = np.tile([0.0, 0.0, 1.0], (2000, 1))
    assert R.plane_step_f64(src, tgt, flat, Tp, j)[0] is None


def test_knn_restatement():
    rng = np.random.default_rng(6)
    p = np.round(rng.uniform(-2, 2, size=(300, 3)) * 4) / 4          # a 0.25 m lattice: exact d2, many ties
    p[7] = p[3]
    idx, gap = R.knn_f64(p, 5)
    d2 = ((p[:, None] - p[None]) ** 2).sum(-1)
    for i in (0, 3, 7, 150, 299):
        order = sorted(range(300), key=lambda j: (d2[i, j], j))
        assert idx[i].tolist() == order[:5] and gap[i] == d2[i, order[5]] - d2[i, order[4]]
    assert idx[3, :2].tolist() == [3, 7] and idx[7, :2].tolist() == [3, 7]       # duplicates: the lower index first
    assert (gap == 0).any()
    few, g = R.knn_f64(p[:4], 20)
    assert (few[:, :4] >= 0).all() and (few[:, 4:] == -1).all() and np.isinf(g).all()
    # the tree route agrees with brute force where the gap is open
    q = rng.uniform(-20, 20, size=(1500, 3))
    a, ga = R.knn_f64(q, 8)
    d2 = R._d2(q[:, None, :], q[None])
    b = np.argsort(d2, axis=1, kind="stable")[:, :8]
    assert np.array_equal(a[ga > BAND], b[ga > BAND]) and (ga > BAND).mean() > 0.99


def test_normals_restatement():
    rng = np.random.default_rng(7)
    # points on the plane z = 0.1 x + 5, seen from the origin: the normal is +-(0.1, 0, -1) / |.|, turned towards the origin
    xy = rng.uniform(-3, 3, size=(400, 2))
    p = np.column_stack([xy, 0.1 * xy[:, 0] + 5.0])
    idx, _ = R.knn_f64(p, 20)
    nrm, lam, C = R.normals_f64(p, idx)
    want = np.array([0.1, 0.0, -1.0]) / np.sqrt(1.01)
    assert np.abs(nrm - want).max() < 1e-9 and ((nrm * p).sum(1) < 0).all()
    assert (lam[:, 0] < 1e-12).all() and (np.diff(lam, axis=1) >= 0).all() and np.abs(C - C.transpose(0, 2, 1)).max() == 0
    # two points: degenerate
    n2, _, _ = R.normals_f64(p[:2], R.knn_f64(p[:2], 20)[0])
    assert np.array_equal(n2, [[0, 0, 1.0], [0, 0, 1.0]])


# ------------------------------------------------------------------ the conditioning the GPU tests rely on
@pytest.mark.parametrize("name", list(ICP_CASES))
def test_cases_are_well_conditioned(name):
    c = R.plane_case(name)
    free, lam = c["free"], c["lam"]
    point = icp_case_result(name)
    rel = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    print(name, "target rows", len(c["tgt"]), "smallest knn gap", c["gap"].min(), "smallest (l1-l0)/l2", rel.min(), "plane rounds",
          free["iterations"], "point rounds", point["iterations"], "largest cond", max(free["conds"]), "final err",
          pose_error(free["T"], c["T_planted"]))
    assert (c["gap"] > BAND).all(), int((c["gap"] <= BAND).sum())
    assert (rel >= 1e-6).all(), rel.min()
    assert max(free["conds"]) <= 1e4
    assert free["status"] == 0 and free["iterations"] <= point["iterations"] and not any(free["near_stop"])
    assert max(free["near_rows"]) <= 1e-3
    rot0, tr0 = pose_error(c["T_init"], c["T_planted"])
    rot1, tr1 = pose_error(free["T"], c["T_planted"])
    assert rot1 < rot0 and tr1 < tr0
