"""CPU tests of the pose-graph layer: the new symbols, every refusal of the entry points (made on the host before any launch, so
none of this needs a device), the scratch size, the float64 restatement tests/pose_graph_ref.py on hand-made graphs whose
numbers are written out here, and the argument checks of the Python surface."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import pose_graph_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["egonn_pose_graph_scratch_bytes", "egonn_pose_graph_odometry", "egonn_pose_graph_plan", "egonn_pose_graph_cost", "egonn_pose_graph_hessvec",
               "egonn_pose_graph_optimize"]
INVALID = 1


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_new_symbols_declared_and_exported(built):
    import egonn_amd
    from egonn_amd import _lib, pose_graph
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    declared = set(re.findall(r"\b(egonn_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for name in ("pose_graph_cost", "pose_graph_hessvec", "optimize_pose_graph", "odometry_edges", "loop_edges", "optimize_trajectory"):
        assert getattr(egonn_amd, name) is getattr(pose_graph, name) and name in egonn_amd.__all__
    bits = dict(re.findall(r"EGONN_PG_STATUS_([A-Z_]+) = (\d+)", header))
    for name in ("BAD_INDEX", "SELF_LOOP", "NONFINITE", "NEGATIVE_WEIGHT", "ANGLE", "ISOLATED", "PIVOT"):
        assert int(bits[name]) == getattr(pose_graph, name) == getattr(ref, name), name
    assert len(set(bits.values())) == len(bits)


def test_scratch_bytes(built):
    from egonn_amd import _lib
    f = _lib.load().egonn_pose_graph_scratch_bytes
    for bad in ((0, 5, 10), (-1, 5, 10), (5, -1, 10), (5, 5, 0), (5, 5, -3), (1 << 31, 5, 10), (5, 1 << 30, 10)):
        assert f(*bad) == -1, bad
    assert f(1, 0, 1) > 0 and f(1, 0, 1) % 256 == 0
    for a, b in (((10, 20, 5), (1000, 20, 5)), ((10, 20, 5), (10, 2000, 5)), ((10, 20, 5), (10, 20, 5000)),
                 ((20000, 22000, 100), (20001, 22000, 100)), ((64, 1, 1), (65, 1, 1))):
        assert f(*a) <= f(*b), (a, b)
    assert f(1000, 20, 5) > f(10, 20, 5) and f(10, 2000, 5) > f(10, 20, 5)
    # linear in the graph: no n x n or n x E buffer
    assert f(20000, 22000, 4000) < 20000 * 2000 + 22000 * 2000


def test_argument_checks_need_no_gpu(built):
    """every up-front refusal returns the library's invalid status before anything is launched"""
    from egonn_amd import _lib
    lib = _lib.load()
    one, big = 256, 1 << 40      # non-null, aligned, never dereferenced: every call below fails its argument check first
    nan, inf = math.nan, math.inf
    need = lib.egonn_pose_graph_scratch_bytes(10, 12, 50)

    def plan(ei=one, Z=one, w=None, fixed=None, n=10, E=12, est=one, gst=one, scratch=one, nbytes=big):
        return lib.egonn_pose_graph_plan(ei, Z, w, fixed, n, E, est, gst, scratch, nbytes, None)
    for kw, word in ((dict(ei=None), b"null"), (dict(Z=None), b"null"), (dict(est=None), b"null"), (dict(gst=None), b"null"),
                     (dict(n=0), b"n=0"), (dict(n=-4), b"n=-4"), (dict(E=-1), b"E=-1"), (dict(scratch=None), b"scratch needs"),
                     (dict(nbytes=need - 1), b"scratch needs"), (dict(scratch=one + 8), b"256-byte aligned")):
        assert plan(**kw) == INVALID, kw
        assert word in lib.egonn_last_error(), (kw, lib.egonn_last_error())

    for args, word in (((None, 10, one, one), b"null"), ((one, 10, None, one), b"null"), ((one, 10, one, None), b"null"),
                       ((one, 0, one, one), b"n=0"), ((one, 1 << 31, one, one), b"n=")):
        assert lib.egonn_pose_graph_odometry(*args, None) == INVALID, args
        assert word in lib.egonn_last_error(), (args, lib.egonn_last_error())

    def cost(poses=one, n=10, E=12, Z=one, delta=0.0, c=one, r=one, rho=one, s=one, g=one, est=one, scratch=one, nbytes=big):
        return lib.egonn_pose_graph_cost(poses, n, E, Z, delta, c, r, rho, s, g, est, scratch, nbytes, None)
    for kw, word in ((dict(poses=None), b"null"), (dict(Z=None), b"null"), (dict(c=None), b"null"), (dict(r=None), b"null"),
                     (dict(rho=None), b"null"), (dict(s=None), b"null"), (dict(g=None), b"null"), (dict(est=None), b"null"),
                     (dict(n=0), b"n=0"), (dict(E=-1), b"E=-1"), (dict(delta=-1.0), b"robust_delta"), (dict(delta=nan), b"robust_delta"),
                     (dict(delta=inf), b"robust_delta"), (dict(scratch=None), b"scratch needs"), (dict(nbytes=need - 1), b"scratch needs")):
        assert cost(**kw) == INVALID, kw
        assert word in lib.egonn_last_error(), (kw, lib.egonn_last_error())

    def hv(poses=one, n=10, E=12, Z=one, delta=0.0, lam=0.0, p=one, out=one, est=one, scratch=one, nbytes=big):
        return lib.egonn_pose_graph_hessvec(poses, n, E, Z, delta, lam, p, out, est, scratch, nbytes, None)
    for kw, word in ((dict(poses=None), b"null"), (dict(Z=None), b"null"), (dict(p=None), b"null"), (dict(out=None), b"null"),
                     (dict(est=None), b"null"), (dict(n=0), b"n=0"), (dict(E=-1), b"E=-1"), (dict(delta=-1.0), b"robust_delta"),
                     (dict(lam=-1.0), b"lambda"), (dict(lam=nan), b"lambda"), (dict(scratch=None), b"scratch needs"),
                     (dict(nbytes=need - 1), b"scratch needs")):
        assert hv(**kw) == INVALID, kw
        assert word in lib.egonn_last_error(), (kw, lib.egonn_last_error())

    def opt(poses=one, n=10, E=12, Z=one, delta=0.0, max_it=5, pcg=50, pcg_tol=1e-8, l0=1e-4, lmin=1e-10, lmax=1e10, rel=0.0,
            gtol=0.0, pout=one, trace=one, acc=one, cnt=one, lam=one, est=one, gst=one, scratch=one, nbytes=big):
        return lib.egonn_pose_graph_optimize(poses, n, E, Z, delta, max_it, pcg, pcg_tol, l0, lmin, lmax, rel, gtol, pout, trace, acc,
                                             cnt, lam, est, gst, scratch, nbytes, None)
    for kw, word in ((dict(poses=None), b"null"), (dict(Z=None), b"null"), (dict(pout=None), b"null"), (dict(trace=None), b"null"),
                     (dict(acc=None), b"null"), (dict(cnt=None), b"null"), (dict(lam=None), b"null"), (dict(est=None), b"null"),
                     (dict(gst=None), b"null"), (dict(n=0), b"n=0"), (dict(E=-1), b"E=-1"), (dict(max_it=0), b"max_iterations=0"),
                     (dict(max_it=-2), b"max_iterations=-2"), (dict(pcg=0), b"pcg_iterations=0"), (dict(delta=-1.0), b"tolerance"),
                     (dict(delta=nan), b"tolerance"), (dict(pcg_tol=-1e-3), b"tolerance"), (dict(pcg_tol=inf), b"tolerance"),
                     (dict(rel=-1.0), b"tolerance"), (dict(rel=nan), b"tolerance"), (dict(gtol=-1.0), b"tolerance"),
                     (dict(gtol=inf), b"tolerance"), (dict(lmin=0.0), b"lambda_min"), (dict(l0=1e-12), b"lambda_min"),
                     (dict(lmax=1e-6), b"lambda_min"), (dict(lmax=inf), b"lambda_min"), (dict(l0=nan), b"lambda_min"),
                     (dict(scratch=None), b"scratch needs"), (dict(nbytes=need - 1), b"scratch needs"),
                     (dict(scratch=one + 16), b"256-byte aligned")):
        assert opt(**kw) == INVALID, kw
        assert word in lib.egonn_last_error(), (kw, lib.egonn_last_error())


# ------------------------------------------------------------------ the restatement on hand-made graphs
def _poses(n):
    return np.tile(np.eye(4), (n, 1, 1))


def test_restated_translation_error():
    # two nodes, Z = identity, node 1 at (1, 2, 3): t_E = (1, 2, 3), cost = 1/2 * w_trans * 14 with w_trans = 2
    X = _poses(2)
    X[1, :3, 3] = [1.0, 2.0, 3.0]
    res = ref.residuals(X, [[0, 1]], np.eye(4)[None], [[5.0, 2.0]])
    assert res["r"].tolist() == [[1.0, 2.0, 3.0, 0.0, 0.0, 0.0]] and res["cost"] == pytest.approx(14.0, abs=1e-14)
    assert res["s"][0] == pytest.approx(math.sqrt(28.0), abs=1e-14) and res["rho"].tolist() == [1.0]
    _, g, _ = ref.normal_equations(X, [[0, 1]], np.eye(4)[None], [[5.0, 2.0]])
    # d t_E / d v_1 = R_E = I, d t_E / d v_0 = -I, d t_E / d w_0 = [t_M]x whose transpose annihilates t_M: g = (-+) w_trans t_E
    assert np.allclose(g, [-2, -4, -6, 0, 0, 0, 2, 4, 6, 0, 0, 0], rtol=0, atol=1e-8)
    # Huber: s = sqrt(28) > delta = 1 -> rho = 1 / s, cost = delta s - delta^2 / 2
    hub = ref.residuals(X, [[0, 1]], np.eye(4)[None], [[5.0, 2.0]], robust_delta=1.0)
    assert hub["rho"][0] == pytest.approx(1 / math.sqrt(28.0), abs=1e-15) and hub["cost"] == pytest.approx(math.sqrt(28.0) - 0.5, abs=1e-14)
    assert ref.cost(X, [[0, 1]], np.eye(4)[None], [[5.0, 2.0]], robust_delta=100.0) == pytest.approx(14.0, abs=1e-14)


def test_restated_rotation_error():
    X = _poses(2)
    X[1, :3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]                 # 90 degrees about z
    res = ref.residuals(X, [[0, 1]], np.eye(4)[None], [[3.0, 2.0]])
    assert np.allclose(res["r"][0], [0, 0, 0, 0, 0, math.pi / 2], rtol=0, atol=1e-15)
    assert res["cost"] == pytest.approx(0.5 * 3.0 * (math.pi / 2) ** 2, abs=1e-14)
    # the measurement equal to the relative pose: zero
    assert ref.cost(X, [[0, 1]], X[1][None], [[3.0, 2.0]]) == 0.0
    # just inside and just outside the supported angle
    for ang, bit in ((math.pi - 2e-3, 0), (math.pi - 5e-4, ref.ANGLE)):
        X[1, :3, :3] = ref.exp_so3([0.0, ang, 0.0])
        res = ref.residuals(X, [[0, 1]], np.eye(4)[None])
        assert res["status"][0] == bit and (res["cost"] == 0.0) == bool(bit)
        if not bit:
            assert np.allclose(res["r"][0, 3:], [0, ang, 0], rtol=0, atol=1e-12)


def test_restated_status_bits():
    Z = np.tile(np.eye(4), (6, 1, 1))
    Z[2, 0, 3] = np.nan
    Z[3, 3, 0] = 1.0
    w = np.ones((6, 2))
    w[4, 0] = -1.0
    _, _, weff, st = ref.edge_checks(3, [[0, 3], [1, 1], [0, 1], [1, 2], [0, 2], [0, 1]], Z, w)
    assert st.tolist() == [ref.BAD_INDEX, ref.SELF_LOOP, ref.NONFINITE, ref.NONFINITE, ref.NEGATIVE_WEIGHT, 0]
    assert (weff[:5] == 0).all() and (weff[5] == 1).all()


def test_restated_triangle_minimiser():
    """Three nodes on a line, node 0 fixed at the origin, identity rotations, unit weights: edges 0->1 and 1->2 measure a step of
    1, edge 0->2 measures 2.3.  With x1, x2 the free positions the cost is 1/2 [(x1 - 1)^2 + (x2 - x1 - 1)^2 + (x2 - 2.3)^2], whose
    normal equations 2 x1 - x2 = 0, -x1 + 2 x2 = 3.3 give x1 = 1.1, x2 = 2.2 and the cost 1/2 * 3 * 0.01 = 0.015."""
    X = _poses(3)
    X[1, 0, 3], X[2, 0, 3] = 0.7, 2.9
    Z = _poses(3)
    Z[0, 0, 3], Z[1, 0, 3], Z[2, 0, 3] = 1.0, 1.0, 2.3
    edges = [[0, 1], [1, 2], [0, 2]]
    res = ref.optimize(X, edges, Z, max_iterations=12)
    P = res["poses"]
    assert np.array_equal(P[0], X[0])
    assert np.allclose(P[:, 0, 3], [0.0, 1.1, 2.2], rtol=0, atol=1e-6) and np.allclose(P[:, :3, :3], np.eye(3), rtol=0, atol=1e-6)
    tr = res["cost_trace"][: res["iterations"] + 1]
    assert tr[-1] == pytest.approx(0.015, abs=1e-9) and (np.diff(tr) <= 0).all() and res["accepted"] >= 1
    assert ref.cost(P, edges, Z) == pytest.approx(tr[-1], abs=1e-15)


def test_restated_retraction():
    X = _poses(2)
    X[1, :3, :3] = ref.exp_so3([0.3, -0.2, 0.5])
    X[1, :3, 3] = [4.0, 5.0, 6.0]
    d = np.zeros((2, 6))
    d[1] = [1.0, 0.0, 0.0, 0.0, 0.0, 0.25]
    Y = ref.retract(X, d)
    assert np.array_equal(Y[0], X[0])                                               # a zero delta leaves the bits alone
    assert np.allclose(Y[1, :3, 3], X[1, :3, 3] + X[1, :3, 0], rtol=0, atol=1e-15)   # t + R e_x
    assert np.allclose(Y[1, :3, :3], X[1, :3, :3] @ ref.exp_so3([0, 0, 0.25]), rtol=0, atol=1e-15)
    assert np.allclose(ref.log_so3(ref.exp_so3([1e-9, 0, 0])), [1e-9, 0, 0], rtol=0, atol=1e-24)


# ------------------------------------------------------------------ the host side of the Python surface
def test_edge_builders_check_their_arguments():
    from egonn_amd import loop_edges, odometry_edges, optimize_pose_graph, pose_graph_cost
    with pytest.raises(ValueError, match=r"poses \(n, 4, 4\)"):
        odometry_edges(np.zeros((5, 3, 4)))
    with pytest.raises(ValueError, match=r"poses \(n, 4, 4\)"):
        odometry_edges(np.zeros((0, 4, 4)))
    for bad in ((1.0,), (1.0, -2.0), (math.nan, 1.0), (1.0, math.inf), "ab", 3.0):
        with pytest.raises(ValueError, match="weight"):
            odometry_edges(np.zeros((5, 4, 4)), weight=bad)
        with pytest.raises(ValueError, match="weight"):
            loop_edges({}, weight=bad)
    b = 4
    good = {"best_index": torch.zeros(b, dtype=torch.int32), "index": torch.arange(b, dtype=torch.int32),
            "T_rel": torch.zeros(b, 4, 4, dtype=torch.float64), "loop": torch.zeros(b, dtype=torch.bool)}
    for drop in good:
        with pytest.raises(ValueError, match="lacks"):
            loop_edges({k: v for k, v in good.items() if k != drop})
    for k, v in (("best_index", good["best_index"][:-1]), ("T_rel", good["T_rel"][:, :3]), ("loop", good["loop"][:2]),
                 ("index", good["index"].reshape(2, 2))):
        with pytest.raises(ValueError, match="must agree in b"):
            loop_edges(dict(good, **{k: v}))
    e = loop_edges(dict(good, loop=torch.tensor([True, False, True, False])), weight=(4.0, 9.0))      # CPU tensors: no device needed
    assert e["weights"].tolist() == [[4.0, 9.0], [0.0, 0.0], [4.0, 9.0], [0.0, 0.0]] and e["edge_index"].shape == (b, 2)
    X, Z, ei = np.zeros((3, 4, 4)), np.zeros((2, 4, 4)), np.zeros((2, 2), np.int32)
    for kw, word in ((dict(poses=np.zeros((3, 4, 3))), "poses"), (dict(edge_index=np.zeros((2, 3), np.int32)), "edge_index"),
                     (dict(Z=np.zeros((3, 4, 4))), "Z"), (dict(weights=np.zeros((2, 3))), "weights")):
        a = dict(poses=X, edge_index=ei, Z=Z)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            pose_graph_cost(**a)
    for kw in (dict(max_iterations=0), dict(pcg_iterations=0), dict(robust_delta=-1.0), dict(pcg_tol=math.nan), dict(rel_tol=math.inf),
               dict(fixed=np.zeros(4, bool))):
        with pytest.raises(ValueError):
            optimize_pose_graph(X, ei, Z, **kw)
