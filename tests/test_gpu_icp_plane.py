"""GPU tests of the point-to-plane ICP (run with -m gpu on an MI355X) against the float64 restatement of
tests/icp_plane_ref.py: the neighbour lists exactly on lattice clouds, the normals of the six committed targets, every plane
round teacher-forced from the device's trace, the free-running result, the edges, the invariances (runs, batch, graph) and the
wrappers.

Measured on an MI355X (the tests print them and assert the inequalities on the values they measure):
  MEASURED_RAYLEIGH    largest (n^T C n - l0) / l2 over every row of the six targets, C in float64 from the device's own
                       neighbour list, l0 <= l1 <= l2 from np.linalg.eigh.  R_TOL must be >= 100 x that and <= 1e-9.  The
                       excess is of second order in the eigenvector's error, so what is left is the rounding of the
                       expression itself, a few 2^-53: R_TOL = 1e-12 was set from that before the first run.
  MEASURED_PLANE_DIFF  largest displacement of a point of the +-114 m box between the device's T_k+1 and plane_step_f64 on the
                       device's correspondences and normals under the device's T_k, over every round of every case.  BAND
                       (tests/test_icp_host.py, 1e-8 m) must be >= 100 x that.
  MEASURED_PLANE_FREE  the same displacement between the device's final T and the free-running restatement's.  FREE_TOL must
                       be >= 10 x that and <= 1 mm."""
import numpy as np
import pytest
import torch

from tests import icp_plane_ref as R
from tests.test_icp_host import (BAND, ICP_CASES, ICP_EMPTY, ICP_FEW_CORR, ICP_MAX_ITER, NEAR_ROW_CAP, box_displacement,
                                 evaluate_f64, icp_case, pose_error)

pytestmark = pytest.mark.gpu

MEASURED_RAYLEIGH = 6.172e-16     # as printed by test_normals_of_the_case_targets on an MI355X (60 282 rows of the 6 targets)
MEASURED_PLANE_DIFF = 4.020e-14   # metres, as printed by test_plane_band_measurement on an MI355X (34 rounds of the 6 cases)
MEASURED_PLANE_FREE = 3.178e-14   # metres, the largest value printed by test_free_running on an MI355X
R_TOL = 1e-12
FREE_TOL = 1e-6               # metres, the tolerance of the point-to-point tests
MAX_DIST = 1.2
KNN = 20
SMALL = [n for n in ICP_CASES if n != "scan_50k"]
KEYS = ("T", "fitness", "inlier_rmse", "iterations", "status", "T_trace", "eval_trace")


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


def _np(t):
    return t.detach().cpu().numpy()


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _offsets(clouds):
    off = np.zeros(len(clouds) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    return off


def _cat(clouds):
    return np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds]) if clouds else np.zeros((0, 3))


def _normals(gpu, clouds, knn=KNN):
    """-> per-cloud lists normals, neighbors, eigenvalues and the status array"""
    off = _offsets(clouds)
    out = gpu.estimate_normals(_cu(_cat(clouds)), _cu(off), knn, True)
    torch.cuda.synchronize()
    sp = lambda k: [_np(out[k])[off[c]:off[c + 1]] for c in range(len(clouds))]      # noqa: E731
    return dict(normals=sp("normals"), neighbors=sp("neighbors"), eigenvalues=sp("eigenvalues"), status=_np(out["status"]))


def _plane(gpu, srcs, tgts, nrms, T_init=None, max_iteration=200, max_dist=MAX_DIST):
    so, to = _offsets(srcs), _offsets(tgts)
    out = gpu.icp_pairs(_cu(_cat(srcs)), _cu(so), _cu(_cat(tgts)), _cu(to), None if T_init is None else _cu(np.asarray(T_init, np.float64)),
                        max_dist, max_iteration, True, _cu(_cat(nrms)))
    torch.cuda.synchronize()
    r = {k: _np(v) for k, v in out.items() if not k.startswith("_")}
    r["corr"] = [r["corr"][so[p]:so[p + 1]] for p in range(len(srcs))]
    return r


def _lattice(n, seed, side=9):
    """n distinct points of a 0.25 m lattice around (3, -2, 1.5): every coordinate and every d2 is exact in fp64"""
    rng = np.random.default_rng([seed, n])
    cells = rng.choice(side ** 3, size=n, replace=False)
    ijk = np.stack([cells // (side * side), (cells // side) % side, cells % side], 1).astype(np.float64)
    return (ijk - side // 2) * 0.25 + np.array([3.0, -2.0, 1.5])


# ------------------------------------------------------------------ 1. neighbour lists, exact, at the edges
LATTICE_SIZES = (1, 2, 3, 19, 20, 21, 255, 256, 257, 513)


def _check_lists(dev, c, cloud, knn):
    idx, _ = R.knn_f64(cloud, knn)
    assert np.array_equal(dev["neighbors"][c], idx), (len(cloud), knn, int((dev["neighbors"][c] != idx).any(1).sum()))
    assert dev["status"][c] == (R.NORMALS_FEW_POINTS if len(cloud) < knn else 0)
    nrm = dev["normals"][c]
    if len(cloud) < 3:
        assert np.array_equal(nrm, np.tile([0.0, 0.0, 1.0], (len(cloud), 1)))
    assert (np.abs(np.linalg.norm(nrm, axis=1) - 1.0) <= 1e-12).all()


@pytest.mark.parametrize("knn", [3, 20, 32])
def test_neighbour_lists_on_lattice_clouds(gpu, knn):
    clouds = [_lattice(n, 1) for n in LATTICE_SIZES]
    batch = _normals(gpu, clouds, knn)
    for c, cloud in enumerate(clouds):
        _check_lists(batch, c, cloud, knn)
        alone = _normals(gpu, [cloud], knn)
        _check_lists(alone, 0, cloud, knn)
        for k in ("normals", "neighbors", "eigenvalues"):
            assert np.array_equal(alone[k][0], batch[k][c]), (k, len(cloud))
    assert any((R.knn_f64(cloud, knn)[1] == 0).any() for cloud in clouds)       # there are exact ties at the boundary


def test_neighbour_lists_far_point_duplicates_and_range(gpu):
    far = np.concatenate([_lattice(300, 2), [[503.0, -2.0, 1.5]]])                # the radius doubles up to the whole grid
    dup = _lattice(50, 3)
    dup[7] = dup[3]
    nan = _lattice(40, 4)
    nan[11, 1] = np.nan
    inf = _lattice(40, 5)
    inf[0, 0] = np.inf
    clouds = [far, dup, nan, _lattice(30, 6), inf, np.zeros((0, 3))]
    dev = _normals(gpu, clouds)
    for c in (0, 1, 3):
        _check_lists(dev, c, clouds[c], KNN)
    assert dev["neighbors"][0][300, 0] == 300 and dev["neighbors"][1][3, :2].tolist() == [3, 7] and \
        dev["neighbors"][1][7, :2].tolist() == [3, 7]
    for c in (2, 4):
        assert dev["status"][c] == R.NORMALS_RANGE and np.array_equal(dev["normals"][c], np.tile([0.0, 0.0, 1.0], (40, 1)))
    assert dev["status"][5] == R.NORMALS_FEW_POINTS
    # offsets beyond the capacity are clipped to it
    pts, off = _cat(clouds[:2]), _offsets(clouds[:2])
    off[-1] += 1000
    out = gpu.estimate_normals(_cu(pts), _cu(off), KNN, True)
    torch.cuda.synchronize()
    assert np.array_equal(_np(out["neighbors"])[301:], dev["neighbors"][1]) and np.array_equal(_np(out["normals"])[:301], dev["normals"][0])


# ------------------------------------------------------------------ 2. normals of the six case targets
_NRM = {}


def _case_normals(gpu):
    """device normals of the six targets, one call"""
    if not _NRM:
        names = list(ICP_CASES)
        dev = _normals(gpu, [icp_case(n)["tgt"] for n in names])
        assert (dev["status"] == 0).all()
        for c, n in enumerate(names):
            _NRM[n] = {k: dev[k][c] for k in ("normals", "neighbors", "eigenvalues")}
    return _NRM


def test_normals_of_the_case_targets(gpu):
    worst = 0.0
    for name in ICP_CASES:
        c, dev = R.plane_case(name), _case_normals(gpu)[name]
        p, near = c["tgt"], c["gap"] <= BAND
        assert near.mean() <= NEAR_ROW_CAP
        assert np.array_equal(dev["neighbors"][~near], c["idx"][~near]), (name, int((dev["neighbors"] != c["idx"]).any(1).sum()))
        C, m = R.covariance_f64(p, dev["neighbors"].astype(np.int64))
        lam = np.linalg.eigvalsh(C)
        n = dev["normals"]
        assert (m == KNN).all() and (np.abs(np.linalg.norm(n, axis=1) - 1.0) <= 1e-12).all()
        excess = (np.einsum("na,nab,nb->n", n, C, n) - lam[:, 0]) / lam[:, 2]
        worst = max(worst, float(excess.max()))
        assert excess.max() <= R_TOL, (name, excess.max())
        dot = (n * p).sum(1)
        assert (dot[np.abs(dot) > 1e-6 * np.linalg.norm(p, axis=1)] < 0).all()
        # Jacobi is backward stable: the eigenvalues are those of a matrix within a few 2^-53 |C| of C
        assert (np.abs(dev["eigenvalues"] - lam) <= 1e-12 * lam[:, 2:3]).all() and (np.diff(dev["eigenvalues"], axis=1) >= 0).all()
        print(name, "rows", len(p), "largest Rayleigh excess", excess.max(), "rows near a tie", int(near.sum()))
    print("MEASURED_RAYLEIGH =", worst)
    assert 100.0 * worst <= R_TOL and 100.0 * MEASURED_RAYLEIGH <= R_TOL <= 1e-9


# ------------------------------------------------------------------ 3. every plane round, teacher-forced
_TF = {}


def _teacher_forced(gpu, name):
    if name in _TF:
        return _TF[name]
    c = icp_case(name)
    src, tgt, nrm = c["src"], c["tgt"], _case_normals(gpu)[name]["normals"]
    dev = _plane(gpu, [src], [tgt], [nrm], c["T_init"][None], c["max_iteration"])
    K = int(dev["iterations"][0])
    rec = dict(dev=dev, K=K, diff=0.0, excused=0, rows=0)
    prev = None
    for k in range(K + 1):
        Tk = dev["T_trace"][0, k]
        ev = evaluate_f64(src, tgt, Tk, MAX_DIST)
        near = (ev["gap"] <= BAND) | (ev["thr"] <= BAND)
        assert near.mean() <= NEAR_ROW_CAP, (name, k, near.mean())
        rec["excused"] += int(near.sum())
        rec["rows"] += len(src)
        one = _plane(gpu, [src], [tgt], [nrm], Tk[None], 0)              # the device's j(i) under T_k: one evaluation
        j_dev = one["corr"][0]
        assert np.array_equal(j_dev[~near], ev["j"][~near]), (name, k, int((j_dev != ev["j"])[~near].sum()))
        n_dev, sum_dev, stop_dev = dev["eval_trace"][0, k]
        assert abs(n_dev - ev["n_corr"]) <= near.sum() and one["eval_trace"][0, 0, 0] == n_dev, (name, k, n_dev, ev["n_corr"])
        if near.sum() == 0:
            assert n_dev == ev["n_corr"] and abs(sum_dev - ev["sum_d2"]) <= 1e-12 * max(ev["sum_d2"], 1.0)
        stop, bit, near_stop = R.plane_stop_rule(k, ev, prev, c["max_iteration"])
        assert not near_stop and bool(stop_dev) == stop, (name, k, stop_dev, stop)
        if not stop:
            T_next, cond = R.plane_step_f64(src, tgt, nrm, Tk, j_dev)
            assert T_next is not None and cond <= 1e4
            d = box_displacement(T_next, dev["T_trace"][0, k + 1])
            rec["diff"] = max(rec["diff"], d)
            assert d <= BAND, (name, k, d)
        else:
            assert k == K and int(dev["status"][0]) == bit
            assert np.array_equal(dev["T"][0], Tk) and not dev["T_trace"][0, k + 1:].any()
        prev = ev
    _TF[name] = rec
    return rec


@pytest.mark.parametrize("name", list(ICP_CASES))
def test_every_plane_round_teacher_forced(gpu, name):
    rec = _teacher_forced(gpu, name)
    print(name, "rounds", rec["K"], "largest T_k+1 difference on the box [m]", rec["diff"], "excused rows", rec["excused"], "of",
          rec["rows"])
    assert rec["excused"] <= NEAR_ROW_CAP * rec["rows"]


def test_plane_band_measurement(gpu):
    worst = max(_teacher_forced(gpu, name)["diff"] for name in ICP_CASES)
    print("MEASURED_PLANE_DIFF =", worst)
    assert BAND >= 100.0 * worst and BAND >= 100.0 * MEASURED_PLANE_DIFF and BAND <= 1e-6


# ------------------------------------------------------------------ 4. free-running
@pytest.mark.parametrize("name", list(ICP_CASES))
def test_free_running(gpu, name):
    c = R.plane_case(name)
    ref, dev = c["free"], _teacher_forced(gpu, name)["dev"]
    d = box_displacement(dev["T"][0], ref["T"])
    print(name, "MEASURED_PLANE_FREE candidate [m]", d, "iterations", int(dev["iterations"][0]), ref["iterations"], "fitness",
          dev["fitness"][0], ref["fitness"], "rmse", dev["inlier_rmse"][0], ref["rmse"])
    assert 10.0 * MEASURED_PLANE_FREE <= FREE_TOL <= 1e-3 and 10.0 * d <= FREE_TOL
    assert not any(ref["near_stop"]) and int(dev["iterations"][0]) == ref["iterations"] and int(dev["status"][0]) == ref["status"]
    assert abs(dev["inlier_rmse"][0] - ref["rmse"]) <= 1e-9
    r0, t0 = pose_error(c["T_init"], c["T_planted"])
    r1, t1 = pose_error(dev["T"][0], c["T_planted"])
    assert r1 < r0 and t1 < t0
    point = gpu.icp_pairs(_cu(c["src"]), _cu(_offsets([c["src"]])), _cu(c["tgt"]), _cu(_offsets([c["tgt"]])), _cu(c["T_init"][None]))
    assert int(point["status"][0]) == 0 and int(dev["iterations"][0]) <= int(point["iterations"][0])


# ------------------------------------------------------------------ 5. edges
def test_edges(gpu):
    c = icp_case("scan_8k")
    src, tgt, T0 = c["src"], c["tgt"], c["T_init"]
    nrm = _case_normals(gpu)["scan_8k"]["normals"]
    # every normal exactly (0,0,1): columns 2-4 of A are exactly zero
    flat = np.tile([0.0, 0.0, 1.0], (len(tgt), 1))
    r = _plane(gpu, [src], [tgt], [flat], T0[None])
    assert r["status"][0] == R.ICP_SINGULAR and r["iterations"][0] == 0 and np.array_equal(r["T"][0], T0)
    full = _teacher_forced(gpu, "scan_8k")["dev"]                      # the same first evaluation, then stopped
    assert np.array_equal(r["eval_trace"][0, 0, :2], full["eval_trace"][0, 0, :2]) and r["eval_trace"][0, 0, 2] == 1.0
    assert abs(r["inlier_rmse"][0] - evaluate_f64(src, tgt, T0, MAX_DIST)["rmse"]) <= 1e-9 and not r["T_trace"][0, 1:].any()
    # five correspondences are one too few; six run
    near = tgt[:6] + 0.01
    five = _plane(gpu, [near[:5]], [tgt], [nrm], None)
    assert five["status"][0] == ICP_FEW_CORR and five["iterations"][0] == 0 and five["fitness"][0] == 1.0 and \
        np.array_equal(five["T"][0], np.eye(4))
    assert not _plane(gpu, [near], [tgt], [nrm], None, max_iteration=1)["status"][0] & ICP_FEW_CORR
    # an empty side, next to a pair that runs
    e = np.zeros((0, 3))
    r = _plane(gpu, [src, e, src, e], [tgt, tgt, e, e], [nrm, nrm, e, e], np.stack([T0] * 4))
    assert r["status"].tolist()[1:] == [ICP_EMPTY] * 3 and r["status"][0] == 0
    for p in (1, 2, 3):
        assert np.array_equal(r["T"][p], T0) and r["fitness"][p] == 0.0 and r["iterations"][p] == 0
    assert np.array_equal(r["T"][0], full["T"][0])
    # max_iteration = 0 evaluates only
    z = _plane(gpu, [src], [tgt], [nrm], T0[None], max_iteration=0)
    assert np.array_equal(z["T"][0], T0) and z["iterations"][0] == 0 and z["status"][0] == ICP_MAX_ITER
    assert z["T_trace"].shape == (1, 1, 4, 4) and z["eval_trace"][0, 0, 0] == full["eval_trace"][0, 0, 0]
    # offsets beyond the capacities are clipped, as in the point-to-point call
    so, to = _offsets([src]), _offsets([tgt])
    so[-1] += 100
    to[-1] += 100
    out = gpu.icp_pairs(_cu(src), _cu(so), _cu(tgt), _cu(to), _cu(T0[None]), MAX_DIST, 200, True, _cu(nrm))
    torch.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(_np(out[k]), full[k]), k


# ------------------------------------------------------------------ 6. invariances
def test_runs_and_batches_are_bitwise_equal(gpu):
    names = [SMALL[i % len(SMALL)] for i in range(16)]
    cs = [icp_case(n) for n in names]
    srcs, tgts, T0 = [c["src"] for c in cs], [c["tgt"] for c in cs], np.stack([c["T_init"] for c in cs])
    na, nb = _normals(gpu, tgts), _normals(gpu, tgts)
    for k in ("normals", "neighbors", "eigenvalues"):
        assert all(np.array_equal(x, y) for x, y in zip(na[k], nb[k])), k
    a = _plane(gpu, srcs, tgts, na["normals"], T0)
    b = _plane(gpu, srcs, tgts, na["normals"], T0)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    for pos in (0, 7, 15):
        alone = _normals(gpu, tgts[pos:pos + 1])
        for k in ("normals", "neighbors", "eigenvalues"):
            assert np.array_equal(alone[k][0], na[k][pos]), (k, pos)
        assert np.array_equal(alone["normals"][0], _case_normals(gpu)[names[pos]]["normals"])
        one = _plane(gpu, srcs[pos:pos + 1], tgts[pos:pos + 1], alone["normals"], T0[pos:pos + 1])
        for k in KEYS:
            assert np.array_equal(one[k][0], a[k][pos]), (k, pos)
        assert np.array_equal(one["corr"][0], a["corr"][pos])
    assert names[0] == names[5]
    for k in KEYS:
        assert np.array_equal(a[k][0], a[k][5]), k
    assert np.array_equal(_teacher_forced(gpu, names[0])["dev"]["T"][0], a["T"][0])


def test_edge_sizes_in_one_batch_equal_the_pair_alone(gpu):
    """the pairs of tests/test_gpu_icp.py:edge_batch (300, 0, 256, 257 and 1 source points) with the plane estimator"""
    from tests.test_gpu_icp import edge_batch
    srcs, tgts, T0 = edge_batch()
    nrm = _normals(gpu, tgts[:1])["normals"] * len(tgts)
    a = _plane(gpu, srcs, tgts, nrm, T0)
    print("edge batch: iterations", a["iterations"].tolist(), "status", a["status"].tolist())
    assert a["status"][1] == ICP_EMPTY and a["status"][4] == ICP_FEW_CORR and (a["iterations"][[0, 2, 3]] >= 1).all()
    for pos in range(len(srcs)):                                       # each alone is also the single-pair batch
        one = _plane(gpu, srcs[pos:pos + 1], tgts[pos:pos + 1], nrm[pos:pos + 1], T0[pos:pos + 1])
        for k in KEYS:
            assert np.array_equal(one[k][0], a[k][pos]), (k, pos)
        assert np.array_equal(one["corr"][0], a["corr"][pos]), pos


def test_graph_replay_equals_eager(gpu):
    cs = [icp_case(n) for n in SMALL[:3]]
    srcs, tgts, T0 = [c["src"] for c in cs], [c["tgt"] for c in cs], np.stack([c["T_init"] for c in cs])
    s, so, t, to, ti = _cu(_cat(srcs)), _cu(_offsets(srcs)), _cu(_cat(tgts)), _cu(_offsets(tgts)), _cu(T0)

    def run():
        n = gpu.estimate_normals(t, to, KNN, True)
        return n, gpu.icp_pairs(s, so, t, to, ti, MAX_DIST, 20, True, n["normals"])
    n0, r0 = run()                                                     # eager, and the warm-up outside the capture
    torch.cuda.synchronize()
    eager = {k: _np(r0[k]) for k in KEYS + ("corr",)}
    eager_n = {k: _np(n0[k]) for k in ("normals", "neighbors", "eigenvalues", "status")}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        n1, r1 = run()
    for k in KEYS:
        r1[k].zero_()
    n1["normals"].zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in eager_n:
        assert np.array_equal(_np(n1[k]), eager_n[k]), k
    for k in eager:
        assert np.array_equal(_np(r1[k]), eager[k]), k


# ------------------------------------------------------------------ 7. wrappers
def test_single_pair_wrapper_is_refine_pairs(gpu):
    c = icp_case("scan_8k")
    T, fit, rmse = gpu.icp_point_to_plane(c["raw_src"], c["raw_tgt"], c["T_init"])
    r = gpu.refine_pairs([c["raw_src"]], [c["raw_tgt"]], torch.from_numpy(c["T_init"][None]), point2plane=True)
    assert T.shape == (4, 4) and T.dtype == np.float64 and isinstance(fit, float) and isinstance(rmse, float)
    assert np.array_equal(T, _np(r["T"][0])) and fit == float(r["fitness"][0]) and rmse == float(r["inlier_rmse"][0])
    assert int(r["status"][0]) == 0
    dev = _teacher_forced(gpu, "scan_8k")["dev"]                       # the device's downsample differs by the means' rounding
    assert box_displacement(T, dev["T"][0]) <= FREE_TOL
    point = gpu.refine_pairs([c["raw_src"]], [c["raw_tgt"]], torch.from_numpy(c["T_init"][None]))
    assert int(r["iterations"][0]) <= int(point["iterations"][0]) and not np.array_equal(_np(point["T"]), _np(r["T"]))
    with pytest.raises(NotImplementedError, match="icp_point_to_plane"):
        gpu.icp(c["raw_src"], c["raw_tgt"], point2plane=True)


def test_evaluate_local_with_the_plane_estimator(gpu):
    from egonn_amd.synth import planted_scan_pair
    from tests.test_registration_host import planted_case
    pairs = planted_case("n128_out30")[:2]
    q = [{"keypoints": torch.from_numpy(p[2]), "features": torch.from_numpy(p[0])} for p in pairs]
    m = [{"keypoints": torch.from_numpy(p[3]), "features": torch.from_numpy(p[1])} for p in pairs]
    gt = np.stack([p[4] for p in pairs])
    qc, mc = [], []
    for i, T in enumerate(gt):
        Rm = T[:3, :3]
        ypr = (np.arctan2(Rm[1, 0], Rm[0, 0]), -np.arcsin(Rm[2, 0]), np.arctan2(Rm[2, 1], Rm[2, 2]))
        s, t, _, _ = planted_scan_pair(40 + i, 6000, translation=T[:3, 3], yaw_pitch_roll=ypr)
        qc.append(s)
        mc.append(t)
    nn = np.arange(2)[:, None]
    crop = (-80, 80, -80, 80, -30.0, None)
    kw = dict(n_k=(128,), ransac_max_it=2000, query_clouds=qc, map_clouds=mc, crop=crop)
    plane = gpu.evaluate_local(q, m, nn, gt, icp_point2plane=True, **kw)[128]
    point = gpu.evaluate_local(q, m, nn, gt, **kw)[128]
    new = {'rre_refined', 'rte_refined', 'success_refined', 'success_inliers_refined', 'failure_inliers_refined'}
    assert new <= set(plane) and set(plane) == set(point)
    for k in ('rre', 'rte', 'repeatability', 'success', 'success_inliers', 'failure_inliers'):
        assert plane[k] == point[k], k                                 # the estimator touches the refined family only
    ref = gpu.refine_pairs(qc, mc, torch.from_numpy(gt), crop, point2plane=True)
    assert (_np(ref["status"]) == 0).all() and max(box_displacement(_np(ref["T"])[i], gt[i]) for i in range(2)) < 1.0


def test_training_tuples_with_the_plane_estimator(gpu):
    from egonn_amd import CloudBank, generate_training_tuples
    from tests import tuples_data as D
    from tests.test_gpu_tuples import NEG_TH, POS_TH
    raws, planted, gps = D.planted_sequence()
    bank = CloudBank().add(raws)
    runs = {n: generate_training_tuples(gps, bank, POS_TH, NEG_TH, pairs_per_call=n, negate_translation=False, point2plane=True)
            for n in (16, 1, 5)}
    tuples, stats = runs[16]
    start, _ = generate_training_tuples(gps, None, POS_TH, NEG_TH, refine=False, negate_translation=False)
    # the scans overlap: no pair may end EMPTY, FEW_CORR or SINGULAR.  (The round limit is a legitimate end: nothing makes the
    # stop rule's 1e-6 fire within 200 rounds when a handful of correspondences keep flipping.)
    assert stats["pairs"] >= 10 and set(stats["status_counts"]) <= {0, ICP_MAX_ITER}
    for a in tuples:
        for b, T in tuples[a].positives_poses.items():
            truth = np.linalg.inv(planted[b]) @ planted[a]
            assert np.linalg.norm(T - truth) < np.linalg.norm(start[a].positives_poses[b] - truth), (a, b)
            for n in (1, 5):
                assert np.array_equal(runs[n][0][a].positives_poses[b], T), (a, b, n)
    for n in (1, 5):
        for k in ("fitness_per_pair", "inlier_rmse_per_pair", "status_per_pair"):
            assert np.array_equal(runs[n][1][k], stats[k]), (k, n)
    plain, _ = generate_training_tuples(gps, bank, POS_TH, NEG_TH, negate_translation=False)
    assert any(not np.array_equal(plain[a].positives_poses[b], T) for a in tuples for b, T in tuples[a].positives_poses.items())
