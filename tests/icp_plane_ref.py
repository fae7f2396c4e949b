"""Float64 restatement of the surface normals (egonn_estimate_normals) and the point-to-plane ICP (egonn_icp_plane_pairs),
shared by tests/test_icp_plane_host.py and tests/test_gpu_icp_plane.py.  It shares no logic with the device: the neighbour
search is brute force or scipy's cKDTree, the eigenvectors come from np.linalg.eigh (the device: cyclic Jacobi) and the
6 x 6 system is solved by np.linalg.solve (the device: LDL^T without pivoting).

Restated contract (egonn_amd/csrc/icp.hip; the reference delegates to Open3D, misc/point_clouds.py:31-62 [recall]):
  neighbours   all points of the same cloud, the query included, by (d2, index) ascending, d2 = (dx*dx + dy*dy) + dz*dz;
               the first m = min(knn, cloud size).
  covariance   mean = (sum q) / m, C = sum (q - mean)(q - mean)^T / m.
  normal       unit eigenvector of C's smallest eigenvalue, flipped so that n . p <= 0; with n . p == 0 the first non-zero
               component is positive; m < 3, a largest eigenvalue that is not > 0 or a non-finite value -> (0, 0, 1).
  round k      vs = T_k s_i, r = (vs - t_j) . n_j, J = [vs x n_j, n_j]; A = sum J J^T, b = sum J r; A x = -b;
               U = [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)]; T_k+1 = U T_k.  Evaluation, fitness, rmse and the stop rule are those
               of the point-to-point loop (tests/test_icp_host.py); before a round fewer than 6 correspondences stop the loop
               with FEW_CORR, a rank-deficient A with SINGULAR."""
import numpy as np

from tests.test_icp_host import BAND, ICP_EMPTY, ICP_FEW_CORR, evaluate_f64, icp_case, stop_rule, transform_f64

try:
    from scipy.spatial import cKDTree
except Exception:                                   # pragma: no cover
    cKDTree = None

ICP_SINGULAR = 16
NORMALS_FEW_POINTS, NORMALS_RANGE = 1, 2
BRUTE_MAX = 1024
SINGULAR_COND = 2.0 ** 40       # the restatement's reading of "rank deficient"; the committed cases sit eight decades below


def _d2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn_f64(points, knn):
    """-> (idx (n, knn) int64 in (d2, index) order, -1 beyond m = min(knn, n); gap (n,) = d2 of entry knn+1 minus d2 of entry
    knn, inf when the cloud has no entry knn+1).  Brute force in the device's operation order up to 1024 points, else
    cKDTree with k = knn + 1 and the candidates re-ordered by (d2, index): a row whose gap is within BAND may differ."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(p)
    idx = np.full((n, knn), -1, np.int64)
    gap = np.full(n, np.inf)
    if n == 0:
        return idx, gap
    k = min(knn + 1, n)
    if n <= BRUTE_MAX or cKDTree is None:
        cand = np.zeros((n, k), np.int64)
        for a in range(0, n, 256):
            d2 = _d2(p[a:a + 256, None, :], p[None])
            cand[a:a + 256] = np.argsort(d2, axis=1, kind="stable")[:, :k]       # stable: ties in ascending index
    else:
        _, cand = cKDTree(p).query(p, k=k)
        cand = np.asarray(cand).reshape(n, k)
    d2 = _d2(p[:, None, :], p[cand])
    order = np.lexsort((cand, d2), axis=1)                                       # by d2, then by index
    cand, d2 = np.take_along_axis(cand, order, 1), np.take_along_axis(d2, order, 1)
    m = min(knn, n)
    idx[:, :m] = cand[:, :m]
    if k > knn:
        gap = d2[:, knn] - d2[:, knn - 1]
    return idx, gap


def covariance_f64(points, idx):
    """-> (C (n,3,3), m (n,)) of the neighbour lists idx (n, knn), -1 = absent"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    w = (idx >= 0)[..., None].astype(np.float64)
    q = p[np.maximum(idx, 0)]
    m = np.maximum((idx >= 0).sum(1), 1).astype(np.float64)
    mean = (q * w).sum(1) / m[:, None]
    d = (q - mean[:, None, :]) * w
    return np.einsum("nka,nkb->nab", d, d) / m[:, None, None], (idx >= 0).sum(1)


def normals_f64(points, idx):
    """-> (normals (n,3), eigenvalues (n,3) ascending, C (n,3,3))"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    C, m = covariance_f64(p, idx)
    lam, vec = np.linalg.eigh(C)
    nrm = vec[:, :, 0].copy()
    dot = (nrm * p).sum(1)
    lead = np.where(nrm[:, 0] != 0, nrm[:, 0], np.where(nrm[:, 1] != 0, nrm[:, 1], nrm[:, 2]))
    flip = (dot > 0) | ((dot == 0) & (lead < 0))
    nrm[flip] *= -1.0
    bad = (m < 3) | ~(lam[:, 2] > 0) | ~np.isfinite(nrm).all(1)
    nrm[bad] = (0.0, 0.0, 1.0)
    return nrm, lam, C


def vec6_to_T(x):
    """(x0..x5) -> [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)] as a 4 x 4 pose"""
    a, b, c = float(x[0]), float(x[1]), float(x[2])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    U = np.eye(4)
    U[:3, :3], U[:3, 3] = Rz @ Ry @ Rx, x[3:6]
    return U


def plane_system_f64(src, tgt, normals, T, j):
    """-> (A (6,6), b (6,)) of the correspondences j (n,) (-1 = none) under T"""
    rows = np.nonzero(j >= 0)[0]
    vs = transform_f64(T, np.asarray(src, np.float64)[rows])
    t, n = np.asarray(tgt, np.float64)[j[rows]], np.asarray(normals, np.float64)[j[rows]]
    r = ((vs - t) * n).sum(1)
    J = np.concatenate([np.cross(vs, n), n], 1)
    return J.T @ J, J.T @ r


def plane_step_f64(src, tgt, normals, T, j):
    """-> (T_k+1 = U T_k or None when the system is rank deficient, cond(A))"""
    A, b = plane_system_f64(src, tgt, normals, T, j)
    if not np.isfinite(A).all():
        return None, np.inf
    cond = float(np.linalg.cond(A))
    if not cond < SINGULAR_COND:
        return None, cond
    x = np.linalg.solve(A, -b)
    if not np.isfinite(x).all():
        return None, cond
    return vec6_to_T(x) @ T, cond


def icp_plane_f64(src, tgt, normals, T_init=None, max_dist=1.2, max_iteration=200):
    """the free-running loop -> dict: T, fitness, rmse, iterations, status, near_rows, near_stop, trace, conds"""
    T = np.eye(4) if T_init is None else np.array(T_init, dtype=np.float64)
    out = dict(near_rows=[], near_stop=[], trace=[T], conds=[])
    if len(src) == 0 or len(tgt) == 0:
        return dict(out, T=T, fitness=0.0, rmse=0.0, iterations=0, status=ICP_EMPTY)
    prev = None
    for k in range(max_iteration + 1):
        ev = evaluate_f64(src, tgt, T, max_dist)
        out["near_rows"].append(float(((ev["gap"] <= BAND) | (ev["thr"] <= BAND)).mean()))
        stop, bit, near = plane_stop_rule(k, ev, prev, max_iteration)
        out["near_stop"].append(near)
        T_next = None
        if not stop:
            T_next, cond = plane_step_f64(src, tgt, normals, T, ev["j"])
            out["conds"].append(cond)
            if T_next is None:
                stop, bit = True, ICP_SINGULAR
        if stop:
            return dict(out, T=T, fitness=ev["fitness"], rmse=ev["rmse"], iterations=k, status=bit)
        T = T_next
        out["trace"].append(T)
        prev = ev
    raise AssertionError("unreachable")


def plane_stop_rule(k, ev, prev, max_iteration):
    """`stop_rule` with the plane estimator's correspondence minimum: 6 instead of 3"""
    stop, bit, near = stop_rule(k, ev, prev, max_iteration)
    if not stop and ev["n_corr"] < 6:
        return True, ICP_FEW_CORR, near
    return stop, bit, near


_CACHE = {}


def plane_case(name):
    """icp_case(name) plus, computed once: knn (idx, gap) of the target at knn = 20, its restatement normals / eigenvalues and
    the free-running restatement result"""
    if name not in _CACHE:
        c = dict(icp_case(name))
        c["idx"], c["gap"] = knn_f64(c["tgt"], 20)
        c["normals"], c["lam"], _ = normals_f64(c["tgt"], c["idx"])
        c["free"] = icp_plane_f64(c["src"], c["tgt"], c["normals"], c["T_init"], 1.2, c["max_iteration"])
        _CACHE[name] = c
    return _CACHE[name]
