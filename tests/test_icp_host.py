"""CPU tests of the ICP refinement (egonn_voxel_downsample / egonn_icp_pairs) and the home of its float64 restatement, which
tests/test_gpu_icp.py imports.

Restated contract (egonn_amd/csrc/icp.hip; the reference delegates to Open3D, misc/point_clouds.py:31-62 [recall]):
  downsample   optional crop (x > min, x <= max per axis, NaN / None = no bound); mb = min over the kept points - voxel/2;
               idx = floor((p - mb) / voxel); one point per occupied voxel = mean of its points summed in input order; output
               in ascending (ix, iy, iz); an index beyond 21 bits -> RANGE, nothing written.
  evaluation   under T: j(i) = nearest target of T s_i by squared distance, ties lowest index; correspondence iff
               d2 < max_dist^2; fitness = n_corr / n_source; rmse = sqrt(sum d2 / n_corr) (0 without correspondences).
  loop         T_0 = init (evaluated).  After evaluation k: stop if k >= 1 and |d fitness| < 1e-6 and |d rmse| < 1e-6; else
               stop with MAX_ITER if k == max_iteration; else stop with FEW_CORR if n_corr < 3; else U = Kabsch of
               {T_k s_i} onto {t_j(i)} (np.linalg.svd, reflection corrected), T_k+1 = U T_k.  iterations = k at the stop.
The neighbour search here is scipy's cKDTree (k = 2) when scipy imports, else chunked brute force: float64 distances, no
cell logic shared with the device.  The device solves the rotation by Horn's quaternion form with a Jacobi eigen-solver;
the SVD here is an independent route to the same least-squares rotation."""
import os
import re

import numpy as np
import pytest
import torch

from egonn_amd.synth import planted_scan_pair, rot_zyx

try:
    from scipy.spatial import cKDTree
except Exception:                                   # pragma: no cover
    cKDTree = None

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ICP_FEW_CORR, ICP_MAX_ITER, ICP_EMPTY, ICP_RANGE = 1, 2, 4, 8
EPS_STOP = 1e-6
NEW_SYMBOLS = ["egonn_voxel_downsample", "egonn_voxel_downsample_scratch_bytes", "egonn_icp_pairs", "egonn_icp_scratch_bytes"]

# A row is "near a decision" when the gap between its nearest and second-nearest squared distance (m^2), or the distance of
# its nearest neighbour to max_dist (m), is within BAND; a stop decision is near when ||delta| - 1e-6| is within BAND.  The
# issue asks for BAND >= 100 x the largest device-vs-restatement difference of transformed coordinates (measured in
# tests/test_gpu_icp.py and recorded there as MEASURED_COORD_DIFF) and BAND <= 1e-6 m.
BAND = 1e-8
NEAR_ROW_CAP = 1e-3          # share of a round's rows that may be near a decision (the cap of the GPU test)
BOX = 114.0                  # the +-114 m box whose points measure a difference of two transforms

# planted_scan_pair arguments; `max_iteration` is the round limit of the case
ICP_CASES = {
    "scan_50k": dict(seed=11, n_points=50000),
    "scan_8k": dict(seed=12, n_points=8000, translation=(-2.0, 1.0, 0.0), yaw_pitch_roll=(-0.1, 0.0, 0.02)),
    "src_6k_tgt_9k": dict(seed=13, n_points=(6000, 9000)),
    "src_10k_tgt_5k": dict(seed=14, n_points=(10000, 5000), translation=(0.0, 3.0, -0.1), yaw_pitch_roll=(0.3, 0.02, 0.0)),
    "far_init_7k": dict(seed=15, n_points=7000, init_translation=(0.9, 0.6, 0.2), init_yaw_pitch_roll=(0.04, 0.01, 0.0)),
    "converged_init_5k": dict(seed=16, n_points=5000, init_translation=(0.02, 0.01, 0.005), init_yaw_pitch_roll=(0.001, 0.0, 0.0)),
}
MAX_ITERATION = 200


# ------------------------------------------------------------------ restatement
def crop_mask(p, crop):
    keep = np.ones(len(p), bool)
    if crop is not None:
        for ax in range(3):
            lo, hi = crop[2 * ax], crop[2 * ax + 1]
            if lo is not None and not np.isnan(lo):
                keep &= p[:, ax] > lo
            if hi is not None and not np.isnan(hi):
                keep &= p[:, ax] <= hi
    return keep


def downsample_f64(points, voxel_size=0.1, crop=None):
    """-> (points (m,3) f64 in ascending voxel index, counts (m,) int, voxel index (m,3) int64, status)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    p = p[crop_mask(p, crop)]
    empty = (np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros((0, 3), np.int64))
    if len(p) == 0:
        return (*empty, 0)
    mb = p.min(0) - voxel_size / 2
    f = np.floor((p - mb) / voxel_size)
    if not np.isfinite(f).all() or f.max() >= 2 ** 21:
        return (*empty, ICP_RANGE)
    idx = f.astype(np.int64)
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    uniq, first, inv, counts = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    sums = np.zeros((len(uniq), 3))
    np.add.at(sums, inv.reshape(-1), p)                # unbuffered: one addition per point, in input order
    return sums / counts[:, None], counts, idx[first], 0


def transform_f64(T, s):
    """T s row by row, in the operation order of the device: ((r0 x + r1 y) + r2 z) + t, no fused multiply-add"""
    s = np.asarray(s, dtype=np.float64)
    R, t = T[:3, :3], T[:3, 3]
    return ((s[:, 0:1] * R[:, 0] + s[:, 1:2] * R[:, 1]) + s[:, 2:3] * R[:, 2]) + t


def _two_nearest(p, tgt):
    """indices (n,2) of the two nearest targets (second = -1 with one target), by an exact float64 search"""
    n, m = len(p), len(tgt)
    k = min(2, m)
    if cKDTree is not None:
        _, j = cKDTree(tgt).query(p, k=k)
        j = np.asarray(j).reshape(n, k)
    else:
        j = np.zeros((n, k), np.int64)
        for a in range(0, n, 512):
            d2 = ((p[a:a + 512, None, :] - tgt[None]) ** 2).sum(-1)
            j[a:a + 512] = np.argsort(d2, axis=1, kind="stable")[:, :k]
    if k == 1:
        j = np.concatenate([j, np.full((n, 1), -1)], 1)
    return j


def evaluate_f64(src, tgt, T, max_dist):
    """-> dict: j (n,) nearest target or -1 where no correspondence, nn (n,) nearest target regardless of the threshold, d2 (n,),
    n_corr, sum_d2, fitness, rmse, gap (n,) second-nearest d2 minus nearest d2 (inf with one target), thr (n,) |d - max_dist|"""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    n = len(src)
    if n == 0 or len(tgt) == 0:
        z = np.zeros(n)
        return dict(j=np.full(n, -1), nn=np.full(n, -1), d2=z, n_corr=0, sum_d2=0.0, fitness=0.0, rmse=0.0, gap=z + np.inf, thr=z + np.inf)
    p = transform_f64(T, src)
    jj = _two_nearest(p, tgt)

    def sq(j):
        d = p - tgt[j]
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    d1 = sq(jj[:, 0])
    d2nd = np.where(jj[:, 1] >= 0, sq(np.maximum(jj[:, 1], 0)), np.inf)
    swap = (d2nd < d1) | ((d2nd == d1) & (jj[:, 1] >= 0) & (jj[:, 1] < jj[:, 0]))      # ties: lowest index
    nn = np.where(swap, jj[:, 1], jj[:, 0])
    lo, hi = np.minimum(d1, d2nd), np.maximum(d1, d2nd)
    ok = lo < max_dist * max_dist
    n_corr = int(ok.sum())
    sum_d2 = float(np.cumsum(lo[ok])[-1]) if n_corr else 0.0
    return dict(j=np.where(ok, nn, -1), nn=nn, d2=lo, n_corr=n_corr, sum_d2=sum_d2, fitness=n_corr / n,
                rmse=float(np.sqrt(sum_d2 / n_corr)) if n_corr else 0.0, gap=hi - lo, thr=np.abs(np.sqrt(lo) - max_dist))


def kabsch_f64(S, Q):
    """(m,3) point sets -> U (4,4) minimising sum |U s - q|^2 over rigid motions (det +1), by SVD"""
    cs, cq = S.mean(0), Q.mean(0)
    Hm = (S - cs).T @ (Q - cq)
    W, _, Vt = np.linalg.svd(Hm)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ W.T))])
    R = Vt.T @ D @ W.T
    U = np.eye(4)
    U[:3, :3], U[:3, 3] = R, cq - R @ cs
    return U


def icp_step_f64(src, tgt, T, j):
    """T_k+1 = U T_k for the correspondences j (n,) (-1 = none) of the evaluation under T_k"""
    rows = np.nonzero(j >= 0)[0]
    U = kabsch_f64(transform_f64(T, np.asarray(src, np.float64)[rows]), np.asarray(tgt, np.float64)[j[rows]])
    return U @ T


def stop_rule(k, ev, prev, max_iteration):
    """-> (stop, status bit, near): the decision after evaluation k; near = a threshold of the rule within BAND"""
    near = False
    if k >= 1:
        df, dr = abs(ev["fitness"] - prev["fitness"]), abs(ev["rmse"] - prev["rmse"])
        near = abs(df - EPS_STOP) <= BAND or abs(dr - EPS_STOP) <= BAND
        if df < EPS_STOP and dr < EPS_STOP:
            return True, 0, near
    if k >= max_iteration:
        return True, ICP_MAX_ITER, near
    if ev["n_corr"] < 3:
        return True, ICP_FEW_CORR, near
    return False, 0, near


def icp_f64(src, tgt, T_init=None, max_dist=1.2, max_iteration=200):
    """the free-running loop -> dict: T, fitness, rmse, iterations, status, near_rows (per round share of rows near a
    decision), near_stop (per round bool), trace (list of T_k)"""
    T = np.eye(4) if T_init is None else np.array(T_init, dtype=np.float64)
    out = dict(near_rows=[], near_stop=[], trace=[T])
    if len(src) == 0 or len(tgt) == 0:
        return dict(out, T=T, fitness=0.0, rmse=0.0, iterations=0, status=ICP_EMPTY)
    prev = None
    for k in range(max_iteration + 1):
        ev = evaluate_f64(src, tgt, T, max_dist)
        out["near_rows"].append(float(((ev["gap"] <= BAND) | (ev["thr"] <= BAND)).mean()))
        stop, bit, near = stop_rule(k, ev, prev, max_iteration)
        out["near_stop"].append(near)
        if stop:
            return dict(out, T=T, fitness=ev["fitness"], rmse=ev["rmse"], iterations=k, status=bit)
        T = icp_step_f64(src, tgt, T, ev["j"])
        out["trace"].append(T)
        prev = ev
    raise AssertionError("unreachable")


def box_displacement(Ta, Tb):
    """largest displacement of a corner of the +-114 m box between two transforms (the maximum over the box is at a corner)"""
    c = np.array([[x, y, z] for x in (-BOX, BOX) for y in (-BOX, BOX) for z in (-BOX, BOX)])
    d = (c @ Ta[:3, :3].T + Ta[:3, 3]) - (c @ Tb[:3, :3].T + Tb[:3, 3])
    return float(np.sqrt((d * d).sum(1)).max())


def pose_error(T, T_ref):
    """(rotation angle in degrees, translation distance) between two poses"""
    c = (np.trace(T[:3, :3].T @ T_ref[:3, :3]) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), float(np.linalg.norm(T[:3, 3] - T_ref[:3, 3]))


_CACHE = {}


def icp_case(name):
    """-> dict: src, tgt (downsampled f64), raw_src, raw_tgt (float32), T_planted, T_init, max_iteration"""
    if name not in _CACHE:
        raw_src, raw_tgt, T_planted, T_init = planted_scan_pair(**ICP_CASES[name])
        _CACHE[name] = dict(src=downsample_f64(raw_src)[0], tgt=downsample_f64(raw_tgt)[0], raw_src=raw_src, raw_tgt=raw_tgt,
                            T_planted=T_planted, T_init=T_init, max_iteration=MAX_ITERATION)
    return _CACHE[name]


def icp_case_result(name):
    c = icp_case(name)
    if "free" not in c:
        c["free"] = icp_f64(c["src"], c["tgt"], c["T_init"], 1.2, c["max_iteration"])
    return c["free"]


# ------------------------------------------------------------------ tests
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
    for bits in ("EGONN_ICP_STATUS_FEW_CORR = 1", "EGONN_ICP_STATUS_MAX_ITER = 2", "EGONN_ICP_STATUS_EMPTY = 4",
                 "EGONN_ICP_STATUS_RANGE = 8"):
        assert bits in header
    assert lib.egonn_icp_scratch_bytes(50000, 50000, 1) > 0 and lib.egonn_voxel_downsample_scratch_bytes(50000, 2) > 0
    assert lib.egonn_icp_scratch_bytes(-1, 10, 1) == -1 and lib.egonn_icp_scratch_bytes(10, 10, 0) == -1
    assert lib.egonn_voxel_downsample_scratch_bytes(1 << 31, 1) == -1 and lib.egonn_voxel_downsample_scratch_bytes(10, 0) == -1
    # a function of the capacities only, and growing with them
    assert lib.egonn_icp_scratch_bytes(50000, 50000, 16) > lib.egonn_icp_scratch_bytes(50000, 50000, 1)


def test_argument_checks_need_no_gpu(built):
    """the up-front checks return the library's invalid status before anything is launched"""
    from egonn_amd import _lib
    lib = _lib.load()
    one = 256       # non-null, aligned, never dereferenced: every call below fails its argument check first
    big = 1 << 40
    assert lib.egonn_voxel_downsample(one, 10, one, 0, 0.1, None, one, one, one, one, one, big, None) == 1
    assert b"n_clouds" in lib.egonn_last_error()
    assert lib.egonn_voxel_downsample(one, 10, one, 1, 0.0, None, one, one, one, one, one, big, None) == 1
    assert lib.egonn_voxel_downsample(one, 10, None, 1, 0.1, None, one, one, one, one, one, big, None) == 1
    assert lib.egonn_voxel_downsample(one, 10, one, 1, 0.1, None, one, one, one, one, one, 8, None) == 1
    assert b"scratch" in lib.egonn_last_error()
    args = (one, one, one, one, one, None, None, None)
    assert lib.egonn_icp_pairs(one, 10, one, one, 10, one, 0, None, 1.2, 200, 1e-6, 1e-6, *args, one, big, None) == 1
    assert lib.egonn_icp_pairs(one, 10, one, one, 10, one, 1, None, 0.0, 200, 1e-6, 1e-6, *args, one, big, None) == 1
    assert lib.egonn_icp_pairs(one, 10, one, one, 10, one, 1, None, 1.2, -1, 1e-6, 1e-6, *args, one, big, None) == 1
    assert b"max_iteration" in lib.egonn_last_error()
    assert lib.egonn_icp_pairs(one, 10, None, one, 10, one, 1, None, 1.2, 200, 1e-6, 1e-6, *args, one, big, None) == 1
    assert lib.egonn_icp_pairs(one, 10, one, one, 10, one, 1, None, 1.2, 200, 1e-6, 1e-6, *args, one, 8, None) == 1
    assert lib.egonn_icp_pairs(one, 10, one, one, 10, one, 1, None, 1.2, 200, 1e-6, 1e-6, *args, one + 8, big, None) == 1


def test_public_functions_exist_and_reject_bad_shapes():
    """shape errors are raised before a device is asked for: these pass (by raising) without a GPU"""
    import egonn_amd
    from egonn_amd import synth
    assert callable(synth.planted_scan_pair)
    for name in ("icp", "icp_pairs", "voxel_downsample"):
        assert callable(getattr(egonn_amd, name)), name
    z = np.zeros
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        egonn_amd.voxel_downsample(z((10, 2), np.float32), [0, 10])
    with pytest.raises(ValueError, match="offsets"):
        egonn_amd.voxel_downsample(z((10, 3), np.float32), [10])
    with pytest.raises(ValueError, match="crop"):
        egonn_amd.voxel_downsample(z((10, 3), np.float32), [0, 10], crop=(0, 1, 2))
    with pytest.raises(ValueError, match="voxel_size"):
        egonn_amd.voxel_downsample(z((10, 3), np.float32), [0, 10], voxel_size=0.0)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        egonn_amd.icp_pairs(z((10, 4)), [0, 10], z((10, 3)), [0, 10])
    with pytest.raises(ValueError, match="same number of pairs"):
        egonn_amd.icp_pairs(z((10, 3)), [0, 10], z((10, 3)), [0, 5, 10])
    with pytest.raises(ValueError, match="T_init"):
        egonn_amd.icp_pairs(z((10, 3)), [0, 10], z((10, 3)), [0, 10], T_init=z((2, 4, 4)))
    with pytest.raises(ValueError, match="max_iteration"):
        egonn_amd.icp_pairs(z((10, 3)), [0, 10], z((10, 3)), [0, 10], max_iteration=-1)
    with pytest.raises(NotImplementedError):
        egonn_amd.icp(z((10, 3)), z((10, 3)), point2plane=True)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        egonn_amd.icp(z((10,)), z((10, 3)))
    with pytest.raises(ValueError, match=r"\(4, 4\)"):
        egonn_amd.icp(z((10, 3)), z((10, 3)), transform=np.eye(3))
    with pytest.raises(ValueError, match="go together"):
        egonn_amd.evaluate_local([], [], [], z((0, 4, 4)), query_clouds=[])


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_icp_has_no_cpu_path(built):
    import egonn_amd
    s, t, _, T0 = planted_scan_pair(3, 500)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        egonn_amd.icp(s, t, T0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        egonn_amd.voxel_downsample(s, [0, len(s)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        egonn_amd.icp_pairs(s.astype(np.float64), [0, len(s)], t.astype(np.float64), [0, len(t)])


def test_planted_scan_pair():
    s, t, T, T0 = planted_scan_pair(5, (3000, 2000), translation=(1, 2, 3), yaw_pitch_roll=(0.1, 0.2, 0.3), noise=0.0,
                                    init_translation=(0, 0, 0), init_yaw_pitch_roll=(0, 0, 0))
    assert s.shape == (3000, 3) and t.shape == (2000, 3) and s.dtype == t.dtype == np.float32
    assert np.array_equal(T, T0) and np.allclose(T[:3, :3], rot_zyx(0.1, 0.2, 0.3)) and np.allclose(T[:3, 3], [1, 2, 3])
    # both sides are subsamples of ONE scene: without noise every moved-back target point is a point of that scene
    s2, t2, _, _ = planted_scan_pair(5, (3000, 2000), translation=(1, 2, 3), yaw_pitch_roll=(0.1, 0.2, 0.3), noise=0.0)
    assert np.array_equal(s, s2) and np.array_equal(t, t2)
    back = (t.astype(np.float64) - T[:3, 3]) @ T[:3, :3]
    ev = evaluate_f64(back, np.concatenate([s.astype(np.float64), back[:1] + 50.0]), np.eye(4), 1.2)
    assert 0.0 < (ev["d2"] < 1e-8).mean() < 1.0          # the subsamples overlap and differ
    _, _, T1, T2 = planted_scan_pair(5, 100, init_translation=(0.5, 0, 0), init_yaw_pitch_roll=(0.02, 0, 0))
    rot, tr = pose_error(T2, T1)
    assert abs(rot - np.degrees(0.02)) < 1e-9 and 0.4 < tr < 0.6


def test_downsample_restatement():
    p = np.array([[0.0, 0, 0], [0.04, 0.04, 0.04], [0.06, 0, 0], [1.0, 1.0, 1.0], [-0.3, 5, 5]], np.float32)
    q, cnt, idx, st = downsample_f64(p)
    assert st == 0 and cnt.sum() == 5 and len(q) == len(cnt) == len(idx)
    keys = [tuple(r) for r in idx]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    # mb = min - voxel/2: the minimum sits in the middle of voxel 0
    assert idx.min(0).tolist() == [0, 0, 0]
    # crop: a point exactly on min is dropped, one exactly on max is kept
    q2, cnt2, _, _ = downsample_f64(p, crop=(0.0, 1.0, None, None, float("nan"), None))
    assert cnt2.sum() == 3 and np.abs(q2 - 1.0).max(1).min() == 0.0
    assert downsample_f64(p[:0])[3] == 0 and len(downsample_f64(p[:0])[0]) == 0
    one = downsample_f64(p[3:4])
    assert np.array_equal(one[0], p[3:4].astype(np.float64)) and one[1].tolist() == [1]
    far = np.array([[0, 0, 0], [0.1 * 2 ** 21 + 1, 0, 0]], np.float32)
    assert downsample_f64(far)[3] == ICP_RANGE and len(downsample_f64(far)[0]) == 0
    # means: sequential sums in input order
    rng = np.random.default_rng(0)
    pts = rng.uniform(-5, 5, size=(4000, 3)).astype(np.float32)
    q, cnt, idx, _ = downsample_f64(pts, 0.5)
    mb = pts.astype(np.float64).min(0) - 0.25
    i0 = np.floor((pts.astype(np.float64) - mb) / 0.5).astype(np.int64)
    for r in (0, len(q) // 2, len(q) - 1):
        rows = np.nonzero((i0 == idx[r]).all(1))[0]
        acc = np.zeros(3)
        for i in rows:
            acc = acc + pts[i].astype(np.float64)
        assert len(rows) == cnt[r] and np.array_equal(acc / cnt[r], q[r])


def test_kabsch_and_search_restatement():
    rng = np.random.default_rng(1)
    S = rng.uniform(-50, 50, size=(500, 3))
    U0 = np.eye(4)
    U0[:3, :3], U0[:3, 3] = rot_zyx(0.7, -0.2, 0.1), [3.0, -2.0, 0.5]
    Q = S @ U0[:3, :3].T + U0[:3, 3]
    assert np.abs(kabsch_f64(S, Q) - U0).max() < 1e-10
    assert np.isclose(np.linalg.det(kabsch_f64(S, Q * np.array([1, 1, -1.0]))[:3, :3]), 1.0)
    # the search against plain brute force, threshold strict, ties to the lowest index
    tgt = rng.uniform(-3, 3, size=(300, 3))
    tgt[7] = tgt[3]
    src = np.concatenate([rng.uniform(-3, 3, size=(200, 3)), tgt[3:4], [[100.0, 0, 0]]])
    ev = evaluate_f64(src, tgt, np.eye(4), 0.5)
    d2 = ((src[:, None] - tgt[None]) ** 2).sum(-1)
    assert np.array_equal(ev["nn"], d2.argmin(1)) and ev["nn"][200] == 3 and ev["gap"][200] == 0.0
    assert np.array_equal(ev["j"] >= 0, d2.min(1) < 0.25) and ev["j"][201] == -1
    assert ev["n_corr"] == (d2.min(1) < 0.25).sum() and np.isclose(ev["sum_d2"], d2.min(1)[d2.min(1) < 0.25].sum())
    e1 = evaluate_f64(src, tgt[:1], np.eye(4), 0.5)
    assert np.isinf(e1["gap"]).all() and (e1["nn"] == 0).all()
    assert evaluate_f64(src[:0], tgt, np.eye(4), 0.5)["n_corr"] == 0 and evaluate_f64(src, tgt[:0], np.eye(4), 0.5)["fitness"] == 0.0


def test_loop_rules():
    rng = np.random.default_rng(2)
    tgt = rng.uniform(-10, 10, size=(400, 3))
    src = tgt[:300] + 0.01
    r = icp_f64(src, tgt, None, 1.2, 50)
    assert r["status"] == 0 and 1 <= r["iterations"] < 50 and r["fitness"] == 1.0 and r["rmse"] < 1e-9
    r0 = icp_f64(src, tgt, None, 1.2, 0)
    assert r0["iterations"] == 0 and r0["status"] == ICP_MAX_ITER and np.array_equal(r0["T"], np.eye(4)) and r0["fitness"] == 1.0
    far = icp_f64(src + 100.0, tgt, None, 1.2, 50)
    assert far["status"] == ICP_FEW_CORR and far["iterations"] == 0 and np.array_equal(far["T"], np.eye(4)) and far["fitness"] == 0.0
    assert icp_f64(src[:0], tgt, None)["status"] == ICP_EMPTY and icp_f64(src, tgt[:0], None)["status"] == ICP_EMPTY
    c = icp_case("far_init_7k")
    cut = icp_f64(c["src"], c["tgt"], c["T_init"], 1.2, 3)
    assert cut["status"] == ICP_MAX_ITER and cut["iterations"] == 3 and len(cut["trace"]) == 4


def test_case_list_covers_what_the_issue_asks():
    n = {k: v["n_points"] for k, v in ICP_CASES.items()}
    assert 50000 in n.values()
    assert sum(1 for v in n.values() if np.isscalar(v) and 5000 <= v <= 10000) >= 3
    assert sum(1 for v in n.values() if not np.isscalar(v) and v[0] != v[1]) >= 2
    assert icp_case_result("far_init_7k")["iterations"] >= 3 * icp_case_result("converged_init_5k")["iterations"]
    assert icp_case_result("far_init_7k")["iterations"] >= 15 and icp_case_result("converged_init_5k")["iterations"] <= 6


@pytest.mark.parametrize("name", list(ICP_CASES))
def test_cases_are_well_conditioned_and_refined(name):
    """the condition on the inputs that the GPU test relies on, and the point of the exercise: ICP improves the pose"""
    c, r = icp_case(name), icp_case_result(name)
    print(name, "rows", len(c["src"]), len(c["tgt"]), "rounds", r["iterations"], "status", r["status"], "fitness", r["fitness"],
          "rmse", r["rmse"], "near rows max", max(r["near_rows"]), "init err", pose_error(c["T_init"], c["T_planted"]),
          "final err", pose_error(r["T"], c["T_planted"]))
    assert 1e-6 >= BAND > 0
    assert r["status"] == 0 and r["iterations"] < c["max_iteration"]
    assert max(r["near_rows"]) <= NEAR_ROW_CAP
    assert not any(r["near_stop"])
    rot0, tr0 = pose_error(c["T_init"], c["T_planted"])
    rot1, tr1 = pose_error(r["T"], c["T_planted"])
    assert rot1 < rot0 and tr1 < tr0, (rot0, rot1, tr0, tr1)
