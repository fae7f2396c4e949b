"""Float64 numpy restatement of egonn_spectral_verify (include/egonn_hip.h), independent of the device's Horn / Jacobi fit:
the rigid fit here is Kabsch by np.linalg.svd.  Written from the formulas of the contract, steps 1 to 6:

  1. M_ij = max(0, 1 - d_ij^2 / d_thr^2), d_ij = | |p_i - p_j| - |q_i - q_j| |, M_ii = 0
  2. v = 1 / sqrt(m); `iterations` times u = M v, stop if |u| = 0, v = u / |u|; eigenvalue = v^T M v
  3. score = eigenvalue / (n_max - 1)
  4. seeds S = { i : v_i >= seed_ratio * max v }
  5. T0 = rigid fit of S, I = { i : |T0 p_i - q_i| < dist_th }, T = rigid fit of I, then the final evaluation of
     egonn_registration_finish under T (tests/test_registration_host.py: final_eval, metrics_f64, repeatability_f64)
  6. m < 3: FEW_CORR; M = 0, |S| < 3, |I| < 3 or a degenerate fit: NO_MODEL; both: T = identity, 0 inliers

and it reports, per pair, how close each decision came to its threshold, so that a test can tell a real difference from a
tie: `residual_margin` = the smallest | residual - dist_th | over the residuals of step 5 (the correspondences under T0 and
the nearest-neighbour distances of the final evaluation under T), `seed_margin` = the smallest | v_i - seed_ratio * max v |.
"""
import numpy as np

from tests.test_registration_host import (STATUS_BAD_INDEX, STATUS_CLIPPED, STATUS_FEW_CORR, STATUS_NO_MODEL, final_eval,
                                          metrics_f64, repeatability_f64)

D_THR, ITERATIONS, SEED_RATIO, DIST_TH = 0.6, 32, 0.5, 0.5
DEGEN = 1e-10


def consistency_matrix(p, q, d_thr=D_THR):
    """(m,3) x 2 float64 -> (m,m) float64"""
    m = len(p)
    if m == 0:
        return np.zeros((0, 0))
    dp, dq = p[:, None, :] - p[None, :, :], q[:, None, :] - q[None, :, :]
    lp = np.sqrt((dp[..., 0] * dp[..., 0] + dp[..., 1] * dp[..., 1]) + dp[..., 2] * dp[..., 2])
    lq = np.sqrt((dq[..., 0] * dq[..., 0] + dq[..., 1] * dq[..., 1]) + dq[..., 2] * dq[..., 2])
    d = lp - lq
    M = np.maximum(0.0, 1.0 - (d * d) / (d_thr * d_thr))
    M[np.arange(m), np.arange(m)] = 0.0
    return M


def power_iteration(M, iterations=ITERATIONS):
    """-> v, eigenvalue, zero (M v = 0 was met)"""
    m = len(M)
    if m == 0:
        return np.zeros(0), 0.0, True
    v = np.full(m, 1.0 / np.sqrt(float(m)))
    for _ in range(iterations):
        u = M @ v
        n = np.sqrt(np.sum(u * u))
        if n == 0.0:
            return v, 0.0, True
        v = u / n
    return v, float(v @ (M @ v)), False


def spread(x):
    """the degeneracy rule: e2(C) > 1e-10 tr(C)^2 for the scatter matrix C of the centred points x"""
    C = x.T @ x
    tr = C[0, 0] + C[1, 1] + C[2, 2]
    e2 = (C[0, 0] * C[1, 1] - C[0, 1] ** 2) + (C[0, 0] * C[2, 2] - C[0, 2] ** 2) + (C[1, 1] * C[2, 2] - C[1, 2] ** 2)
    return bool(e2 > DEGEN * (tr * tr))


def rigid_fit(p, q):
    """least-squares R, t (no scale, det +1) with q ~ R p + t, by SVD; None when fewer than 3 points or degenerate"""
    if len(p) < 3:
        return None
    pm, qm = p.mean(0), q.mean(0)
    a, b = p - pm, q - qm
    if not (spread(a) and spread(b)):
        return None
    U, _, Vt = np.linalg.svd(a.T @ b)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, qm - R @ pm
    return T


def spectral_f64(k1, k2, corr, n_max, T_gt=None, d_thr=D_THR, iterations=ITERATIONS, seed_ratio=SEED_RATIO, dist_th=DIST_TH,
                 repeat_th=0.5, gap=False):
    """one pair: k1 (n1,3), k2 (n2,3) (only the valid rows), corr (m,2) int (only the valid rows).  -> dict with the operator's
    outputs (weights padded to n_max), the margins and, with gap, the spectral gap of M (eigvalsh: l1 - l2)."""
    a, b = np.asarray(k1, dtype=np.float64).reshape(-1, 3), np.asarray(k2, dtype=np.float64).reshape(-1, 3)
    c = np.asarray(corr, dtype=np.int64).reshape(-1, 2)
    status = 0
    if len(a) == 0 or len(b) == 0:
        status |= STATUS_CLIPPED if len(c) else 0
        c = c[:0]
    if len(c) and ((c[:, 0] < 0) | (c[:, 0] >= len(a)) | (c[:, 1] < 0) | (c[:, 1] >= len(b))).any():
        status |= STATUS_BAD_INDEX
        c = np.stack([np.clip(c[:, 0], 0, len(a) - 1), np.clip(c[:, 1], 0, len(b) - 1)], 1)
    m = len(c)
    p, q = a[c[:, 0]], b[c[:, 1]]
    M = consistency_matrix(p, q, d_thr)
    v, lam, zero = power_iteration(M, iterations)
    out = dict(M=M, eigenvalue=lam, score=lam / (n_max - 1) if n_max > 1 else 0.0, weights=np.zeros(n_max),
               residual_margin=np.inf, seed_margin=np.inf)
    out["weights"][:m] = v
    seeds = np.zeros(m, bool)
    if m:
        thr = seed_ratio * v.max()
        seeds = v >= thr
        out["seed_margin"] = float(np.abs(v - thr).min())
    out["seeds"], out["n_seeds"] = seeds, int(seeds.sum())
    T = None
    if m < 3:
        status |= STATUS_FEW_CORR
    elif not zero:
        T0 = rigid_fit(p[seeds], q[seeds])
        if T0 is not None:
            r2 = (((p @ T0[:3, :3].T + T0[:3, 3]) - q) ** 2).sum(1)
            out["residual_margin"] = float(np.abs(np.sqrt(r2) - dist_th).min())
            inl = r2 < dist_th * dist_th
            out["fit_inliers"] = inl
            T = rigid_fit(p[inl], q[inl])
    if T is None:
        status |= STATUS_NO_MODEL
        T = np.eye(4)
        k, fit, rmse, cset = 0, 0.0, 0.0, np.zeros((0, 2), np.int32)
    else:
        k, fit, rmse, cset = final_eval(a, b, T, dist_th)
        pt = a @ T[:3, :3].T + T[:3, 3]
        nn = np.sqrt(((pt[:, None, :] - b[None]) ** 2).sum(-1).min(1))
        out["residual_margin"] = min(out["residual_margin"], float(np.abs(nn - dist_th).min()))
    out.update(T=T, inliers=k, fitness=fit, inlier_rmse=rmse, correspondence_set=cset, status=status)
    if T_gt is not None:
        out["rte"], out["rre"], out["success"] = metrics_f64(T, T_gt)
        out["repeatability"] = repeatability_f64(a, b, T_gt, repeat_th)
    if gap:
        w = np.linalg.eigvalsh(M) if m >= 2 else np.zeros(2)
        out["gap"] = float(w[-1] - w[-2])
    return out


def planted_corr(n, seed, n_inliers, noise=0.05, box=60.0):
    """the inputs of the method's CPU sketch: n source keypoints uniform in +-box (z +-10), correspondence i -> i, of which
    n_inliers carry the planted pose plus N(0, noise) and the others point at unrelated uniform targets.
    -> k1, k2 (n,3) float32, corr (n,2) int32, T (4,4), inlier mask"""
    from egonn_amd.synth import rot_zyx
    rng = np.random.default_rng([seed, n, n_inliers])
    lo, hi = [-box, -box, -10.0], [box, box, 10.0]
    src = rng.uniform(lo, hi, size=(n, 3))
    T = np.eye(4)
    T[:3, :3] = rot_zyx(rng.uniform(-np.pi, np.pi), np.deg2rad(rng.uniform(-3, 3)), np.deg2rad(rng.uniform(-3, 3)))
    T[:3, 3] = rng.uniform(-10, 10, 3)
    tgt = rng.uniform(lo, hi, size=(n, 3))
    good = np.zeros(n, bool)
    good[rng.choice(n, size=n_inliers, replace=False)] = True
    tgt[good] = src[good] @ T[:3, :3].T + T[:3, 3] + noise * rng.standard_normal((n_inliers, 3))
    corr = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    return src.astype(np.float32), tgt.astype(np.float32), corr, T, good


# ------------------------------------------------------------------ the inputs the GPU tests compare against this restatement
SWEEP_M = (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 200, 256)      # correspondences; every m <= n_max is run at n_max 128 / 256
HIGH_OUTLIER = (5, 8, 13)                                           # planted inliers of 128, 20 seeds each


def sweep_pair(m, n_max, seed=0, noise=0.05):
    """n_max keypoints per side in the +-60 m box and m correspondences between distinct points, ascending in the source index
    as the matcher writes them.  Up to 4 correspondences all carry the planted pose, beyond that every second one does (the
    others point at unrelated targets), so the consistent set is unique and the power iteration converges.
    -> k1, k2 (n_max,3) float32, corr (m,2) int32, T (4,4)"""
    from egonn_amd.synth import rot_zyx
    rng = np.random.default_rng([seed, n_max, m])
    lo, hi = [-60.0, -60.0, -10.0], [60.0, 60.0, 10.0]
    src, tgt = rng.uniform(lo, hi, size=(n_max, 3)), rng.uniform(lo, hi, size=(n_max, 3))
    T = np.eye(4)
    T[:3, :3] = rot_zyx(rng.uniform(-np.pi, np.pi), np.deg2rad(rng.uniform(-3, 3)), np.deg2rad(rng.uniform(-3, 3)))
    T[:3, 3] = rng.uniform(-10, 10, 3)
    i = np.sort(rng.choice(n_max, size=m, replace=False))
    j = rng.permutation(n_max)[:m]
    good = np.ones(m, bool) if m <= 4 else (np.arange(m) % 2 == 0)
    tgt[j[good]] = src[i[good]] @ T[:3, :3].T + T[:3, 3] + noise * rng.standard_normal((int(good.sum()), 3))
    return src.astype(np.float32), tgt.astype(np.float32), np.stack([i, j], 1).astype(np.int32), T


def sweep_cases():
    """[(name, n_max, k1, k2, corr, T)] of the size sweep"""
    return [(f"m{m}_n{n_max}", n_max, *sweep_pair(m, n_max)) for n_max in (128, 256) for m in SWEEP_M if m <= n_max]


def planted_registration_cases(names=("n128_out60", "n256_n2_200")):
    """[(name, n_max, k1, k2, corr, T)] of the registration suite's planted pairs under the restated mutual matching"""
    from tests.test_registration_host import PLANTED_CASES, match_f64, planted_case
    out = []
    for name in names:
        for i, (f1, f2, k1, k2, T) in enumerate(planted_case(name)):
            out.append((f"{name}[{i}]", PLANTED_CASES[name]["n"], k1, k2, match_f64(f1, f2)[0], T))
    return out


def planted_relocalization_cases():
    """{(q, m): (k1, k2, corr, T)} for every (query, candidate) of the relocalisation suite's planted case (n_max = 64)"""
    from tests.test_registration_host import match_f64
    from tests.test_relocalize_host import PLANTED_M, planted_case
    c = planted_case()
    return {(q, int(m)): (c["q_kp"][q], c["map_kp"][m], match_f64(c["q_feat"][q], c["map_feat"][m])[0], c["T_planted"][m])
            for q in range(PLANTED_M) for m in c["nn"][q]}


def high_outlier_cases(seeds=20):
    """[(name, 128, k1, k2, corr, T, inlier mask)]: `planted_corr` for HIGH_OUTLIER x seeds"""
    return [(f"in{ni}_s{s}", 128, *planted_corr(128, s, ni)) for ni in HIGH_OUTLIER for s in range(seeds)]


_SOLVED = {}


def solved(key, make):
    """the restatement's results of a case list, computed once per process: {name: spectral_f64(..., gap=True)}"""
    if key not in _SOLVED:
        _SOLVED[key] = {c[0]: spectral_f64(c[2], c[3], c[4], c[1], c[5], gap=True) for c in make()}
    return _SOLVED[key]
