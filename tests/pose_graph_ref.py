"""float64 numpy restatement of the pose-graph layer, written from the stated problem and nothing else.
It shares no code with egonn_amd/pose_graph.py or csrc/pose_graph.hip and holds no analytic Jacobian: every derivative here is
a central difference of the residual through the retraction (h = 1e-5).  tests/test_pose_graph_host.py checks it on hand-made
graphs with written-out numbers, tests/test_gpu_pose_graph.py holds the device to it.

Problem: poses X_i = [R_i | t_i]; edge e = (a, b, Z, (w_rot, w_trans)) measures Z ~ X_a^-1 X_b; E = Z^-1 X_a^-1 X_b;
r = [t_E ; Log R_E]; s = sqrt(w_trans |t_E|^2 + w_rot |Log R_E|^2); rho = 1, or min(1, delta / s) with delta > 0 (the IRLS
weight of the Huber kernel); cost = sum of s^2 / 2 where s <= delta (or delta = 0) and delta s - delta^2 / 2 beyond, which is
rho (1 - rho / 2) s^2 in both cases and whose gradient is sum J^T rho W r.  Retraction: R <- R Exp(w), t <- t + R v with delta_i = (v, w).
"""
import numpy as np

BAD_INDEX, SELF_LOOP, NONFINITE, NEGATIVE_WEIGHT, ANGLE, ISOLATED, PIVOT = 1, 2, 4, 8, 16, 32, 64
MAX_ANGLE = np.pi - 1e-3
H_FD = 1e-5


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_so3(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = hat(w)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + (np.sin(th) / th) * K + (2.0 * np.sin(0.5 * th) ** 2 / th ** 2) * K @ K


def log_so3(R):
    """rotation vector of R, angle in [0, pi): atan2 of the axial vector's length and the trace"""
    ax = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(ax), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    if s < 1e-6:
        return ax * (1.0 + th * th / 6.0) if c > 0 else ax * (th / max(s, 1e-300))
    return ax * (th / s)


def retract(poses, delta):
    out = np.array(poses, np.float64, copy=True)
    for i, d in enumerate(np.asarray(delta, np.float64).reshape(-1, 6)):
        if not d.any():
            continue
        R = out[i, :3, :3]
        out[i, :3, 3] = out[i, :3, 3] + R @ d[:3]
        out[i, :3, :3] = R @ exp_so3(d[3:])
    return out


def edge_checks(n, edge_index, Z, weights):
    """plan status of every edge and the weights with the dead edges switched off"""
    ei = np.asarray(edge_index, np.int64).reshape(-1, 2)
    E = len(ei)
    Z = np.asarray(Z, np.float64).reshape(E, 4, 4)
    w = np.ones((E, 2)) if weights is None else np.array(weights, np.float64).reshape(E, 2)
    st = np.zeros(E, np.int32)
    st[((ei < 0) | (ei >= n)).any(axis=1)] |= BAD_INDEX
    st[(ei[:, 0] == ei[:, 1]) & (st == 0)] |= SELF_LOOP
    bad = ~np.isfinite(Z).all(axis=(1, 2)) | ~np.isfinite(w).all(axis=1) | (Z[:, 3] != np.array([0.0, 0.0, 0.0, 1.0])).any(axis=1)
    st[bad] |= NONFINITE
    with np.errstate(invalid="ignore"):
        st[(w < 0).any(axis=1)] |= NEGATIVE_WEIGHT
    w = np.where((st != 0)[:, None], 0.0, w)
    return ei, Z, w, st


def log_so3_rows(R):
    """log_so3 of every matrix of (m,3,3)"""
    ax = 0.5 * np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    s, c = np.linalg.norm(ax, axis=1), 0.5 * (np.trace(R, axis1=1, axis2=2) - 1.0)
    th = np.arctan2(s, c)
    k = np.where((s < 1e-6) & (c > 0), 1.0 + th * th / 6.0, th / np.maximum(s, 1e-300))
    return ax * k[:, None]


def exp_so3_rows(w):
    """exp_so3 of every row of (m,3)"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w, axis=1)
    small = th < 1e-8
    t = np.where(small, 1.0, th)
    ca, cb = np.where(small, 1.0, np.sin(t) / t), np.where(small, 0.5, 2.0 * np.sin(0.5 * t) ** 2 / t ** 2)
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    return np.eye(3) + ca[:, None, None] * K + cb[:, None, None] * (K @ K)


def retract_rows(X, d):
    """retract pose X[k] by d[k] for every k: (m,4,4), (m,6) -> (m,4,4)"""
    out = np.array(X, np.float64, copy=True)
    out[:, :3, 3] = X[:, :3, 3] + np.einsum("eij,ej->ei", X[:, :3, :3], d[:, :3])
    out[:, :3, :3] = X[:, :3, :3] @ exp_so3_rows(d[:, 3:])
    return out


def pair_residuals(Xa, Xb, Z):
    """r = [t_E ; Log R_E] of E = Z^-1 X_a^-1 X_b for every row: three (m,4,4) -> (m,6)"""
    Ra, Rb, RZ = Xa[:, :3, :3], Xb[:, :3, :3], Z[:, :3, :3]
    tM = np.einsum("eji,ej->ei", Ra, Xb[:, :3, 3] - Xa[:, :3, 3])                # the difference first: UTM offsets cancel
    RE = np.einsum("eji,ejk->eik", RZ, np.einsum("eji,ejk->eik", Ra, Rb))
    return np.concatenate([np.einsum("eji,ej->ei", RZ, tM - Z[:, :3, 3]), log_so3_rows(RE)], axis=1)


def pair_angles(Xa, Xb, Z):
    """the rotation angle of E = Z^-1 X_a^-1 X_b in [0, pi] for every row: atan2 of the axial vector's length and the trace.
    At a half turn the axial vector is 0 and Log R_E has no direction (log_so3_rows returns 0 there): the angle still is pi."""
    RE = np.einsum("eji,ejk->eik", Z[:, :3, :3], np.einsum("eji,ejk->eik", Xa[:, :3, :3], Xb[:, :3, :3]))
    ax = 0.5 * np.stack([RE[:, 2, 1] - RE[:, 1, 2], RE[:, 0, 2] - RE[:, 2, 0], RE[:, 1, 0] - RE[:, 0, 1]], axis=1)
    return np.arctan2(np.linalg.norm(ax, axis=1), 0.5 * (np.trace(RE, axis1=1, axis2=2) - 1.0))


def residuals(poses, edge_index, Z, weights=None, robust_delta=0.0, rho=None):
    """-> dict r (E,6), s (E,), rho (E,), terms (E,) = rho (1 - rho / 2) s^2, cost, status (E,), w (E,2) effective weights.
    rho given: held fixed and the terms are the quadratic 1/2 rho s^2 the linear solve sees; else recomputed here."""
    poses = np.asarray(poses, np.float64)
    ei, Z, w, st = edge_checks(len(poses), edge_index, Z, weights)
    E = len(ei)
    r, st = np.zeros((E, 6)), st.copy()
    ok = np.flatnonzero(st == 0)
    r[ok] = pair_residuals(poses[ei[ok, 0]], poses[ei[ok, 1]], Z[ok])
    far = ok[(np.linalg.norm(r[ok, 3:], axis=1) > MAX_ANGLE) | (pair_angles(poses[ei[ok, 0]], poses[ei[ok, 1]], Z[ok]) > MAX_ANGLE)]
    st[far] |= ANGLE
    w[far] = 0.0
    s = np.sqrt(w[:, 1] * (r[:, :3] ** 2).sum(axis=1) + w[:, 0] * (r[:, 3:] ** 2).sum(axis=1))
    if rho is None:
        rho = np.ones(E)
        if robust_delta > 0:
            big = s > robust_delta
            rho[big] = robust_delta / s[big]
        terms = rho * (1.0 - 0.5 * rho) * s * s
    else:
        terms = 0.5 * rho * s * s
    return {"r": r, "s": s, "rho": rho, "terms": terms, "cost": float(terms.sum()), "status": st, "w": w, "edges": ei}


def cost(poses, edge_index, Z, weights=None, robust_delta=0.0, rho=None):
    return residuals(poses, edge_index, Z, weights, robust_delta, rho)["cost"]


def jacobian(poses, edge_index, Z, weights=None):
    """dense (6E, 6n) Jacobian of the stacked residuals by central differences through the retraction (a residual depends on
    its two poses only, so each side of every edge is perturbed in turn); rows of dead edges are 0"""
    poses = np.asarray(poses, np.float64)
    n = len(poses)
    base = residuals(poses, edge_index, Z, weights)
    ei, E = base["edges"], len(base["edges"])
    Zs = np.asarray(Z, np.float64).reshape(E, 4, 4)
    J = np.zeros((6 * E, 6 * n))
    live = np.flatnonzero((base["w"] > 0).any(axis=1))
    Xa, Xb, Zl = poses[ei[live, 0]], poses[ei[live, 1]], Zs[live]
    rows = 6 * live[:, None] + np.arange(6)[None, :]
    for side in (0, 1):
        for c in range(6):
            d = np.zeros((len(live), 6))
            d[:, c] = H_FD
            if side == 0:
                diff = pair_residuals(retract_rows(Xa, d), Xb, Zl) - pair_residuals(retract_rows(Xa, -d), Xb, Zl)
            else:
                diff = pair_residuals(Xa, retract_rows(Xb, d), Zl) - pair_residuals(Xa, retract_rows(Xb, -d), Zl)
            J[rows, (6 * ei[live, side] + c)[:, None]] = diff / (2 * H_FD)
    return J


def weight_vector(res):
    """(6E,) diagonal of W: rho * (w_trans x3, w_rot x3)"""
    w, rho = res["w"], res["rho"]
    return (rho[:, None] * np.concatenate([np.repeat(w[:, 1:2], 3, 1), np.repeat(w[:, 0:1], 3, 1)], axis=1)).reshape(-1)


def normal_equations(poses, edge_index, Z, weights=None, robust_delta=0.0, fixed=None):
    """-> (H = J^T W J (6n, 6n), g = J^T W r (6n,), res).  Rows and columns of fixed nodes are zeroed."""
    res = residuals(poses, edge_index, Z, weights, robust_delta)
    J = jacobian(poses, edge_index, Z, res["w"])
    W = weight_vector(res)
    H = J.T @ (W[:, None] * J)
    g = J.T @ (W * res["r"].reshape(-1))
    if fixed is not None:
        m = np.repeat(np.asarray(fixed, bool), 6)
        H[m, :] = 0.0
        H[:, m] = 0.0
        g[m] = 0.0
    return H, g, res


def default_fixed(n, fixed=None):
    if fixed is None:
        f = np.zeros(n, bool)
        f[0] = True
        return f
    return np.asarray(fixed).astype(bool)


def optimize(poses, edge_index, Z, weights=None, fixed=None, max_iterations=20, robust_delta=0.0, lambda_init=1e-4,
             lambda_min=1e-10, lambda_max=1e10, rel_tol=0.0, grad_tol=0.0):
    """Levenberg-Marquardt with the device's accept / reject / stop rules and a dense solve of (H + lambda I) d = -g on the free
    nodes.  -> dict poses, cost_trace (max_iterations + 1, NaN after the stop), accept_trace, iterations, accepted, lambda."""
    X = np.array(poses, np.float64, copy=True)
    n = len(X)
    fx = default_fixed(n, fixed)
    free = np.repeat(~fx, 6)
    lam = float(lambda_init)
    trace = np.full(max_iterations + 1, np.nan)
    acc_trace = np.full(max_iterations, -1, np.int32)
    c = cost(X, edge_index, Z, weights, robust_delta)
    trace[0] = c
    its = acc = 0
    for k in range(max_iterations):
        H, g, _ = normal_equations(X, edge_index, Z, weights, robust_delta, fx)
        gmax = float(np.abs(g).max(initial=0.0))
        d = np.zeros(6 * n)
        A = H[np.ix_(free, free)] + lam * np.eye(int(free.sum()))
        d[free] = np.linalg.solve(A, -g[free])
        dead = ~np.abs(np.where(free, g, 0.0)).reshape(n, 6).any(axis=1) & ~np.abs(H).reshape(n, 6, 6 * n).any(axis=(1, 2))
        d.reshape(n, 6)[dead] = 0.0                               # a node with no live edge does not move
        Xc = retract(X, d.reshape(n, 6))
        cc = cost(Xc, edge_index, Z, weights, robust_delta)
        its += 1
        done = False
        if cc < c:
            done = (c - cc) < rel_tol * c
            X, c = Xc, cc
            lam = max(lam / 10.0, lambda_min)
            acc += 1
            acc_trace[k] = 1
        else:
            lam *= 10.0
            acc_trace[k] = 0
        trace[k + 1] = c
        if done or lam > lambda_max or gmax <= grad_tol:
            break
    return {"poses": X, "cost_trace": trace, "accept_trace": acc_trace, "iterations": its, "accepted": acc, "lambda": lam}
