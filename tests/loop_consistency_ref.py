"""float64 numpy restatement of the loop-consistency filter, written from the stated contract and nothing else.
It shares no code with egonn_amd/loop_consistency.py or csrc/loop_consistency.hip.  tests/test_loop_consistency_host.py checks
it on hand-made cases with written-out answers, tests/test_gpu_loop_consistency.py holds the device to it.  Every function that
does arithmetic takes a dtype, so the same statement evaluated in numpy.longdouble is the yardstick of the float64 one.

Contract: poses X (n,4,4); edge e = (a, b, Z, (w_rot, w_trans)) with Z ~ X_a^-1 X_b.  Live: no status bit (the pose graph's
BAD_INDEX, SELF_LOOP, NONFINITE, NEGATIVE_WEIGHT; NONFINITE also for a non-finite pose at either end) and a positive weight.
Cycle: C = Z_e (X_be^-1 X_bf) Z_f^-1 (X_af^-1 X_ae), c_trans = |t_C|, c_rot = |Log R_C|, the edge that is first by (b, row) as e.
Comparable: |b_e - b_f| <= window, |a_e - a_f| <= window, at most max_partners / 2 places apart among the live edges ordered by
(b, row).  Consistent: c_trans <= trans_thr + trans_drift g, c_rot <= rot_thr + rot_drift g, g = |b_e - b_f| + |a_e - a_f|.
Selection: synchronous rounds, count the surviving consistent partners, remove all below min_support at once.
"""
import numpy as np

BAD_INDEX, SELF_LOOP, NONFINITE, NEGATIVE_WEIGHT = 1, 2, 4, 8
TRUNCATED, ROUNDS = 1, 2


def edge_status(poses, edge_index, Z, weights=None):
    """-> (status (E,) int32, live (E,) bool)"""
    poses = np.asarray(poses, np.float64)
    n = len(poses)
    ei = np.asarray(edge_index, np.int64).reshape(-1, 2)
    E = len(ei)
    Z = np.asarray(Z, np.float64).reshape(E, 4, 4)
    w = np.ones((E, 2)) if weights is None else np.asarray(weights, np.float64).reshape(E, 2)
    st = np.zeros(E, np.int32)
    pose_ok = np.isfinite(poses[:, :3, :]).all(axis=(1, 2))
    for e in range(E):
        a, b = ei[e]
        if a < 0 or a >= n or b < 0 or b >= n:
            st[e] |= BAD_INDEX
        elif a == b:
            st[e] |= SELF_LOOP
        if not (np.isfinite(Z[e]).all() and np.isfinite(w[e]).all() and (Z[e, 3] == [0.0, 0.0, 0.0, 1.0]).all()):
            st[e] |= NONFINITE
        if not (st[e] & BAD_INDEX) and not (pose_ok[a] and pose_ok[b]):
            st[e] |= NONFINITE
        if (w[e] < 0).any():
            st[e] |= NEGATIVE_WEIGHT
    live = (st == 0) & (w > 0).any(axis=1)
    return st, live


def _rel(Xa, Xb):
    """X_a^-1 X_b with the difference of the translations taken first"""
    out = np.zeros((4, 4), Xa.dtype)
    out[3, 3] = 1
    out[:3, :3] = Xa[:3, :3].T @ Xb[:3, :3]
    out[:3, 3] = Xa[:3, :3].T @ (Xb[:3, 3] - Xa[:3, 3])
    return out


def _inv(T):
    out = np.zeros((4, 4), T.dtype)
    out[3, 3] = 1
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def rotation_angle(R):
    """|Log_SO3 R| in [0, pi]: atan2 of the axial vector's length and the trace"""
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], R.dtype) / 2
    return np.arctan2(np.sqrt((ax * ax).sum()), (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2)


def cycle(poses, edge_index, Z, e, f, dtype=np.float64):
    """(c_trans, c_rot) of the cycle with row e in the role of e"""
    X, Zs = np.asarray(poses).astype(dtype), np.asarray(Z).astype(dtype)
    (ae, be), (af, bf) = edge_index[e], edge_index[f]
    C = Zs[e] @ _rel(X[be], X[bf]) @ _inv(Zs[f]) @ _rel(X[af], X[ae])
    return np.sqrt((C[:3, 3] ** 2).sum()), rotation_angle(C[:3, :3])


def first_of(edge_index, i, j):
    """the pair in its canonical role: first by (b, row)"""
    return (i, j) if (edge_index[i][1], i) <= (edge_index[j][1], j) else (j, i)


def cycle_errors(poses, edge_index, Z, pairs, dtype=np.float64):
    """(P,2) = (c_trans, c_rot) per pair in the canonical role; NaN for a pair out of range or with a status bit"""
    ei = np.asarray(edge_index, np.int64).reshape(-1, 2)
    st, _ = edge_status(poses, ei, Z, None)
    out = np.full((len(pairs), 2), np.nan, dtype)
    for k, (i, j) in enumerate(np.asarray(pairs, np.int64).reshape(-1, 2)):
        if 0 <= i < len(ei) and 0 <= j < len(ei) and st[i] == 0 and st[j] == 0:
            out[k] = cycle(poses, ei, Z, *first_of(ei, int(i), int(j)), dtype=dtype)
    return out


def relation(poses, edge_index, Z, weights, window=16, trans_thr=1.0, rot_thr=0.1, trans_drift=0.0, rot_drift=0.0,
             max_partners=None):
    """-> dict: adj (E,E) bool symmetric, comparable (E,E) bool, ct / cr (E,E) cycle errors of the comparable pairs (NaN elsewhere),
    margin = the smallest relative distance of a comparable pair's error to its threshold, status (E,), live (E,), pos (E,)
    sorted position of every edge, truncated bool"""
    ei = np.asarray(edge_index, np.int64).reshape(-1, 2)
    E, n = len(ei), len(poses)
    st, live = edge_status(poses, ei, Z, weights)
    key = np.where(live, ei[:, 1], n)
    order = np.argsort(key, kind="stable")
    pos = np.empty(E, np.int64)
    pos[order] = np.arange(E)
    adj, comp = np.zeros((E, E), bool), np.zeros((E, E), bool)
    ct, cr = np.full((E, E), np.nan), np.full((E, E), np.nan)
    truncated, margin = False, np.inf
    H = None if max_partners is None else max_partners // 2
    idx = np.flatnonzero(live)
    for x in idx:
        for y in idx:
            if pos[x] >= pos[y]:
                continue                                        # each pair once, x earlier in sorted order: x plays e
            db, da = abs(ei[x, 1] - ei[y, 1]), abs(ei[x, 0] - ei[y, 0])
            if db > window:
                continue
            if H is not None and pos[y] - pos[x] > H:
                truncated = True
                continue
            if da > window:
                continue
            t, r = cycle(poses, ei, Z, x, y)
            g = float(db + da)
            tt, rr = trans_thr + trans_drift * g, rot_thr + rot_drift * g
            comp[x, y] = comp[y, x] = True
            ct[x, y] = ct[y, x] = t
            cr[x, y] = cr[y, x] = r
            if tt > 0:
                margin = min(margin, abs(t - tt) / tt)
            if rr > 0:
                margin = min(margin, abs(r - rr) / rr)
            adj[x, y] = adj[y, x] = bool(t <= tt and r <= rr)
    return {"adj": adj, "comparable": comp, "ct": ct, "cr": cr, "margin": margin, "status": st, "live": live, "pos": pos,
            "truncated": truncated}


def select(adj, live, min_support=2, max_rounds=16):
    """synchronous rounds on the relation -> dict keep, support0, support, rounds (those that removed something), hit_limit"""
    alive = np.array(live, bool)
    support0 = (adj & alive[None, :]).sum(axis=1).astype(np.int32) * alive
    rounds, last = 0, False
    for _ in range(max_rounds):
        count = (adj & alive[None, :]).sum(axis=1)
        gone = alive & (count < min_support)
        last = bool(gone.any())
        if not last:
            break
        alive = alive & ~gone
        rounds += 1
    support = ((adj & alive[None, :]).sum(axis=1) * alive).astype(np.int32)
    return {"keep": alive, "support0": support0.astype(np.int32), "support": support, "rounds": rounds, "hit_limit": last}


def filter_loops(poses, edge_index, Z, weights, window=16, trans_thr=1.0, rot_thr=0.1, trans_drift=0.0, rot_drift=0.0,
                 min_support=2, max_rounds=16, max_partners=256):
    rel = relation(poses, edge_index, Z, weights, window, trans_thr, rot_thr, trans_drift, rot_drift, max_partners)
    sel = select(rel["adj"], rel["live"], min_support, max_rounds)
    w = np.asarray(weights, np.float64).reshape(-1, 2)
    out = dict(rel)
    out.update(sel)
    out["weights"] = np.where(sel["keep"][:, None], w, 0.0)
    out["flags"] = (TRUNCATED if rel["truncated"] else 0) | (ROUNDS if sel["hit_limit"] else 0)
    return out
