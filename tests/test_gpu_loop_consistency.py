"""GPU tests of the loop-consistency filter (run with -m gpu on an MI355X) against the float64 restatement
tests/loop_consistency_ref.py: the cycle arithmetic against the restatement in numpy.longdouble, supports, survivors and rounds
exactly on a planted trajectory at every size around the wave width, symmetry and row order, the cascade of a path graph, the
position cap, dead edges bit for bit, the seam to optimize_trajectory, determinism eager and replayed."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import loop_consistency_ref as ref
from tests import pose_graph_ref as pg_ref

pytestmark = pytest.mark.gpu

KW = dict(window=16, trans_thr=1.5, rot_thr=0.15)
N_TRUE, N_FALSE = 129, 12


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


def _np(t):
    return t.detach().cpu().numpy()


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _rand_pose(rng, angle, span, offset=0.0):
    T = np.eye(4)
    ax = rng.standard_normal(3)
    T[:3, :3] = pg_ref.exp_so3(ax / np.linalg.norm(ax) * rng.uniform(0, angle))
    T[:3, 3] = offset + rng.uniform(-span, span, 3)
    return T


def _rel(Xa, Xb):
    out = np.eye(4)
    out[:3, :3] = Xa[:3, :3].T @ Xb[:3, :3]
    out[:3, 3] = Xa[:3, :3].T @ (Xb[:3, 3] - Xa[:3, 3])
    return out


_PLANTED = {}


def _planted(seed=3, n=257, lap=128, radius=20.0):
    """257 poses on a 20 m circle driven twice (lap 128), odometry noise up to 0.02 m and 0.002 rad per step, dead-reckoned; one
    true loop per pose from 128 on (noise up to 0.05 m, 0.005 rad): 129; 12 false loops with a random Z of up to 1 rad and 5 m
    between random nodes at least 32 steps apart.  -> truth, drifting poses, edge_index (141,2), Z, weights: true loops first"""
    if seed not in _PLANTED:
        rng = np.random.default_rng(seed)
        T = np.tile(np.eye(4), (n, 1, 1))
        for i in range(n):
            a = 2 * math.pi * i / lap
            T[i, :3, :3] = pg_ref.exp_so3([0.0, 0.0, a + math.pi / 2])
            T[i, :3, 3] = [radius * math.cos(a), radius * math.sin(a), 0.0]
        Zo = np.stack([_rel(T[i], T[i + 1]) @ _rand_pose(rng, 0.002, 0.02) for i in range(n - 1)])
        X0 = T.copy()
        for i in range(n - 1):
            X0[i + 1] = X0[i] @ Zo[i]
        true = np.array([[i - lap, i] for i in range(lap, n)], np.int32)
        Zt = np.stack([_rel(T[a], T[b]) @ _rand_pose(rng, 0.005, 0.05) for a, b in true])
        false = []
        while len(false) < N_FALSE:
            a, b = sorted(int(v) for v in rng.integers(0, n, 2))
            if b - a >= 32:
                false.append([a, b])
        Zf = np.stack([_rand_pose(rng, 1.0, 5.0) for _ in false])
        ei, Z = np.concatenate([true, np.array(false, np.int32)]), np.concatenate([Zt, Zf])
        assert len(true) == N_TRUE and len(ei) == N_TRUE + N_FALSE
        _PLANTED[seed] = (T, X0, ei, Z, np.tile([1000.0, 400.0], (len(ei), 1)))
    return _PLANTED[seed]


def _mixed(seed=3):
    """the planted case with the false loops spread among the true ones (one after every tenth), so that prefixes hold both"""
    T, X0, ei, Z, w = _planted(seed)
    order = []
    for k in range(N_TRUE):
        order.append(k)
        if k % 10 == 9 and k // 10 < N_FALSE:
            order.append(N_TRUE + k // 10)
    order = np.array(order)
    assert len(order) == N_TRUE + N_FALSE
    return T, X0, ei[order], Z[order], w[order], order >= N_TRUE


def _run(gpu, X, ei, Z, w, **kw):
    got = gpu.filter_loops(_cu(X), {"edge_index": _cu(ei), "Z": _cu(Z), "weights": _cu(w)}, **kw)
    return {k: _np(got[k]).copy() for k in ("keep", "support0", "support", "weights", "rounds", "edge_status", "status")}


def _same(got, want, w):
    """the device's outputs against the restatement's, exactly"""
    assert got["support0"].tolist() == want["support0"].tolist()
    assert got["keep"].tolist() == want["keep"].tolist()
    assert got["support"].tolist() == want["support"].tolist()
    assert int(got["rounds"]) == want["rounds"] and int(got["status"][0]) == want["flags"]
    assert got["edge_status"].tolist() == want["status"].tolist()
    assert np.array_equal(_bits(got["weights"]), _bits(np.where(want["keep"][:, None], w, 0.0)))


# ------------------------------------------------------------------ 1. the cycle arithmetic
ANGLES = [0.0, 1e-9, 1e-4, 1.0, 3.0, math.pi - 2e-3, math.pi]


def test_cycle_errors_against_the_restatement_in_longdouble(gpu):
    """Pairs whose cycle rotates by {0, 1e-9, 1e-4, 1, 3, pi - 2e-3} (both sides of the series switch at 0.05) on poses 1e6 m from
    the origin.  The yardstick is the restatement evaluated in numpy.longdouble on the same float64 inputs; the device may be off
    by 4 x the float64 restatement's own error against it, and never has to be closer than 16 * 2^-53 times the largest
    coordinate (c_trans) or 16 * 2^-53 (c_rot): the margin covers another, equally valid operation order and FMA contraction.
    Measured on the MI355X: c_trans error 2.2e-14 m (restatement 2.4e-14 m, floor 1.8e-9 m), c_rot error 1.3e-16 rad (restatement
    1.3e-16 rad, floor 1.8e-15 rad).  (e, f) and (f, e) are equal bit for bit; out-of-range pairs and dead edges give NaN.
    The last angle is an exact half turn, the yaw flip of a false loop: poses without rotation, Z_e = I and Z_f = diag(-1, -1, 1),
    so the cycle's rotation is the half turn bit for bit, its axial vector is 0 and theta / sin(theta) is not a number.  c_rot is
    theta itself there: pi to one ulp, never NaN."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    rng = np.random.default_rng(21)
    m = len(ANGLES)
    assert ANGLES[-1] == math.pi
    nan_pose = 4 * (m - 1)
    X = np.stack([_rand_pose(rng, math.pi, 100.0, offset=1e6) for _ in range(nan_pose + 1)])
    ei, Z = [], []
    for k, ang in enumerate(ANGLES[:-1]):
        a, b, a2, b2 = 4 * k, 4 * k + 1, 4 * k + 2, 4 * k + 3
        ax = rng.standard_normal(3)
        Err = np.eye(4)
        Err[:3, :3] = pg_ref.exp_so3(ax / np.linalg.norm(ax) * ang)
        Err[:3, 3] = rng.uniform(-3, 3, 3) if k else 0.0
        ei += [[a, b], [a2, b2]]
        Z += [_rel(X[a], X[b]), _rel(X[a2], X[b2]) @ Err]               # the cycle is a conjugate of Err^-1: it turns by ang
    flat = np.tile(np.eye(4), (4, 1, 1))                                  # the half turn: four poses that do not rotate
    flat[:, :3, 3] = 1e6 + np.array([[3.0, -40.5, 7.25], [-12.0, 8.0, 0.5], [55.5, 1.0, -2.0], [-7.0, 66.0, 30.0]])
    X = np.concatenate([X, flat])
    ei += [[nan_pose + 1, nan_pose + 2], [nan_pose + 3, nan_pose + 4]]
    Z += [np.eye(4), np.diag([-1.0, -1.0, 1.0, 1.0])]
    dead0 = len(ei)
    ei += [[-1, 3], [5, 5], [2, 3], [1, nan_pose]]                        # bad index, self loop, NaN in Z, NaN pose
    Z += [np.eye(4)] * 4
    ei, Z = np.array(ei, np.int32), np.stack(Z)
    Z[dead0 + 2, 0, 3] = np.nan
    X[nan_pose, 2, 2] = np.nan
    pairs = [[2 * k, 2 * k + 1] for k in range(m)] + [[2 * k + 1, 2 * k] for k in range(m)] + [[0, 3], [7, 2], [4, 4]]
    n_live = len(pairs)
    pairs += [[0, dead0 + j] for j in range(4)] + [[dead0 + 1, 2], [0, len(ei)], [-1, 0], [2 ** 31 - 1, 1]]
    pairs = np.array(pairs, np.int64)
    want = ref.cycle_errors(X, ei, Z, pairs, dtype=np.longdouble)
    own = ref.cycle_errors(X, ei, Z, pairs, dtype=np.float64)
    assert np.allclose(want[:m, 1].astype(np.float64), ANGLES, rtol=0, atol=1e-9)
    assert not np.isnan(want[:n_live]).any() and np.isnan(want[n_live:]).all()
    loops = {"edge_index": _cu(ei), "Z": _cu(Z), "weights": _cu(np.ones((len(ei), 2)))}
    got = _np(gpu.loop_cycle_errors(_cu(X), loops, _cu(pairs.astype(np.int32))))
    assert np.isnan(got[n_live:]).all() and not np.isnan(got[:n_live]).any()
    floor = 16 * 2.0 ** -53 * np.array([np.nanmax(np.abs(X[:, :3, 3])), 1.0])
    err = np.abs(got[:n_live].astype(np.longdouble) - want[:n_live]).astype(np.float64)
    own_err = np.abs(own[:n_live].astype(np.longdouble) - want[:n_live]).astype(np.float64)
    bound = np.maximum(4 * own_err, floor[None, :])
    print(f"[loop consistency] cycle errors against longdouble: device c_trans {err[:, 0].max():.2e} m, c_rot {err[:, 1].max():.2e} rad; "
          f"restatement c_trans {own_err[:, 0].max():.2e} m, c_rot {own_err[:, 1].max():.2e} rad; floors {floor[0]:.2e} m, {floor[1]:.2e} rad")
    assert (err <= bound).all(), (err, bound)
    assert np.array_equal(_bits(got[:m]), _bits(got[m: 2 * m]))               # (e, f) and (f, e): the same bits
    assert abs(float(want[m - 1, 1]) - math.pi) <= 2.0 ** -51 and abs(got[m - 1, 1] - math.pi) <= 2.0 ** -51 and got[2 * m - 1, 1] == got[m - 1, 1]


# ------------------------------------------------------------------ 2. support, survivors and rounds exactly
def _check_margin(want, least=1e-6):
    """a condition of the exact comparison, not a measurement: no comparable pair sits within a relative 1e-6 of a threshold"""
    assert want["margin"] >= least, want["margin"]


@pytest.mark.parametrize("seed", [3, 5])
@pytest.mark.parametrize("min_support", [1, 2])
def test_planted_loops_match_the_restatement_exactly(gpu, seed, min_support):
    """window 16, thresholds 1.5 m and 0.15 rad.  Checked on the restatement first: the margin to the thresholds (seed 3: 0.79,
    seed 5: 0.78 relative), all 129 true loops kept, all 12 false loops removed; seed 3: the smallest true support is 16, the
    true-true cycles stay below 0.32 m and 0.016 rad."""
    T, X0, ei, Z, w = _planted(seed)
    want = ref.filter_loops(X0, ei, Z, w, min_support=min_support, **KW)
    _check_margin(want, 0.1)
    assert want["keep"][:N_TRUE].all() and not want["keep"][N_TRUE:].any() and not want["truncated"]
    if seed == 3:
        assert want["support0"][:N_TRUE].min() == 16
        assert np.nanmax(want["ct"][:N_TRUE, :N_TRUE]) < 0.75 and np.nanmax(want["cr"][:N_TRUE, :N_TRUE]) < 0.052
    _same(_run(gpu, X0, ei, Z, w, min_support=min_support, **KW), want, w)


@pytest.mark.parametrize("E", [1, 2, 63, 64, 65, 141])
def test_prefixes_and_padded_rows(gpu, E):
    """E rows of the planted case with the false loops spread among the true ones: as a prefix, and as the first half of that
    prefix with rows of weight 0 and a = -1, as loop_edges makes them, scattered in between"""
    T, X0, ei, Z, w, is_false = _mixed()
    for pad in (False, True):
        e2, Z2, w2 = ei[:E].copy(), Z[:E].copy(), w[:E].copy()
        if pad:
            off = np.random.default_rng(E).permutation(E)[: E - E // 2]
            e2[off, 0], w2[off] = -1, 0.0
            Z2[off] = np.eye(4)
        want = ref.filter_loops(X0, e2, Z2, w2, min_support=2, **KW)
        _check_margin(want)
        if pad:
            assert (want["status"][off] == ref.BAD_INDEX).all() and not want["keep"][off].any()
        _same(_run(gpu, X0, e2, Z2, w2, min_support=2, **KW), want, w2)
        if E == 141 and not pad:
            assert want["keep"].tolist() == (~is_false).tolist()


# ------------------------------------------------------------------ 3. symmetry and row order
def test_adjacency_is_symmetric_and_rows_may_be_permuted(gpu):
    """The adjacency that the outputs imply: A[i, j] = the drop of support0[i] when edge j alone is switched off.  On the first 44
    rows of the mixed case (4 false loops among them) it is symmetric and the restatement's.  Then the whole case with its rows
    permuted: every output row moves with its row and nothing else changes (no truncation: max_partners = 256)."""
    T, X0, ei, Z, w, _ = _mixed()
    m = 44
    e2, Z2, w2 = ei[:m], Z[:m], w[:m]
    want = ref.filter_loops(X0, e2, Z2, w2, **KW)
    _check_margin(want)
    base = _run(gpu, X0, e2, Z2, w2, **KW)["support0"]
    A = np.zeros((m, m), np.int64)
    for j in range(m):
        wj = w2.copy()
        wj[j] = 0.0
        A[:, j] = base - _run(gpu, X0, e2, Z2, wj, **KW)["support0"]
        A[j, j] = 0                                                           # its own support falls to 0: that is not a vote
    assert np.array_equal(A, A.T) and np.array_equal(A, want["adj"].astype(np.int64)) and A.sum() > 0
    first = _run(gpu, X0, ei, Z, w, **KW)
    assert int(first["status"][0]) == 0
    perm = np.random.default_rng(9).permutation(len(ei))
    second = _run(gpu, X0, ei[perm], Z[perm], w[perm], **KW)
    for k in ("keep", "support0", "support", "weights", "edge_status"):
        assert np.array_equal(_bits(second[k]), _bits(first[k][perm])), k
    assert int(second["rounds"]) == int(first["rounds"]) and int(second["status"][0]) == 0


# ------------------------------------------------------------------ 4. the cascade of a path graph
def test_cascade_of_a_path_graph(gpu):
    """The first 40 true loops with window = 1: each is comparable with its two neighbours only, a path.  min_support = 2 peels
    it from both ends, two edges a round: nothing survives after exactly 20 removing rounds.  With max_rounds = 5 ROUNDS is set
    and the survivors are the restatement's after 5 synchronous rounds.  min_support = 1 keeps all 40 in 0 rounds."""
    T, X0, ei, Z, w = _planted()
    ei, Z, w = ei[:40], Z[:40], w[:40]
    kw = dict(window=1, trans_thr=1.5, rot_thr=0.15)
    rel = ref.relation(X0, ei, Z, w, **kw)
    deg = rel["adj"].sum(axis=1)
    assert deg.tolist() == [1] + [2] * 38 + [1] and rel["margin"] >= 0.5
    want = ref.filter_loops(X0, ei, Z, w, min_support=2, max_rounds=32, **kw)
    assert not want["keep"].any() and want["rounds"] == 20 and want["flags"] == 0
    _same(_run(gpu, X0, ei, Z, w, min_support=2, max_rounds=32, **kw), want, w)
    # exactly as many rounds as it needs: the last one still removes, so the limit is reported although nothing is left
    want = ref.filter_loops(X0, ei, Z, w, min_support=2, max_rounds=20, **kw)
    assert not want["keep"].any() and want["rounds"] == 20 and want["flags"] == ref.ROUNDS
    _same(_run(gpu, X0, ei, Z, w, min_support=2, max_rounds=20, **kw), want, w)
    want = ref.filter_loops(X0, ei, Z, w, min_support=2, max_rounds=5, **kw)
    assert want["keep"].tolist() == [False] * 5 + [True] * 30 + [False] * 5 and want["flags"] == ref.ROUNDS and want["rounds"] == 5
    _same(_run(gpu, X0, ei, Z, w, min_support=2, max_rounds=5, **kw), want, w)
    want = ref.filter_loops(X0, ei, Z, w, min_support=1, **kw)
    assert want["keep"].all() and want["rounds"] == 0 and want["flags"] == 0
    _same(_run(gpu, X0, ei, Z, w, min_support=1, **kw), want, w)


# ------------------------------------------------------------------ 5. the position cap
def test_position_cap(gpu):
    """window = 40 on the planted case: an edge has partners more than 32 places away among the edges sorted by b.  With
    max_partners = 64 TRUNCATED is set and the result is the restatement's under the same cap; with 256 the bit is clear."""
    T, X0, ei, Z, w = _planted()
    kw = dict(window=40, trans_thr=1.5, rot_thr=0.15, min_support=2)
    capped = ref.filter_loops(X0, ei, Z, w, max_partners=64, **kw)
    free = ref.filter_loops(X0, ei, Z, w, max_partners=256, **kw)
    _check_margin(capped)
    _check_margin(free)
    assert capped["flags"] == ref.TRUNCATED and free["flags"] == 0 and (capped["support0"] < free["support0"]).any()
    assert capped["support0"].max() <= 64
    _same(_run(gpu, X0, ei, Z, w, max_partners=64, **kw), capped, w)
    _same(_run(gpu, X0, ei, Z, w, max_partners=256, **kw), free, w)


# ------------------------------------------------------------------ 6. dead edges
def test_dead_edges_change_nothing_else(gpu):
    """One row of each dead kind scattered into the first 70 rows of the mixed case: weight 0, a = -1, a self loop, a NaN in Z,
    an edge that touches a NaN pose, a negative weight.  Each carries its bit, is not kept and has weights 0; every other row
    is bit-equal to the run without them.  Then a false loop reported twice: the two keep each other at min_support = 1 and
    fall at 2."""
    T, X0, ei, Z, w, is_false = _mixed()
    m = 70
    X = np.concatenate([X0, X0[-1:]])                                         # node 257 is touched by the dead edge only
    X[-1, 1, 3] = np.nan
    base = _run(gpu, X, ei[:m], Z[:m], w[:m], **KW)
    assert base["keep"].any() and not base["keep"].all()
    dead_e = np.array([[3, 131], [-1, 140], [150, 150], [5, 133], [100, 257], [7, 135]], np.int32)
    dead_Z = np.stack([Z[k] for k in range(6)])
    dead_Z[3, 2, 1] = np.nan
    dead_w = np.array([[0.0, 0.0], [1000.0, 400.0], [1000.0, 400.0], [1000.0, 400.0], [1000.0, 400.0], [1000.0, -400.0]])
    bits = [0, ref.BAD_INDEX, ref.SELF_LOOP, ref.NONFINITE, ref.NONFINITE, ref.NEGATIVE_WEIGHT]
    at = np.array([0, 13, 27, 40, 64, 75])                                    # rows of the dead edges in the larger input
    rows = np.ones(m + 6, bool)
    rows[at] = False
    e2, Z2, w2 = np.zeros((m + 6, 2), np.int32), np.zeros((m + 6, 4, 4)), np.zeros((m + 6, 2))
    e2[rows], Z2[rows], w2[rows] = ei[:m], Z[:m], w[:m]
    e2[at], Z2[at], w2[at] = dead_e, dead_Z, dead_w
    got = _run(gpu, X, e2, Z2, w2, **KW)
    assert got["edge_status"][at].tolist() == bits and not got["keep"][at].any() and (got["weights"][at] == 0.0).all()
    assert (got["support0"][at] == 0).all() and (got["support"][at] == 0).all()
    for k in ("keep", "support0", "support", "weights", "edge_status"):
        assert np.array_equal(_bits(got[k][rows]), _bits(base[k])), k
    assert int(got["rounds"]) == int(base["rounds"]) and int(got["status"][0]) == int(base["status"][0])
    _same(got, ref.filter_loops(X, e2, Z2, w2, **KW), w2)
    # duplicates count each other
    f = int(np.flatnonzero(is_false)[0])
    e3, Z3, w3 = np.concatenate([ei[:m], ei[f: f + 1]]), np.concatenate([Z[:m], Z[f: f + 1]]), np.concatenate([w[:m], w[f: f + 1]])
    one = _run(gpu, X0, e3, Z3, w3, min_support=1, **KW)
    two = _run(gpu, X0, e3, Z3, w3, min_support=2, **KW)
    assert one["keep"][[f, m]].all() and one["support"][[f, m]].tolist() == [1, 1] and not two["keep"][[f, m]].any()
    assert not _run(gpu, X0, ei[:m], Z[:m], w[:m], min_support=1, **KW)["keep"][f]


# ------------------------------------------------------------------ 7. the seam to the pose graph
def _mean_terr(P, T):
    return float(np.linalg.norm(P[:, :3, 3] - T[:, :3, 3], axis=1).mean())


def test_optimize_trajectory_with_the_filter(gpu):
    """optimize_trajectory(poses, loops, consistency={...}) on the planted case is, bit for bit, optimize_trajectory on the same
    loops with the rows the restatement removes given weight 0 (the pose graph's guarantee for switched-off edges).  Its mean
    translation error against the truth is no larger than that of the Huber run (robust_delta = 0.2) on the unfiltered loops.
    Measured on the MI355X: 0.093 m filtered, 20.322 m with Huber, 23.404 m unfiltered without a robust kernel (start: 0.379 m)."""
    T, X0, ei, Z, w, is_false = _mixed()
    n = len(T)
    want = ref.filter_loops(X0, ei, Z, w, **KW)
    _check_margin(want)
    assert want["keep"].tolist() == (~is_false).tolist()
    kw = dict(max_iterations=8, pcg_iterations=4 * n, pcg_tol=1e-9, odometry_weight=(400.0, 100.0))
    loops = {"edge_index": _cu(ei), "Z": _cu(Z), "weights": _cu(w)}
    got = gpu.optimize_trajectory(_cu(X0), loops, consistency=dict(KW), **kw)
    masked = dict(loops, weights=_cu(np.where(want["keep"][:, None], w, 0.0)))
    direct = gpu.optimize_trajectory(_cu(X0), masked, **kw)
    for k in ("poses", "cost_trace", "accept_trace", "edge_status", "weights", "Z", "edge_index"):
        assert np.array_equal(_bits(_np(got[k])), _bits(_np(direct[k]))), k
    assert "consistency" in got and "consistency" not in direct
    assert _np(got["consistency"]["keep"]).tolist() == want["keep"].tolist()
    # with out= the filter's buffers are used again too
    first, filt, scratch = _np(got["poses"]).copy(), got["consistency"], got["consistency"]["_scratch"].data_ptr()
    got["poses"].fill_(-3)
    filt["keep"].fill_(True)
    again = gpu.optimize_trajectory(_cu(X0), loops, consistency=dict(KW), out=got, **kw)
    assert again["consistency"] is filt and filt["_scratch"].data_ptr() == scratch
    assert np.array_equal(_bits(_np(again["poses"])), _bits(first)) and _np(filt["keep"]).tolist() == want["keep"].tolist()
    with pytest.raises(ValueError, match="without consistency"):
        gpu.optimize_trajectory(_cu(X0), loops, consistency=dict(KW), out=direct, **kw)
    huber =gpu.optimize_trajectory(_cu(X0), loops, robust_delta=0.2, **kw)
    plain = gpu.optimize_trajectory(_cu(X0), loops, **kw)
    e0, e_f, e_h, e_p = (_mean_terr(X0, T), _mean_terr(_np(got["poses"]), T), _mean_terr(_np(huber["poses"]), T),
                         _mean_terr(_np(plain["poses"]), T))
    print(f"[loop consistency] mean translation error: start {e0:.3f} m, filtered {e_f:.3f} m, Huber {e_h:.3f} m, "
          f"unfiltered and not robust {e_p:.3f} m")
    assert e_f <= e_h


# ------------------------------------------------------------------ 8. determinism and capture
def _capture(lib, _lib, st, fn):
    g = ctypes.c_void_p()
    _lib.check(lib.egonn_graph_begin(st.cuda_stream))
    try:
        fn()
    finally:
        rc = lib.egonn_graph_end(st.cuda_stream, ctypes.byref(g))
    _lib.check(rc)
    return g


def _scribble():
    """allocate and fill what the caching allocator hands out next: memory a call has freed since is overwritten"""
    junk = [torch.full((1 << k,), 0x7f, dtype=torch.uint8, device="cuda") for k in range(8, 22)]
    torch.cuda.synchronize()
    return junk


KEYS = ("keep", "support0", "support", "weights", "_rounds", "edge_status", "status")


def test_two_runs_and_a_replayed_graph_are_bit_equal(gpu):
    """Two eager runs and two replays of a captured filter_loops(..., out=) give the same bits.  edge_index as int64 and float32
    weights need conversion: with out= they go through staging buffers that the result owns, so a replay after the freed memory
    was overwritten reads live memory, and reads the caller's tensors anew: changed in place between replays they give the bits
    of an eager call on the changed values."""
    from egonn_amd import _lib
    lib = _lib.load()
    T, X0, ei, Z, w, _ = _mixed()
    w32 = w.astype(np.float32)
    poses, e64, Zd, wd = _cu(X0), _cu(ei.astype(np.int64)), _cu(Z), _cu(w32)
    loops = {"edge_index": e64, "Z": Zd, "weights": wd}
    kw = dict(min_support=2, **KW)
    eager = lambda: {k: _np(v).copy() for k, v in gpu.filter_loops(poses, loops, **kw).items() if k in KEYS}       # noqa: E731
    first, again = eager(), eager()
    for k in KEYS:
        assert np.array_equal(_bits(first[k]), _bits(again[k])), k
    want = ref.filter_loops(X0, ei, Z, w32.astype(np.float64), **kw)
    assert first["keep"].tolist() == want["keep"].tolist() and 0 < want["keep"].sum() < len(ei)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        out = gpu.filter_loops(poses, loops, **kw)                                # eager once: every buffer exists now
        st.synchronize()
        assert set(out["_in"]) == {"edge_index", "weights"}
        g = _capture(lib, _lib, st, lambda: gpu.filter_loops(poses, loops, out=out, **kw))
        junk = _scribble()
        for rep in range(2):
            for k in KEYS:
                out[k].fill_(-3)
            _lib.check(lib.egonn_graph_launch(g, st.cuda_stream))
            st.synchronize()
            for k in KEYS:
                assert np.array_equal(_bits(_np(out[k])), _bits(first[k])), (rep, k)
        # the caller's tensors changed in place: the first ten true loops switched off, one loop rewired
        wd[:10] = 0.0
        e64[20, 0] += 60
        _lib.check(lib.egonn_graph_launch(g, st.cuda_stream))
        st.synchronize()
        replay = {k: _np(out[k]).copy() for k in KEYS}
        with pytest.raises(ValueError, match="staging buffer"):
            gpu.filter_loops(poses.to(torch.float32), loops, out=out, **kw)
        with pytest.raises(ValueError, match="other shapes"):
            gpu.filter_loops(poses, {k: v[:-1] for k, v in loops.items()}, out=out, **kw)
    lib.egonn_graph_destroy(g)
    torch.cuda.current_stream().wait_stream(st)
    second = eager()
    for k in KEYS:
        assert np.array_equal(_bits(replay[k]), _bits(second[k])), k
    assert not second["keep"][:10].any() and not second["keep"][20] and first["keep"][20]
    del junk
