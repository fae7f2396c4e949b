"""float64 numpy restatement of the loop-closure layer (include/egonn_hip.h: egonn_time_windows, egonn_knn_window,
egonn_window_radius, egonn_pr_curve; egonn_amd/loop_closure.py: evaluate_loop_closure), written from the stated contract.
It shares no code with egonn_amd/loop_closure.py; tests/test_loop_closure_host.py checks it on hand-made cases and
tests/test_gpu_loop_closure.py holds the device to it.

  windows        hi[q] = #{j : t_db[j] <= t_q[q] - min_gap}, lo[q] = #{j : t_db[j] < t_q[q] - max_gap}
  windowed kNN   rows [max(lo, 0), min(hi, M)) by ascending (distance, index); a NaN distance is never a neighbour, +inf is a
                 distance like any other; (-1, +inf) behind the last neighbour
  radius         count[q] = rows of the window with distance <= radius; pred_dist[q] = distance to row pred[q], +inf outside [0, M)
  curve          predictions by ascending (score, index), -0.0 = +0.0, +inf / NaN = no prediction; one point per distinct score;
                 at threshold tau: predicted iff score <= tau, TP = predicted and correct, FP = predicted and not correct,
                 FN = not predicted and revisit
"""
import numpy as np


def windows(t_db, t_q, min_gap, max_gap=np.inf, dtype=np.float64):
    """dtype = np.float32 restates what a single-precision implementation would compute (the stamps and the bounds rounded)"""
    a, b = np.asarray(t_db, dtype=dtype), np.asarray(t_q, dtype=dtype)
    x_hi, x_lo = (b - dtype(min_gap)).astype(dtype), (b - dtype(max_gap)).astype(dtype)
    hi = np.array([int(np.sum(a <= x)) for x in x_hi], np.int32)
    lo = np.array([int(np.sum(a < x)) for x in x_lo], np.int32)
    return lo, hi


def is_sorted(t_db):
    a = np.asarray(t_db, dtype=np.float64)
    return bool(np.all(a[:-1] <= a[1:]))          # False with a NaN


def knn_window(query, db, k, lo, hi):
    """-> idx (Q, k) int32, dist (Q, k) float32 (the float64 distance rounded once)"""
    q64, d64 = np.asarray(query, np.float64), np.asarray(db, np.float64)
    Q, M = len(q64), len(d64)
    idx = np.full((Q, k), -1, np.int32)
    dist = np.full((Q, k), np.inf, np.float32)
    for q in range(Q):
        a = max(int(lo[q]), 0) if lo is not None else 0
        b = min(int(hi[q]), M)
        if b <= a:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            dd = np.sqrt(((d64[a:b] - q64[q]) ** 2).sum(axis=1))
        rows = [(float(dd[j]), a + j) for j in range(b - a) if not np.isnan(dd[j])]
        rows.sort()                                   # (distance, index): ties to the lower index, +inf last in index order
        for r, (v, j) in enumerate(rows[:k]):
            idx[q, r], dist[q, r] = j, np.float32(v)
    return idx, dist


def window_radius(qpos, dbpos, lo, hi, radius, pred=None):
    """-> count (Q,) int32, pred_dist (Q,) float32 (None without pred).  Distances are rounded to float32 before the comparison
    with the float32 radius, as the contract states the comparison."""
    qp, dp = np.asarray(qpos, np.float64), np.asarray(dbpos, np.float64)
    Q, M = len(qp), len(dp)
    rad = np.float32(radius)
    count = np.zeros(Q, np.int32)
    pd = None if pred is None else np.full(Q, np.inf, np.float32)
    for q in range(Q):
        a = max(int(lo[q]), 0) if lo is not None else 0
        b = min(int(hi[q]), M)
        if b > a:
            dd = np.sqrt(((dp[a:b] - qp[q]) ** 2).sum(axis=1)).astype(np.float32)
            count[q] = int(np.sum(dd <= rad))
        if pred is not None and 0 <= int(pred[q]) < M:
            pd[q] = np.float32(np.sqrt(((dp[int(pred[q])] - qp[q]) ** 2).sum()))
    return count, pd


def _canonical(score):
    s = np.asarray(score, np.float32).astype(np.float64)
    s = np.where(s == 0.0, 0.0, s)                    # -0.0 counts as +0.0
    return s, ~(np.isnan(s) | (s == np.inf))


def pr_curve(score, correct, revisit):
    """-> dict of order, cum_tp, cum_fp, cum_rev (int32), group_end (uint8), n_predicted, n_revisit"""
    s, predicted = _canonical(score)
    n = len(s)
    correct, revisit = np.asarray(correct), np.asarray(revisit)
    first = sorted((i for i in range(n) if predicted[i]), key=lambda i: (s[i], i))
    order = first + [i for i in range(n) if not predicted[i]]
    cum = np.zeros((3, n), np.int32)
    end = np.zeros(n, np.uint8)
    tp = fp = rev = 0
    for p, i in enumerate(order):
        if p < len(first):
            tp += int(correct[i] != 0)
            fp += int(correct[i] == 0)
            rev += int(revisit[i] != 0)
            end[p] = 1 if p + 1 == len(first) or s[order[p + 1]] != s[i] else 0
        cum[:, p] = tp, fp, rev
    return dict(order=np.array(order, np.int32).reshape(n), cum_tp=cum[0], cum_fp=cum[1], cum_rev=cum[2], group_end=end,
                n_predicted=len(first), n_revisit=int(np.sum(revisit != 0)))


def curve(score, correct, revisit):
    """The protocol by its definition, one pass over all scans per threshold.  -> dict: thresholds, tp, fp, fn, precision, recall
    and the scalars f1_max, f1_threshold, average_precision, recall_at_full_precision, extended_precision"""
    s, predicted = _canonical(score)
    correct, revisit = np.asarray(correct) != 0, np.asarray(revisit) != 0
    taus = sorted(set(s[predicted].tolist()))
    tp, fp, fn = [], [], []
    for tau in taus:
        said = predicted & (s <= tau)
        tp.append(int(np.sum(said & correct)))
        fp.append(int(np.sum(said & ~correct)))
        fn.append(int(np.sum(~said & revisit)))
    P = [t / (t + f) for t, f in zip(tp, fp)]
    R = [t / (t + m) if t + m > 0 else 0.0 for t, m in zip(tp, fn)]
    F = [2 * t / (2 * t + f + m) for t, f, m in zip(tp, fp, fn)]
    ap, prev = 0.0, 0.0
    for p, r in zip(P, R):
        ap += (r - prev) * p
        prev = r
    best = max(range(len(F)), key=lambda i: (F[i], -i)) if F else -1          # the first of equal maxima
    full = max([r for p, r in zip(P, R) if p == 1.0], default=0.0)
    return dict(thresholds=np.array(taus, np.float64), tp=np.array(tp, np.int64), fp=np.array(fp, np.int64), fn=np.array(fn, np.int64),
                precision=np.array(P, np.float64), recall=np.array(R, np.float64), f1_max=F[best] if F else 0.0,
                f1_threshold=taus[best] if F else -np.inf, average_precision=ap, recall_at_full_precision=full,
                extended_precision=0.5 * ((P[0] if P else 0.0) + full))


SCALARS = ("f1_max", "f1_threshold", "average_precision", "recall_at_full_precision", "extended_precision")
