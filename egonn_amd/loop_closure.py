"""Loop-closure detection inside one trajectory: "has the vehicle been here before, and if so, what is the relative pose?"

Every scan is searched against the scans that are old enough (`time_windows`: at least `min_time_gap` seconds earlier, so each
query has its own admissible prefix of the database), by a kNN that keeps its k best while the rows stream past
(`knn_window`: no Q x M distance matrix, scratch independent of the map), the candidates are verified from their keypoints
(`relocalize.verify_candidates`) and the detector is graded by its precision/recall curve (`evaluate_loop_closure`), because
a false loop corrupts a pose graph and recall@k cannot see that.  `detect_loops` is the offline search over a whole
trajectory, `LoopDetector` the online form whose batched pushes give the bits of one offline call.
All device arithmetic runs in libegonn_hip (csrc/loop_closure.hip); there is no torch or numpy fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import as_dev as _dev
from .registration import check_method
from .relocalize import KeypointMap, verify_candidates

MAX_K = 64        # one list entry per lane of a wave (csrc/loop_closure.hip)


def knn_window(query: torch.Tensor, database: torch.Tensor, k: int, win_hi, win_lo=None):
    """(Q,D), (M,D), win_hi (Q,) [, win_lo (Q,)] int32 -> indices (Q,k) int32, distances (Q,k): `retrieval.knn` of query q on
    database[lo:hi] with lo = max(win_lo[q], 0) (None: 0), hi = min(win_hi[q], M) and lo added to the indices: ascending L2
    distance, ties to the lower index, (-1, inf) where fewer than k rows are admissible, the same +inf / NaN rules and the
    same bits.  1 <= k <= 64.  Any Q in one call (no chunking, no Q x M buffer); a query's result does not depend on the
    others in the call.  No host synchronisation."""
    dev = _lib.require_gpu() if not query.is_cuda else query.device
    lib = _lib.load()
    q, db = _dev(query, dev, torch.float32), _dev(database, dev, torch.float32)
    if q.dim() != 2 or db.dim() != 2 or q.shape[1] != db.shape[1]:
        raise ValueError(f"knn_window: query (Q, D) and database (M, D) expected, got {tuple(q.shape)}, {tuple(db.shape)}")
    nq, m = q.shape[0], db.shape[0]
    hi = _dev(win_hi, dev, torch.int32)
    lo = None if win_lo is None else _dev(win_lo, dev, torch.int32)
    if hi.shape != (nq,) or (lo is not None and lo.shape != (nq,)):
        raise ValueError(f"knn_window: one window per query expected, ({nq},)")
    idx = torch.empty((nq, int(k)), dtype=torch.int32, device=dev)
    dist = torch.empty((nq, int(k)), dtype=torch.float32, device=dev)
    nb = int(lib.egonn_knn_window_scratch_bytes(nq, int(k)))         # -1 on a bad k: the call below raises
    buf = _lib.scratch(nb, dev)
    _lib.call(dev, lib.egonn_knn_window, q.data_ptr(), nq, db.data_ptr(), m, q.shape[1], int(k), _lib._ptr(lo), hi.data_ptr(),
              idx.data_ptr(), dist.data_ptr(), buf.data_ptr(), buf.numel() * 8)
    return idx, dist


def _time_windows(t_db: torch.Tensor, t_q: torch.Tensor, min_gap: float, max_gap: float):
    """float64 device stamps -> (lo, hi, status), nothing synchronised"""
    dev = t_db.device
    lib = _lib.load()
    nq = t_q.shape[0]
    lo = torch.empty(nq, dtype=torch.int32, device=dev)
    hi = torch.empty(nq, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call(dev, lib.egonn_time_windows, t_db.data_ptr(), t_db.shape[0], t_q.data_ptr(), nq, float(min_gap), float(max_gap),
              lo.data_ptr(), hi.data_ptr(), status.data_ptr())
    return lo, hi, status


def time_windows(t_db, t_q, min_gap: float, max_gap: float = math.inf):
    """Stamps of the database (M,) (non-decreasing) and of the queries (Q,) in seconds -> (lo, hi) int32 on the device:
    hi[q] = #{j : t_db[j] <= t_q[q] - min_gap} (inclusive), lo[q] = #{j : t_db[j] < t_q[q] - max_gap} (0 for max_gap = inf).
    The stamps stay float64 on the device: Unix-time stamps 0.1 s apart do not survive fp32.
    Raises ValueError when t_db is not non-decreasing, which is found on the device: this costs ONE host synchronisation."""
    if isinstance(t_db, torch.Tensor) and t_db.is_cuda:
        dev = t_db.device
    elif isinstance(t_q, torch.Tensor) and t_q.is_cuda:
        dev = t_q.device
    else:
        dev = _lib.require_gpu()
    a, b = _dev(t_db, dev, torch.float64), _dev(t_q, dev, torch.float64)
    if a.dim() != 1 or b.dim() != 1:
        raise ValueError("time_windows: t_db (M,) and t_q (Q,) expected")
    lo, hi, status = _time_windows(a, b, min_gap, max_gap)
    if int(status.item()) & 1:                                   # [SYNC]
        raise ValueError("time_windows: t_db is not non-decreasing")
    return lo, hi


def _check_gaps(who: str, k: int, min_gap: float, max_gap: float):
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"{who}: k must be in [1, {MAX_K}], got {k}")
    if not (float(min_gap) > 0.0) or not (float(max_gap) >= float(min_gap)):
        raise ValueError(f"{who}: 0 < min_time_gap <= max_time_gap expected, got {min_gap}, {max_gap} (with no gap a scan is its "
                         f"own nearest neighbour, and the windows are no longer causal)")


def detect_loops(globals: torch.Tensor, times, k: int = 20, min_time_gap: float = 30.0, max_time_gap: float = math.inf) -> Dict:
    """Offline search over a whole trajectory: globals (n, G) descriptors in time order, times (n,) seconds, non-decreasing.
    Scan i is searched against the scans at least min_time_gap (and at most max_time_gap) older than it.
    -> {'nn_index' (n, k) int32 (-1 = none), 'nn_dist' (n, k), 'win_lo' (n,), 'win_hi' (n,)} on the device.
    One host synchronisation (the order check of `time_windows`)."""
    _check_gaps("detect_loops", k, min_time_gap, max_time_gap)
    dev = globals.device if globals.is_cuda else _lib.require_gpu()
    g = _dev(globals, dev, torch.float32)
    t = _dev(times, dev, torch.float64)
    if g.dim() != 2 or t.shape != (g.shape[0],):
        raise ValueError(f"detect_loops: globals (n, G) and times (n,) expected, got {tuple(g.shape)}, {tuple(t.shape)}")
    lo, hi = time_windows(t, t, min_time_gap, max_time_gap)
    idx, dist = knn_window(g, g, k, hi, lo)
    return {"nn_index": idx, "nn_dist": dist, "win_lo": lo, "win_hi": hi}


class LoopDetector:
    """Online loop-closure detection: `push` appends a batch of scans to the map and searches each new scan against the
    entries that are old enough.

    kmap: a `KeypointMap` to adopt (None: one is made from n_k, dim, global_dim on `device`; a map that already holds
    entries needs their `times`); k: candidates per scan (<= 64); min_time_gap / max_time_gap: the admissible age in
    seconds; verify: register every candidate from its keypoints (`verify_candidates`) and keep the one with the most
    inliers; min_inliers, ransac_dist_th, ransac_max_it, seed: passed on to it, and verify_method as its `method` ("ransac" or
    "spectral").

    min_inliers = 0 means: the best candidate with a model wins.  No threshold for real data can be derived here (there are
    neither trained weights nor a dataset in this project); pick one from the inlier counts of wrong candidates on your data,
    for instance from the curve of `evaluate_loop_closure(score=-best_inliers, predicted=best_index)`.

    Pushing a trajectory in batches of any size gives, entry for entry, the bits of one offline `detect`: the windows are
    causal (the stamps never decrease, and min_time_gap > 0 keeps an entry's window in front of it), the pair ids of the
    RANSAC draws come from the entries' global indices, and `knn_window` does not depend on the batch."""

    def __init__(self, kmap: Optional[KeypointMap] = None, k: int = 20, min_time_gap: float = 30.0, max_time_gap: float = math.inf,
                 verify: bool = True, min_inliers: int = 0, ransac_dist_th: float = 0.5, ransac_max_it: int = 10000, seed: int = 0,
                 n_k: int = 128, dim: int = 128, global_dim: int = 256, device=None, times=None, verify_method: str = "ransac"):
        _check_gaps("LoopDetector", k, min_time_gap, max_time_gap)
        self.verify_method = check_method("LoopDetector(verify_method)", verify_method)
        self.kmap = KeypointMap(n_k, dim, global_dim, device) if kmap is None else kmap
        self.k, self.min_time_gap, self.max_time_gap = int(k), float(min_time_gap), float(max_time_gap)
        self.verify, self.min_inliers = bool(verify), int(min_inliers)
        self.ransac_dist_th, self.ransac_max_it, self.seed = ransac_dist_th, ransac_max_it, seed
        have = np.zeros(0) if times is None else np.asarray(times, dtype=np.float64).reshape(-1)
        if len(have) != len(self.kmap):
            raise ValueError(f"LoopDetector: the map holds {len(self.kmap)} entries, `times` {len(have)}")
        self._check_times(have, -math.inf)
        self._last = float(have[-1]) if len(have) else -math.inf
        self._times = torch.zeros(max(len(have), 64), dtype=torch.float64, device=self.kmap.device)
        self._times[: len(have)] = torch.from_numpy(have)

    @staticmethod
    def _check_times(t: np.ndarray, last: float):
        if len(t) and (not np.isfinite(t).all() or t[0] < last or (np.diff(t) < 0).any()):
            raise ValueError("LoopDetector: times must be finite and continue non-decreasing")

    def __len__(self):
        return len(self.kmap)

    times = property(lambda self: self._times[: len(self.kmap)])

    def push(self, out: Dict[str, torch.Tensor], times, poses=None) -> Dict[str, torch.Tensor]:
        """out: the extractor's dict of the b new scans ('global', 'keypoints', 'descriptors' [, 'count'], as `KeypointMap.add`
        takes it); times (b,) seconds on the host, continuing non-decreasing (ValueError otherwise, before the map is changed);
        poses (b,4,4) or None (identity: `pose` of the result is then meaningless, T_rel is not).

        The batch is appended, the windows of its entries are computed against the map INCLUDING the batch, and the entries
        are searched (`knn_window`) and, with verify, registered against their candidates with query_ids = their global
        indices.  -> the dict of `verify_candidates` (per pair (b, k, ...), per query (b, ...); absent with verify=False) plus
        nn_index (b, k), nn_dist, index (b,) global ids, win_lo, win_hi and loop (b,) bool: best_index >= 0, or with
        verify=False whether a candidate exists.  Nothing is synchronised."""
        t = np.asarray(times.cpu() if isinstance(times, torch.Tensor) else times, dtype=np.float64).reshape(-1)
        if not len(t):
            raise ValueError("LoopDetector.push: an empty batch")
        self._check_times(t, self._last)
        km, dev = self.kmap, self.kmap.device
        start, b = len(km), len(t)
        km.add(out, np.tile(np.eye(4), (b, 1, 1)) if poses is None else poses)
        if len(km) != start + b:
            raise ValueError(f"LoopDetector.push: {b} stamps for {len(km) - start} scans")
        if start + b > self._times.shape[0]:
            grown = torch.zeros(max(start + b, self._times.shape[0] * 3 // 2), dtype=torch.float64, device=dev)
            grown[:start] = self._times[:start]
            self._times = grown
        self._times[start: start + b] = torch.from_numpy(t)
        self._last = float(t[-1])
        t_db = self._times[: start + b]
        lo, hi, _ = _time_windows(t_db, t_db[start:], self.min_time_gap, self.max_time_gap)     # the order was checked on the host
        nn, dist = knn_window(km.globals[start:], km.globals, self.k, hi, lo)
        index = torch.arange(start, start + b, dtype=torch.int32, device=dev)
        r: Dict[str, torch.Tensor] = {}
        if self.verify:
            r = verify_candidates(km.descriptors[start:], km.keypoints[start:], km.counts[start:], km, nn, query_ids=index,
                                  min_inliers=self.min_inliers, ransac_dist_th=self.ransac_dist_th,
                                  ransac_max_it=self.ransac_max_it, seed=self.seed, method=self.verify_method)
        r.update(nn_index=nn, nn_dist=dist, index=index, win_lo=lo, win_hi=hi,
                 loop=(r["best_index"] >= 0) if self.verify else (nn[:, 0] >= 0))
        return r

    def detect(self, outs: Dict[str, torch.Tensor], times, poses=None) -> Dict[str, torch.Tensor]:
        """the offline form: the whole trajectory in one `push` on an empty detector"""
        if len(self.kmap):
            raise ValueError("LoopDetector.detect: the detector already holds entries; use push")
        return self.push(outs, times, poses)


def evaluate_loop_closure(nn_index, score, positions, win_lo, win_hi, revisit_radius: float, predicted=None) -> Dict:
    """Precision/recall of a loop-closure detector over one trajectory of n scans.

    nn_index (n, k) candidates and win_lo / win_hi (n,) as `detect_loops` or `LoopDetector` return them; score (n,): the
    confidence of each scan's prediction, LOWER = more confident (+inf / NaN = no prediction), e.g. nn_dist[:, 0]; positions
    (n, 2 | 3) float64; predicted (n,) = the predicted revisit of each scan, default nn_index[:, 0] (a scan whose prediction is
    < 0 predicts nothing whatever its score).  Pass predicted = best_index and score = -best_inliers to grade the verified
    detector.

    Per scan at threshold tau (the single-trajectory convention of LoGG3D-Net and OverlapTransformer): predicted iff
    score <= tau; TP = predicted and the predicted scan lies within revisit_radius; FP = predicted and not that; FN = not
    predicted although an admissible scan lies within revisit_radius; TN otherwise.  The curve has one point per distinct score.
    -> precision, recall, thresholds, tp, fp, fn (numpy, ascending threshold), f1_max and f1_threshold (0, -inf without a
    point), average_precision = sum (R_n - R_{n-1}) P_n with R_0 = 0, recall_at_full_precision = the largest recall among points
    of precision exactly 1 (0 if none), extended_precision = (precision of the first point + recall_at_full_precision) / 2,
    n_revisit, n_predicted, and the device tensors count (admissible scans within the radius) and pred_dist.
    recall is 0 where TP + FN = 0 (no revisit at all).  One host synchronisation, at the end."""
    n = int(torch.as_tensor(score).shape[0]) if torch.as_tensor(score).dim() == 1 else -1
    pos64 = torch.as_tensor(np.asarray(positions.cpu() if isinstance(positions, torch.Tensor) else positions, dtype=np.float64))
    nn_t = torch.as_tensor(nn_index) if predicted is None else None
    pred_t = torch.as_tensor(predicted) if predicted is not None else None
    shapes_ok = n >= 0 and pos64.dim() == 2 and pos64.shape[0] == n and pos64.shape[1] in (2, 3) and \
        tuple(torch.as_tensor(win_lo).shape) == (n,) and tuple(torch.as_tensor(win_hi).shape) == (n,) and \
        (pred_t is None or tuple(pred_t.shape) == (n,)) and (nn_t is None or (nn_t.dim() == 2 and nn_t.shape[0] == n and nn_t.shape[1] >= 1))
    if not shapes_ok:
        raise ValueError("evaluate_loop_closure: score (n,), positions (n, 2 | 3), win_lo (n,), win_hi (n,) and nn_index (n, k) or "
                         "predicted (n,) must agree in n")
    if not float(revisit_radius) >= 0.0:
        raise ValueError("evaluate_loop_closure: revisit_radius must be non-negative")
    src = nn_t if pred_t is None else pred_t
    dev = src.device if src.is_cuda else _lib.require_gpu()
    lib = _lib.load()
    # positions stay float64 up to here: MulRan / KITTI poses are UTM-scale (~4e6 m), where fp32 resolves 0.25-0.5 m — enough
    # to flip a neighbour at the revisit radius.  A common origin is subtracted in float64 first, the device then works on
    # metre-scale offsets.
    origin = pos64.mean(dim=0, keepdim=True) if n else torch.zeros((1, pos64.shape[1]), dtype=torch.float64)
    pos = (pos64 - origin).to(device=dev, dtype=torch.float32).contiguous()
    pred = _dev(nn_t[:, 0] if pred_t is None else pred_t, dev, torch.int32)
    lo, hi = _dev(win_lo, dev, torch.int32), _dev(win_hi, dev, torch.int32)
    sc = _dev(score, dev, torch.float32)
    sc = torch.where(pred < 0, torch.full_like(sc, math.inf), sc)          # no candidate: no prediction
    i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)                # noqa: E731
    count, pred_dist = i32(), torch.empty(n, dtype=torch.float32, device=dev)
    _lib.call(dev, lib.egonn_window_radius, pos.data_ptr(), n, pos.data_ptr(), n, pos.shape[1], lo.data_ptr(), hi.data_ptr(),
              C.c_float(float(revisit_radius)), pred.data_ptr(), count.data_ptr(), pred_dist.data_ptr())
    correct = (pred_dist <= float(np.float32(revisit_radius))).to(torch.int32)
    revisit = (count > 0).to(torch.int32)
    order, ctp, cfp, crev = i32(), i32(), i32(), i32()
    gend = torch.empty(n, dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    nb = int(lib.egonn_pr_curve_scratch_bytes(n))
    buf = torch.empty(max(nb, 256) + 256, dtype=torch.uint8, device=dev)
    off = (-buf.data_ptr()) % 256                                               # the sort's carves are 256-byte aligned
    _lib.call(dev, lib.egonn_pr_curve, sc.data_ptr(), correct.data_ptr(), revisit.data_ptr(), n, order.data_ptr(), ctp.data_ptr(),
              cfp.data_ptr(), crev.data_ptr(), gend.data_ptr(), totals.data_ptr(), buf.data_ptr() + off, nb)
    h = {name: t.cpu().numpy() for name, t in (("order", order), ("tp", ctp), ("fp", cfp), ("rev", crev), ("end", gend),
                                               ("totals", totals), ("score", sc))}                # [SYNC]
    res = curve_metrics(h["tp"], h["fp"], h["rev"], h["end"], int(h["totals"][1]))
    at = np.flatnonzero(h["end"])
    res["thresholds"] = h["score"][h["order"][at]].astype(np.float64)
    best = res.pop("_f1_at")
    res["f1_threshold"] = float(res["thresholds"][best]) if len(at) else -math.inf
    res.update(n_predicted=int(h["totals"][0]), count=count, pred_dist=pred_dist)
    return res


def curve_metrics(cum_tp, cum_fp, cum_rev, group_end, n_revisit: int) -> Dict:
    """the float64 host part of `evaluate_loop_closure`, from the integer arrays of egonn_pr_curve"""
    at = np.flatnonzero(np.asarray(group_end))
    tp, fp = np.asarray(cum_tp)[at].astype(np.float64), np.asarray(cum_fp)[at].astype(np.float64)
    fn = float(n_revisit) - np.asarray(cum_rev)[at].astype(np.float64)
    precision = tp / (tp + fp)                                                  # a point has at least one prediction
    den = tp + fn
    recall = np.divide(tp, den, out=np.zeros_like(tp), where=den > 0)
    f1 = 2.0 * tp / (2.0 * tp + fp + fn)
    full = recall[precision == 1.0]
    r_full = float(full.max()) if len(full) else 0.0
    res = {"precision": precision, "recall": recall, "tp": tp.astype(np.int64), "fp": fp.astype(np.int64), "fn": fn.astype(np.int64),
           "f1_max": float(f1.max()) if len(at) else 0.0, "_f1_at": int(f1.argmax()) if len(at) else -1,
           "average_precision": float(np.sum(np.diff(recall, prepend=0.0) * precision)),
           "recall_at_full_precision": r_full,
           "extended_precision": 0.5 * ((float(precision[0]) if len(at) else 0.0) + r_full), "n_revisit": int(n_revisit)}
    return res
