"""Pairwise-consistency filter for loop edges, between `loop_edges` and `optimize_trajectory`.

Two loop closures taken close together in time must agree with each other through the odometry between them; a false one
agrees with nobody.  `filter_loops` keeps the edges that at least `min_support` other kept edges agree with and returns the
loop dict with the weights of the others set to 0, so the edge count stays static: no synchronisation, no compaction.
The contract is stated once in csrc/loop_consistency.hip and DESIGN.md §3.18.  All device arithmetic runs in libegonn_hip;
there is no torch or numpy fallback.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import as_dev as _dev
from .pose_graph import _aligned, _check_shapes, _device, _stage

TRUNCATED, ROUNDS = 1, 2
MAX_PARTNERS = MAX_ROUNDS = 1 << 16


def _loop_parts(who: str, loops):
    try:
        return loops["edge_index"], loops["Z"], loops["weights"]
    except (KeyError, TypeError, IndexError):
        raise ValueError(f"{who}: loops = a dict of edge_index (E,2), Z (E,4,4), weights (E,2) expected, as loop_edges returns") from None


def filter_loops(poses, loops: Dict, window: int = 16, trans_thr: float = 1.0, rot_thr: float = 0.1, trans_drift: float = 0.0,
                 rot_drift: float = 0.0, min_support: int = 2, max_rounds: int = 16, max_partners: int = 256,
                 out: Optional[Dict] = None) -> Dict:
    """poses (n,4,4): the drifting, odometry-integrated trajectory; loops: `loop_edges(...)` (or any dict of edge_index (E,2) =
    (a, b), Z (E,4,4) ~ X_a^-1 X_b, weights (E,2)).  Two live edges are comparable when their a's and their b's are at most
    `window` index steps apart (and they are at most max_partners / 2 places apart among the live edges ordered by b), and
    consistent when the cycle C = Z_e (X_be^-1 X_bf) Z_f^-1 (X_af^-1 X_ae) has |t_C| <= trans_thr + trans_drift g and
    |Log R_C| <= rot_thr + rot_drift g, g = |b_e - b_f| + |a_e - a_f|.  Kept: the min_support-core of that graph, computed in at
    most max_rounds synchronous rounds.  An edge never counts itself; two duplicate edges do count each other, so a false loop
    reported twice survives min_support = 1.  The defaults are choices, not tuned values: the project has neither trained
    weights nor a dataset to tune them on.
    -> {'keep' (E,) bool, 'support0' (E,) int32 before any removal, 'support' (E,) int32 among the survivors, 'weights' (E,2) =
    the input weights * keep, 'edge_index', 'Z' (passed through: the dict is a drop-in for `loops` in optimize_trajectory),
    'rounds' () rounds that removed something, 'edge_status' (E,) (the pose graph's bits; an edge with a bit, or with both
    weights 0, is dead: it never votes and is not kept), 'status' (1,): TRUNCATED | ROUNDS} on the device, no host
    synchronisation.  out = a dict this function returned for the same shapes: nothing is allocated (see optimize_pose_graph
    for the staging of inputs that are not contiguous device tensors of their dtype: float64, edge_index int32)."""
    who = "filter_loops"
    edge_index, Z, weights = _loop_parts(who, loops)
    n, E = _check_shapes(who, *(torch.as_tensor(x) for x in (poses, edge_index, Z, weights)))
    window, min_support, max_rounds, max_partners = int(window), int(min_support), int(max_rounds), int(max_partners)
    if window < 0:
        raise ValueError(f"{who}: window={window} must not be negative")
    for name, v in (("trans_thr", trans_thr), ("rot_thr", rot_thr), ("trans_drift", trans_drift), ("rot_drift", rot_drift)):
        if not (0.0 <= float(v) < math.inf):
            raise ValueError(f"{who}: {name}={v} must be non-negative and finite")
    if min_support < 1:
        raise ValueError(f"{who}: min_support={min_support} must be positive")
    if not 1 <= max_rounds <= MAX_ROUNDS:
        raise ValueError(f"{who}: max_rounds={max_rounds} outside [1, {MAX_ROUNDS}]")
    if max_partners < 64 or max_partners % 64 or max_partners > MAX_PARTNERS:
        raise ValueError(f"{who}: max_partners={max_partners} must be a positive multiple of 64 (up to {MAX_PARTNERS})")
    dev = _device(poses, edge_index, Z)
    lib = _lib.load()
    reuse = out is not None
    if reuse and ("_rounds" not in out or out["keep"].shape != (E,)):
        raise ValueError(f"{who}: `out` was made for other shapes")
    store = out["_in"] if reuse else {}
    X = _stage(who, "poses", poses, dev, torch.float64, store, reuse)
    Zd = _stage(who, "Z", Z, dev, torch.float64, store, reuse)
    ei = _stage(who, "edge_index", edge_index, dev, torch.int32, store, reuse)
    w = _stage(who, "weights", weights, dev, torch.float64, store, reuse)
    nb = int(lib.egonn_loop_consistency_scratch_bytes(E, max_partners))
    if nb < 0:
        raise ValueError(f"{who}: E={E}, max_partners={max_partners} are out of range")
    if not reuse:
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)                     # noqa: E731
        out = {"keep": torch.empty(E, dtype=torch.bool, device=dev), "support0": i32(E), "support": i32(E),
               "weights": torch.empty((E, 2), dtype=torch.float64, device=dev), "_rounds": i32(1), "edge_status": i32(E),
               "status": i32(1), "_scratch": _aligned(nb, dev), "_in": store}
        out["rounds"] = out["_rounds"][0]
    elif out["_scratch"].numel() < nb or out["_scratch"].data_ptr() % 256:
        raise ValueError(f"{who}: `out` was made for other shapes (max_partners)")
    _lib.call(dev, lib.egonn_loop_consistency, X.data_ptr(), n, ei.data_ptr(), Zd.data_ptr(), w.data_ptr(), E, window, float(trans_thr),
              float(rot_thr), float(trans_drift), float(rot_drift), min_support, max_rounds, max_partners, out["keep"].data_ptr(),
              out["support0"].data_ptr(), out["support"].data_ptr(), out["weights"].data_ptr(), out["_rounds"].data_ptr(),
              out["edge_status"].data_ptr(), out["status"].data_ptr(), out["_scratch"].data_ptr(), out["_scratch"].numel())
    out.update(edge_index=ei, Z=Zd, _keep=(X, Zd, ei, w))                 # inputs of enqueued work stay alive with the result
    return out


def loop_cycle_errors(poses, loops: Dict, pairs) -> torch.Tensor:
    """pairs (P,2): rows of the loop dict -> (P,2) = (c_trans, c_rot) of the cycle of each pair, evaluated in the canonical role
    (the edge that comes first by (b, row) plays e), so (e, f) and (f, e) give the same bits.  A pair that is out of range or
    names an edge with a status bit gives NaN (the weights are not looked at).  The test seam of the filter's arithmetic."""
    who = "loop_cycle_errors"
    edge_index, Z, weights = _loop_parts(who, loops)
    n, E = _check_shapes(who, *(torch.as_tensor(x) for x in (poses, edge_index, Z, weights)))
    pr = torch.as_tensor(pairs)
    if pr.dim() != 2 or pr.shape[1] != 2:
        raise ValueError(f"{who}: pairs (P, 2) expected, got {tuple(pr.shape)}")
    dev = _device(poses, edge_index, Z)
    X, Zd, ei = _dev(poses, dev, torch.float64), _dev(Z, dev, torch.float64), _dev(edge_index, dev, torch.int32)
    pr = _dev(pr, dev, torch.int32)
    res = torch.empty((pr.shape[0], 2), dtype=torch.float64, device=dev)
    _lib.call(dev, _lib.load().egonn_loop_cycle_errors, X.data_ptr(), n, ei.data_ptr(), Zd.data_ptr(), E, pr.data_ptr(), pr.shape[0],
              res.data_ptr())
    return res
