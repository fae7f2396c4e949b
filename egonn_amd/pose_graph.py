"""Pose-graph optimisation on the device: the corrected trajectory behind the loop detector.

`LoopDetector.push` returns verified revisits with their 6-DoF relative pose, `icp_pairs` / `relative_poses` the odometry;
`optimize_pose_graph` closes the loops: Levenberg-Marquardt over poses X_i = [R_i | t_i] with edges Z_e ~ X_a^-1 X_b, a
matrix-free block-Jacobi preconditioned conjugate-gradient solve inside, float64, deterministic, with no host synchronisation
(the whole call can be captured).  The contract is stated once in csrc/pose_graph.hip and DESIGN.md §3.16.
All device arithmetic runs in libegonn_hip; there is no torch or numpy fallback.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import as_dev as _dev

BAD_INDEX, SELF_LOOP, NONFINITE, NEGATIVE_WEIGHT, ANGLE, ISOLATED, PIVOT = 1, 2, 4, 8, 16, 32, 64


def _device(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return _lib.require_gpu()


def _check_shapes(who: str, poses, edge_index, Z, weights, fixed=None):
    """shape checks on anything with a .shape: nothing here needs a device"""
    ps, es, zs = tuple(poses.shape), tuple(edge_index.shape), tuple(Z.shape)
    if len(ps) != 3 or ps[1:] != (4, 4) or ps[0] < 1:
        raise ValueError(f"{who}: poses (n, 4, 4) with n >= 1 expected, got {ps}")
    if len(es) != 2 or es[1] != 2:
        raise ValueError(f"{who}: edge_index (E, 2) expected, got {es}")
    if zs != (es[0], 4, 4):
        raise ValueError(f"{who}: Z ({es[0]}, 4, 4) expected, got {zs}")
    if weights is not None and tuple(weights.shape) != (es[0], 2):
        raise ValueError(f"{who}: weights ({es[0]}, 2) = (w_rot, w_trans) per edge expected, got {tuple(weights.shape)}")
    if fixed is not None and tuple(fixed.shape) != (ps[0],):
        raise ValueError(f"{who}: fixed ({ps[0]},) expected, got {tuple(fixed.shape)}")
    return ps[0], es[0]


def _aligned(nbytes: int, dev) -> torch.Tensor:
    """a 256-byte aligned span of at least nbytes as a uint8 view"""
    buf = torch.empty(max(int(nbytes), 256) + 256, dtype=torch.uint8, device=dev)
    off = (-buf.data_ptr()) % 256
    return buf[off: off + max(int(nbytes), 256)]


def _stage(who: str, name: str, x, dev, dtype, store: Dict, reuse: bool) -> torch.Tensor:
    """An input as a contiguous tensor of `dtype` on `dev`.  One that is that already is used as it is.  Any other is converted
    into a staging buffer owned by `store` (the result dict keeps it, so enqueued and captured work never reads freed memory):
    made on the first call, and with reuse (a call with out=) filled by one copy_, which allocates nothing; a call with out=
    whose input needs a staging buffer that the first call did not make is refused."""
    t = torch.as_tensor(x)
    if t.device == dev and t.dtype == dtype and t.is_contiguous():
        return t
    buf = store.get(name)
    if reuse:
        if buf is None or buf.shape != t.shape:
            raise ValueError(f"{who}: with out=, `{name}` must be a contiguous {dtype} tensor on {dev}, or of the kind and shape "
                             f"that the call which made `out` converted (its staging buffer is used again)")
        buf.copy_(t)
        return buf
    buf = store[name] = t.to(device=dev, dtype=dtype).contiguous()
    return buf


class _Graph:
    """the inputs on the device, the scratch span and the plan's outputs of one (n, E)"""

    def __init__(self, who, poses, edge_index, Z, weights, fixed, pcg_iterations=1, out=None):
        shapes = [torch.as_tensor(x) if x is not None else None for x in (poses, edge_index, Z, weights, fixed)]
        self.n, self.E = _check_shapes(who, *shapes)
        dev = self.dev = _device(poses, edge_index, Z)
        self.lib = _lib.load()
        reuse = out is not None
        store = self.store = out["_in"] if reuse else {}
        st = lambda name, x, dt: None if x is None else _stage(who, name, x, dev, dt, store, reuse)       # noqa: E731
        self.poses, self.Z, self.edges = st("poses", poses, torch.float64), st("Z", Z, torch.float64), st("edge_index", edge_index, torch.int32)
        self.weights = st("weights", weights, torch.float64)
        self.fixed = st("fixed", fixed, torch.bool)                        # one byte per node, non-zero = fixed
        nb = int(self.lib.egonn_pose_graph_scratch_bytes(self.n, self.E, int(pcg_iterations)))
        if nb < 0:
            raise ValueError(f"{who}: n={self.n}, E={self.E}, pcg_iterations={pcg_iterations} are out of range")
        if not reuse:
            self.scratch = _aligned(nb, dev)
            self.edge_status = torch.empty(self.E, dtype=torch.int32, device=dev)
            self.status = torch.empty(1, dtype=torch.int32, device=dev)
        else:
            self.scratch, self.edge_status, self.status = out["_scratch"], out["edge_status"], out["status"]
            if self.scratch.numel() < nb or self.scratch.data_ptr() % 256 or self.edge_status.shape != (self.E,):
                raise ValueError(f"{who}: `out` was made for other shapes")
        self.span = (self.scratch.data_ptr(), self.scratch.numel())
        self.inputs = (self.poses, self.Z, self.edges, self.weights, self.fixed)

    def plan(self):
        _lib.call(self.dev, self.lib.egonn_pose_graph_plan, self.edges.data_ptr(), self.Z.data_ptr(), _lib._ptr(self.weights),
                  _lib._ptr(self.fixed), self.n, self.E, self.edge_status.data_ptr(), self.status.data_ptr(), *self.span)


def pose_graph_cost(poses, edge_index, Z, weights=None, robust_delta: float = 0.0) -> Dict[str, torch.Tensor]:
    """poses (n,4,4), edge_index (E,2) = (a, b), Z (E,4,4) ~ X_a^-1 X_b, weights (E,2) = (w_rot, w_trans) (None: 1)
    -> {'cost' (), 'residuals' (E,6) = [t_E ; Log R_E], 'rho' (E,), 's' (E,), 'gradient' (n,6) in (v, w) order for every node,
    'edge_status' (E,), 'status' (1,)} on the device.  No host synchronisation."""
    g = _Graph("pose_graph_cost", poses, edge_index, Z, weights, None)
    dev, n, E = g.dev, g.n, g.E
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)                  # noqa: E731
    cost, res, rho, s, grad = f64(1), f64(E, 6), f64(E), f64(E), f64(n, 6)
    g.plan()
    _lib.call(dev, g.lib.egonn_pose_graph_cost, g.poses.data_ptr(), n, E, g.Z.data_ptr(), float(robust_delta), cost.data_ptr(),
              res.data_ptr(), rho.data_ptr(), s.data_ptr(), grad.data_ptr(), g.edge_status.data_ptr(), *g.span)
    return {"cost": cost[0], "residuals": res, "rho": rho, "s": s, "gradient": grad, "edge_status": g.edge_status, "status": g.status,
            "_keep": g.inputs + (g.scratch,)}


def pose_graph_hessvec(poses, edge_index, Z, p, weights=None, fixed=None, damping: float = 0.0, robust_delta: float = 0.0):
    """(J^T W J + damping I) p on the free nodes, (n,6): the product the solver iterates with (rows of fixed nodes are 0, their
    p is ignored).  The test seam of the solver."""
    g = _Graph("pose_graph_hessvec", poses, edge_index, Z, weights, fixed)
    pv = _dev(p, g.dev, torch.float64)
    if tuple(pv.shape) != (g.n, 6):
        raise ValueError(f"pose_graph_hessvec: p ({g.n}, 6) expected, got {tuple(pv.shape)}")
    out = torch.empty((g.n, 6), dtype=torch.float64, device=g.dev)
    g.plan()
    _lib.call(g.dev, g.lib.egonn_pose_graph_hessvec, g.poses.data_ptr(), g.n, g.E, g.Z.data_ptr(), float(robust_delta), float(damping),
              pv.data_ptr(), out.data_ptr(), g.edge_status.data_ptr(), *g.span)
    return out


def optimize_pose_graph(poses, edge_index, Z, weights=None, fixed=None, max_iterations: int = 10, pcg_iterations: int = 200,
                        robust_delta: float = 0.0, out: Optional[Dict] = None, pcg_tol: float = 1e-8, lambda_init: float = 1e-4,
                        lambda_min: float = 1e-10, lambda_max: float = 1e10, rel_tol: float = 0.0, grad_tol: float = 0.0) -> Dict:
    """Levenberg-Marquardt over the poses; fixed (n,) bool: the gauge (None: node 0).  Every outer step enqueues exactly
    pcg_iterations conjugate-gradient iterations (two launches each) whether or not they are needed; block-Jacobi moves a
    correction about one node per iteration along an odometry chain, so a long loop needs a budget of the order of its length.
    -> {'poses' (n,4,4), 'cost_trace' (max_iterations + 1,) NaN after the stop, 'accept_trace' (max_iterations,) 1 / 0 / -1,
    'iterations' (), 'accepted' (), 'lambda' (), 'status' (1,), 'edge_status' (E,)} on the device; fixed nodes and nodes without a
    live edge come out bit-equal.  No host synchronisation.  out = a dict this function returned for the same shapes and
    budgets: every buffer is used again and nothing is allocated, which a capture through egonn_graph_begin / _end needs.
    Inputs that are contiguous device tensors of their dtype (float64; edge_index int32; fixed bool) are read where they are
    (keep them alive as long as a captured graph); any other input is copied into a staging buffer that `out` owns, so the
    call that made `out` must have been given inputs of the same kind."""
    max_iterations, pcg_iterations = int(max_iterations), int(pcg_iterations)
    if max_iterations < 1 or pcg_iterations < 1:
        raise ValueError(f"optimize_pose_graph: max_iterations={max_iterations} and pcg_iterations={pcg_iterations} must be positive")
    for name, v in (("robust_delta", robust_delta), ("pcg_tol", pcg_tol), ("rel_tol", rel_tol), ("grad_tol", grad_tol)):
        if not (0.0 <= float(v) < math.inf):
            raise ValueError(f"optimize_pose_graph: {name}={v} must be non-negative and finite")
    g = _Graph("optimize_pose_graph", poses, edge_index, Z, weights, fixed, pcg_iterations, out)
    dev, n = g.dev, g.n
    if out is None:
        out = {"poses": torch.empty((n, 4, 4), dtype=torch.float64, device=dev),
               "cost_trace": torch.empty(max_iterations + 1, dtype=torch.float64, device=dev),
               "accept_trace": torch.empty(max_iterations, dtype=torch.int32, device=dev),
               "_counters": torch.empty(2, dtype=torch.int32, device=dev), "_lambda": torch.empty(1, dtype=torch.float64, device=dev),
               "status": g.status, "edge_status": g.edge_status, "_scratch": g.scratch, "_in": g.store}
        out.update(iterations=out["_counters"][0], accepted=out["_counters"][1])
        out["lambda"] = out["_lambda"][0]
    elif out["poses"].shape != (n, 4, 4) or out["cost_trace"].shape != (max_iterations + 1,):
        raise ValueError("optimize_pose_graph: `out` was made for other shapes")
    g.plan()
    _lib.call(dev, g.lib.egonn_pose_graph_optimize, g.poses.data_ptr(), n, g.E, g.Z.data_ptr(), float(robust_delta), max_iterations,
              pcg_iterations, float(pcg_tol), float(lambda_init), float(lambda_min), float(lambda_max), float(rel_tol),
              float(grad_tol), out["poses"].data_ptr(), out["cost_trace"].data_ptr(), out["accept_trace"].data_ptr(),
              out["_counters"].data_ptr(), out["_lambda"].data_ptr(), g.edge_status.data_ptr(), g.status.data_ptr(), *g.span)
    out["_keep"] = g.inputs                                  # inputs of enqueued work stay alive with the result
    return out


def _odometry_into(X: torch.Tensor, Z: torch.Tensor, edges: torch.Tensor):
    """X (n,4,4) float64 on the device -> Z[:n-1], edges[:n-1] filled in place by egonn_pose_graph_odometry"""
    _lib.call(X.device, _lib.load().egonn_pose_graph_odometry, X.data_ptr(), X.shape[0], Z.data_ptr(), edges.data_ptr())


def odometry_edges(poses, weight=(1.0, 1.0)) -> Dict[str, torch.Tensor]:
    """poses (n,4,4) -> the chain i -> i + 1 with Z = X_i^-1 X_{i+1}, computed on the device:
    {'edge_index' (n-1,2) int32, 'Z' (n-1,4,4), 'weights' (n-1,2)}"""
    shape = tuple(getattr(poses, "shape", ()))
    if len(shape) != 3 or shape[1:] != (4, 4) or shape[0] < 1:
        raise ValueError(f"odometry_edges: poses (n, 4, 4) with n >= 1 expected, got {shape}")
    wr, wt = _weight_pair("odometry_edges", weight)
    dev = _device(poses)
    X = _dev(poses, dev, torch.float64)
    m = X.shape[0] - 1
    Z = torch.empty((m, 4, 4), dtype=torch.float64, device=dev)
    edges = torch.empty((m, 2), dtype=torch.int32, device=dev)
    _odometry_into(X, Z, edges)
    w = torch.empty((m, 2), dtype=torch.float64, device=dev)
    w[:, 0], w[:, 1] = wr, wt
    return {"edge_index": edges, "Z": Z, "weights": w, "_keep": (X,)}


def _weight_pair(who: str, weight):
    try:
        wr, wt = (float(v) for v in weight)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: weight = (w_rot, w_trans) expected, got {weight!r}") from None
    if not (0.0 <= wr < math.inf and 0.0 <= wt < math.inf):
        raise ValueError(f"{who}: weight = (w_rot, w_trans) must be non-negative and finite, got {weight!r}")
    return wr, wt


def loop_edges(result: Dict[str, torch.Tensor], weight=(1.0, 1.0)) -> Dict[str, torch.Tensor]:
    """The dict of `LoopDetector.push` / `detect` (verify=True) -> one edge per pushed scan, so the count is static:
    a = best_index, b = index, Z = T_rel (pose_b = pose_a @ T_rel), weight (w_rot, w_trans) where `loop` is true and 0 where it
    is not (a = -1 there: the plan also reports such an edge as BAD_INDEX, and it is off either way).  No synchronisation, no
    compaction."""
    wr, wt = _weight_pair("loop_edges", weight)
    missing = [k for k in ("best_index", "index", "T_rel", "loop") if k not in result]
    if missing:
        raise ValueError(f"loop_edges: the result of LoopDetector.push with verify=True expected; it lacks {missing}")
    a, b, T, loop = result["best_index"], result["index"], result["T_rel"], result["loop"]
    m = tuple(b.shape)[0] if len(tuple(b.shape)) == 1 else -1
    if m < 0 or tuple(a.shape) != (m,) or tuple(T.shape) != (m, 4, 4) or tuple(loop.shape) != (m,):
        raise ValueError("loop_edges: best_index (b,), index (b,), T_rel (b,4,4) and loop (b,) must agree in b")
    w = torch.zeros((m, 2), dtype=torch.float64, device=T.device)
    w[:, 0], w[:, 1] = wr, wt
    w = w * loop.to(torch.float64).unsqueeze(1)
    return {"edge_index": torch.stack([a.to(torch.int32), b.to(torch.int32)], dim=1), "Z": T.to(torch.float64), "weights": w}


def optimize_trajectory(poses, loops: Dict[str, torch.Tensor], odometry: Optional[Dict[str, torch.Tensor]] = None,
                        odometry_weight=(1.0, 1.0), out: Optional[Dict] = None, consistency: Optional[Dict] = None, **kw) -> Dict:
    """poses (n,4,4): the drifting trajectory; loops: `loop_edges(...)` (or any dict of edge_index, Z, weights); odometry: such
    a dict too, e.g. ICP-refined relative poses of consecutive scans, default: the chain of `odometry_edges(poses,
    odometry_weight)`.  The two edge sets are written one behind the other into buffers the result owns ('edge_index', 'Z',
    'weights'; 'n_odometry' = the length of the first) and `optimize_pose_graph(**kw)` runs on them.  out = a result of this
    function for the same shapes: the buffers are filled again by copies and nothing is allocated (see optimize_pose_graph).
    consistency: a dict of `filter_loops` keywords ({} = its defaults): the loops go through the pairwise-consistency filter
    first (loop_consistency.py), its result is kept under 'consistency' and its buffers are used again with out=; None: no
    filter, and nothing of it runs."""
    who = "optimize_trajectory"
    shape = tuple(getattr(poses, "shape", ()))
    if len(shape) != 3 or shape[1:] != (4, 4) or shape[0] < 1:
        raise ValueError(f"{who}: poses (n, 4, 4) with n >= 1 expected, got {shape}")
    wr, wt = _weight_pair(who, odometry_weight)
    m_od = shape[0] - 1 if odometry is None else int(odometry["Z"].shape[0])
    m = m_od + int(loops["Z"].shape[0])
    reuse = out is not None
    if reuse:
        if "_traj_in" not in out or out["Z"].shape != (m, 4, 4) or out["n_odometry"] != m_od:
            raise ValueError(f"{who}: `out` was made for other shapes")
        store, dev = out["_traj_in"], out["Z"].device
        edges, Z, w = out["edge_index"], out["Z"], out["weights"]
    else:
        store, dev = {}, _device(poses, loops["Z"])
        edges = torch.empty((m, 2), dtype=torch.int32, device=dev)
        Z = torch.empty((m, 4, 4), dtype=torch.float64, device=dev)
        w = torch.empty((m, 2), dtype=torch.float64, device=dev)
    X = _stage(who, "poses", poses, dev, torch.float64, store, reuse)
    if consistency is not None:
        from .loop_consistency import filter_loops
        if reuse and "consistency" not in out:
            raise ValueError(f"{who}: `out` was made without consistency=")
        loops = filtered = filter_loops(X, loops, out=out["consistency"] if reuse else None, **consistency)
    if odometry is None:
        _odometry_into(X, Z, edges)
        w[:m_od, 0], w[:m_od, 1] = wr, wt
    for part, lo, hi in ((odometry, 0, m_od), (loops, m_od, m)):
        if part is not None:                                   # copy_ converts and allocates nothing for device sources
            edges[lo:hi].copy_(torch.as_tensor(part["edge_index"]))
            Z[lo:hi].copy_(torch.as_tensor(part["Z"]))
            w[lo:hi].copy_(torch.as_tensor(part["weights"]))
    res = optimize_pose_graph(X, edges, Z, w, out=out, **kw)
    res.update(edge_index=edges, Z=Z, weights=w, n_odometry=m_od, _traj_in=store)
    if consistency is not None:
        res["consistency"] = filtered
    return res
