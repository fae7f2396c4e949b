"""Time the pose-graph optimiser on the device: device events around whole calls of optimize_pose_graph,
warm-up, median of --reps, eager and as a replayed graph (egonn_graph_begin / _end with out=), and the cost trace against the
PCG budget.

Workload: a synthetic trajectory of --poses scans at 10 Hz, 10 m/s on a circle of 200 m radius (about 16 laps for 20 000
poses), odometry edges with noise (0.002 rad, 0.01 m per step) integrated into the start (dead reckoning), and --loops loop
edges to the pose one lap earlier with noise (0.005 rad, 0.03 m).  There is no parent to compare against: the time is
reported, not gated.

    python tools/time_pose_graph.py --out profiles/pose_graph_timing.json [--commit HASH]
"""
import argparse
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def _exp_rows(w):
    th = np.linalg.norm(w, axis=1)
    t = np.where(th < 1e-8, 1.0, th)
    ca, cb = np.where(th < 1e-8, 1.0, np.sin(t) / t), np.where(th < 1e-8, 0.5, 2.0 * np.sin(0.5 * t) ** 2 / t ** 2)
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    return np.eye(3) + ca[:, None, None] * K + cb[:, None, None] * (K @ K)


def _noise(rng, m, rot, trans):
    T = np.tile(np.eye(4), (m, 1, 1))
    T[:, :3, :3] = _exp_rows(rng.normal(0.0, rot, (m, 3)))
    T[:, :3, 3] = rng.normal(0.0, trans, (m, 3))
    return T


def _rel(Xa, Xb):
    T = np.tile(np.eye(4), (len(Xa), 1, 1))
    Rt = Xa[:, :3, :3].transpose(0, 2, 1)
    T[:, :3, :3] = Rt @ Xb[:, :3, :3]
    T[:, :3, 3] = np.einsum("eij,ej->ei", Rt, Xb[:, :3, 3] - Xa[:, :3, 3])
    return T


def synthetic(n, n_loops, seed=0):
    rng = np.random.default_rng(seed)
    radius, speed, rate = 200.0, 10.0, 10.0
    a = speed / rate / radius * np.arange(n)
    T = np.tile(np.eye(4), (n, 1, 1))
    yaw = np.zeros((n, 3))
    yaw[:, 2] = a + math.pi / 2
    T[:, :3, :3] = _exp_rows(yaw)
    T[:, 0, 3], T[:, 1, 3] = radius * np.cos(a), radius * np.sin(a)
    odo = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).astype(np.int32)
    Zo = _rel(T[:-1], T[1:]) @ _noise(rng, n - 1, 0.002, 0.01)
    X0 = T.copy()
    for i in range(n - 1):
        X0[i + 1] = X0[i] @ Zo[i]
    lap = int(round(2 * math.pi * radius / (speed / rate)))
    b = np.sort(rng.choice(np.arange(lap, n), size=min(n_loops, n - lap), replace=False))
    loops = np.stack([b - lap, b], axis=1).astype(np.int32)
    Zl = _rel(T[loops[:, 0]], T[loops[:, 1]]) @ _noise(rng, len(loops), 0.005, 0.03)
    w = np.concatenate([np.tile([1 / 0.002 ** 2, 1 / 0.01 ** 2], (n - 1, 1)), np.tile([1 / 0.005 ** 2, 1 / 0.03 ** 2], (len(loops), 1))])
    return T, X0, np.concatenate([odo, loops]), np.concatenate([Zo, Zl]), w, lap


def _timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "calls": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--poses", type=int, default=20000)
    ap.add_argument("--loops", type=int, default=2000)
    ap.add_argument("--max_iterations", type=int, default=4)
    ap.add_argument("--budgets", type=int, nargs="+", default=[100, 500, 2000])
    ap.add_argument("--graph_max_budget", type=int, default=2000, help="capture and replay only up to this PCG budget")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd as ea
    from egonn_amd import _lib
    lib = _lib.load()
    T, X0, edges, Z, w, lap = synthetic(args.poses, args.loops)
    n = len(T)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (X0, edges, Z, w)]
    terr = lambda P: float(np.linalg.norm(P[:, :3, 3] - T[:, :3, 3], axis=1).mean())          # noqa: E731
    rows = []
    for budget in args.budgets:
        kw = dict(max_iterations=args.max_iterations, pcg_iterations=budget)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            out = ea.optimize_pose_graph(*dev, **kw)
            st.synchronize()
            row = {"pcg_iterations": budget, "max_iterations": args.max_iterations,
                   "launches_per_call": args.max_iterations * (2 * budget + 5) + 12,
                   "cost_trace": out["cost_trace"].cpu().tolist(), "accept_trace": out["accept_trace"].cpu().tolist(),
                   "mean_translation_error_m": {"start": terr(X0), "end": terr(out["poses"].cpu().numpy())},
                   "status": int(out["status"].item()),
                   "scratch_bytes": int(lib.egonn_pose_graph_scratch_bytes(n, len(edges), budget))}
            row["eager_ms"] = _timed(lambda: ea.optimize_pose_graph(*dev, out=out, **kw), 1, args.reps)
            if budget <= args.graph_max_budget:
                gr = ctypes.c_void_p()
                _lib.check(lib.egonn_graph_begin(st.cuda_stream))
                try:
                    ea.optimize_pose_graph(*dev, out=out, **kw)
                finally:
                    rc = lib.egonn_graph_end(st.cuda_stream, ctypes.byref(gr))
                _lib.check(rc)
                row["graph_replay_ms"] = _timed(lambda: _lib.check(lib.egonn_graph_launch(gr, st.cuda_stream)), 1, args.reps)
                lib.egonn_graph_destroy(gr)
        torch.cuda.current_stream().wait_stream(st)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "commit": args.commit,
           "workload": f"{n} poses at 10 Hz on a 200 m circle ({lap} poses per lap), {n - 1} odometry edges (noise 0.002 rad, 0.01 m, "
                       f"integrated into the start), {len(edges) - n + 1} loop edges one lap back (noise 0.005 rad, 0.03 m), weights 1/sigma^2",
           "timer": "device events around one whole optimize_pose_graph call (plan + every launch), one warm-up call, median, min and max "
                    "of the calls; graph_replay_ms: the same call captured once with out= and replayed",
           "runs": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
