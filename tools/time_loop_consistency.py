"""Time the loop-consistency filter on the device by the method of tools/time_pose_graph.py: device events
around whole calls, one warm-up, the median of --reps; filter_loops eager and as a replayed graph (egonn_graph_begin / _end
with out=), and beside it one optimize_trajectory at a PCG budget of 500 with the filter and without.

Workload: the trajectory of tools/time_pose_graph.py (--poses scans at 10 Hz, 10 m/s on a circle of 200 m radius, dead-reckoned
odometry noise), one loop row per scan as loop_edges makes them (a = -1, weight 0 where no loop was found), --loops of them
live loops to the pose one lap earlier (noise 0.005 rad, 0.03 m) and --false planted false loops on other rows (a random
earlier node, a random Z of up to 1 rad and 5 m).  There is no parent to compare against: the time is reported, not gated.

    python tools/time_loop_consistency.py --out profiles/loop_consistency_timing.json [--commit HASH]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from time_pose_graph import _exp_rows, _timed, synthetic


def loop_rows(n, n_loops, n_false, seed=0):
    """-> truth, drifting poses, per-scan loop rows (edge_index (n,2), Z, weights), masks of the true and the false rows, lap"""
    T, X0, edges, Z, w, lap = synthetic(n, n_loops, seed)
    live, Zl, wl = edges[n - 1:], Z[n - 1:], w[n - 1:]
    ei = np.stack([np.full(n, -1), np.arange(n)], axis=1).astype(np.int32)
    Zr, wr = np.tile(np.eye(4), (n, 1, 1)), np.zeros((n, 2))
    ei[live[:, 1], 0], Zr[live[:, 1]], wr[live[:, 1]] = live[:, 0], Zl, wl
    is_true = wr[:, 0] > 0
    rng = np.random.default_rng(seed + 1)
    rows = rng.choice(np.flatnonzero(~is_true & (np.arange(n) >= 200)), size=n_false, replace=False)
    ax = rng.standard_normal((n_false, 3))
    Zf = np.tile(np.eye(4), (n_false, 1, 1))
    Zf[:, :3, :3] = _exp_rows(ax / np.linalg.norm(ax, axis=1, keepdims=True) * rng.uniform(0, 1.0, (n_false, 1)))
    Zf[:, :3, 3] = rng.uniform(-5.0, 5.0, (n_false, 3))
    ei[rows, 0], Zr[rows], wr[rows] = (rng.uniform(0, 1, n_false) * (rows - 100)).astype(np.int32), Zf, wl[0]
    is_false = np.zeros(n, bool)
    is_false[rows] = True
    return T, X0, ei, Zr, wr, is_true, is_false, lap


def _replayed(lib, _lib, st, fn, reps):
    gr = ctypes.c_void_p()
    _lib.check(lib.egonn_graph_begin(st.cuda_stream))
    try:
        fn()
    finally:
        rc = lib.egonn_graph_end(st.cuda_stream, ctypes.byref(gr))
    _lib.check(rc)
    ms = _timed(lambda: _lib.check(lib.egonn_graph_launch(gr, st.cuda_stream)), 1, reps)
    lib.egonn_graph_destroy(gr)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--poses", type=int, default=20000)
    ap.add_argument("--loops", type=int, default=2000)
    ap.add_argument("--false", type=int, default=100, dest="n_false")
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--max_partners", type=int, default=256)
    ap.add_argument("--max_rounds", type=int, default=16)
    ap.add_argument("--max_iterations", type=int, default=4)
    ap.add_argument("--pcg_iterations", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd as ea
    from egonn_amd import _lib
    lib = _lib.load()
    T, X0, ei, Z, w, is_true, is_false, lap = loop_rows(args.poses, args.loops, args.n_false)
    n = len(T)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()                           # noqa: E731
    poses, loops = cu(X0), {"edge_index": cu(ei), "Z": cu(Z), "weights": cu(w)}
    terr = lambda P: float(np.linalg.norm(P[:, :3, 3] - T[:, :3, 3], axis=1).mean())          # noqa: E731
    fkw = dict(window=args.window, max_partners=args.max_partners, max_rounds=args.max_rounds)
    okw = dict(max_iterations=args.max_iterations, pcg_iterations=args.pcg_iterations,
               odometry_weight=(1 / 0.002 ** 2, 1 / 0.01 ** 2))
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        out = ea.filter_loops(poses, loops, **fkw)
        st.synchronize()
        keep = out["keep"].cpu().numpy()
        filt = {"parameters": dict(fkw, trans_thr=1.0, rot_thr=0.1, trans_drift=0.0, rot_drift=0.0, min_support=2),
                "launches_per_call": args.max_rounds + 3, "sort_launches_not_counted": True,
                "scratch_bytes": int(lib.egonn_loop_consistency_scratch_bytes(n, args.max_partners)),
                "true_loops": int(is_true.sum()), "true_kept": int(keep[is_true].sum()),
                "false_loops": int(is_false.sum()), "false_kept": int(keep[is_false].sum()),
                "rounds": int(out["rounds"].item()), "status": int(out["status"].item()),
                "support0_of_true_loops": {"min": int(out["support0"].cpu().numpy()[is_true].min()),
                                           "median": float(np.median(out["support0"].cpu().numpy()[is_true]))}}
        filt["eager_ms"] = _timed(lambda: ea.filter_loops(poses, loops, out=out, **fkw), 1, args.reps)
        filt["graph_replay_ms"] = _replayed(lib, _lib, st, lambda: ea.filter_loops(poses, loops, out=out, **fkw), args.reps)
        print(json.dumps(filt), flush=True)
        runs = []
        for name, extra in (("with_filter", dict(consistency=fkw)), ("without_filter", {})):
            res = ea.optimize_trajectory(poses, loops, **extra, **okw)
            st.synchronize()
            row = {"run": name, "pcg_iterations": args.pcg_iterations, "max_iterations": args.max_iterations,
                   "cost_trace": res["cost_trace"].cpu().tolist(), "accept_trace": res["accept_trace"].cpu().tolist(),
                   "mean_translation_error_m": {"start": terr(X0), "end": terr(res["poses"].cpu().numpy())}}
            row["eager_ms"] = _timed(lambda: ea.optimize_trajectory(poses, loops, out=res, **extra, **okw), 1, args.reps)
            runs.append(row)
            print(json.dumps(row), flush=True)
    torch.cuda.current_stream().wait_stream(st)
    res = {"device": torch.cuda.get_device_name(0), "commit": args.commit,
           "workload": f"{n} poses at 10 Hz on a 200 m circle ({lap} poses per lap, odometry noise 0.002 rad, 0.01 m integrated into the "
                       f"start), E = {n} loop rows, one per scan: {int(is_true.sum())} live loops one lap back (noise 0.005 rad, 0.03 m), "
                       f"{int(is_false.sum())} planted false loops (random earlier node, Z up to 1 rad and 5 m), the rest a = -1 with "
                       f"weight 0",
           "timer": "device events around one whole call, one warm-up call, median, min and max of the calls; graph_replay_ms: the "
                    "same filter_loops call captured once with out= and replayed; optimize_trajectory: eager calls with out=, with "
                    "the filter (consistency=) and without",
           "filter_loops": filt, "optimize_trajectory": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
