"""Time the loop-closure path on the device (method of tools/time_relocalize.py: device events around windows of back-to-back
calls, median of the windows after warm-up; two forms that are compared are ALTERNATED window by window in the same run, so
both see the same machine).

  1. detect_loops over a synthetic trajectory (--entries scans at 10 Hz, --dim descriptor, k = --k, min_time_gap 30 s) next to
     the parent route that does at least that arithmetic: retrieval.knn of all queries on the FULL database at chunk 4096 (every
     query against every scan, where the windowed search reads on average half of them), and the scratch bytes of both.
     The two are also compared where they must agree: the last query, searched by the parent on its admissible prefix.
  2. LoopDetector.push of a 16-scan batch (verify on and off) onto maps of --map_sizes entries.

    python tools/time_loop_closure.py --out profiles/loop_closure_timing.json [--commit HASH]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def _window(fn, burst):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(burst):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / burst


def _time_alternated(forms, warmup, reps, burst):
    """forms: {name: fn}.  -> {name: {median, min, max} in milliseconds per call}; window i of every form before window i + 1"""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(_window(fn, burst))
    return {name: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "windows": reps,
                   "calls_per_window": burst} for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--entries", type=int, default=20000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--min_time_gap", type=float, default=30.0)
    ap.add_argument("--map_sizes", type=int, nargs="+", default=[1000, 5000, 20000])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--n_k", type=int, default=128)
    ap.add_argument("--hypotheses", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd as ea
    from egonn_amd import _lib, retrieval
    from egonn_amd.synth import planted_keypoint_pair as planted_pair
    lib = _lib.load()
    n, d, k = args.entries, args.dim, args.k
    rng = np.random.default_rng(0)
    glob = rng.standard_normal((n + args.batch, d)).astype(np.float32)      # the trajectory and one more batch
    glob /= np.linalg.norm(glob, axis=1, keepdims=True)
    glob_d = torch.from_numpy(glob).cuda()
    times = 1.7e9 + 0.1 * np.arange(n + args.batch)
    glob_n, times_d = glob_d[:n], torch.from_numpy(times[:n]).cuda()
    keep = {}

    def windowed():
        keep["w"] = ea.detect_loops(glob_n, times_d, k, args.min_time_gap)

    def parent_full():
        keep["p"] = retrieval.knn(glob_n, glob_n, k, chunk=4096)

    t = _time_alternated({"detect_loops": windowed, "parent_knn_full_database_chunk_4096": parent_full}, 1, args.reps, 1)
    hi = keep["w"]["win_hi"]
    # where both must agree: the last query's window reaches over all but the last 30 s; search it on that prefix with the parent
    last = int(hi[-1])
    pi, pd = retrieval.knn(glob_n[-1:], glob_n[:last], k)
    agree = bool(torch.equal(pi, keep["w"]["nn_index"][-1:]) and torch.equal(pd.view(torch.int32), keep["w"]["nn_dist"][-1:].view(torch.int32)))
    offline = {"entries": n, "dim": d, "k": k, "min_time_gap_s": args.min_time_gap, "ms": t,
               "rows_read_windowed": int(hi.long().sum()), "rows_read_parent": n * n,
               "scratch_bytes_windowed": int(lib.egonn_knn_window_scratch_bytes(n, k)),
               "scratch_bytes_parent": min(n, 4096) * n * 4,
               "last_query_equals_parent_on_its_prefix": agree}
    print(json.dumps(offline), flush=True)

    nk, D, H, B = args.n_k, 128, args.hypotheses, args.batch
    distinct = 64
    pairs = [planted_pair(nk, 5000 + i, 0.3 + 0.05 * (i % 7)) for i in range(distinct)]
    tile = lambda i, m: torch.from_numpy(np.stack([pairs[j % distinct][i] for j in range(m)]))      # noqa: E731
    pushes = []
    for M in args.map_sizes:
        M = min(M, n)
        km = ea.KeypointMap(n_k=nk, dim=D, global_dim=d)
        for lo in range(0, M, 2048):                              # the resident map: M entries of n_k keypoints and descriptors
            m = min(M, lo + 2048) - lo
            km.add({"global": glob_d[lo:lo + m], "keypoints": tile(3, m), "descriptors": tile(1, m)}, np.tile(np.eye(4), (m, 1, 1)))
        batch = {"global": glob_d[M:M + B], "keypoints": tile(2, B).cuda(), "descriptors": tile(0, B).cuda()}
        row = {"map_entries": M, "batch": B, "k": k, "n_k": nk, "dim": D, "global_dim": d, "hypotheses": H,
               "scratch_bytes_knn_window": int(lib.egonn_knn_window_scratch_bytes(B, k))}
        forms = {}
        for verify in (False, True):
            # both detectors adopt the one map; every timed push lands on exactly M entries: the map is rewound after each call
            det = ea.LoopDetector(kmap=km, k=k, min_time_gap=args.min_time_gap, verify=verify, ransac_max_it=H, times=times[:M])

            def push(det=det, M=M):
                det.push(batch, times[M:M + B])
                det.kmap._n, det._last = M, float(times[M - 1])
            forms["push_verify" if verify else "push_search_only"] = push
        row["ms"] = _time_alternated(forms, 2, args.reps, 4)
        pushes.append(row)
        print(json.dumps(row), flush=True)

    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit,
           "workload": "unit-norm random global descriptors, stamps 0.1 s apart at Unix scale; push: planted keypoint pairs tiled "
                       "into the map (the candidates of the timed batch are unrelated places: every pair runs its full RANSAC)",
           "timer": "device events around a window of back-to-back calls, per-call time = window / calls; median, min and max over "
                    "the windows after warm-up; compared forms alternated window by window in one run",
           "offline": offline, "push": pushes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
