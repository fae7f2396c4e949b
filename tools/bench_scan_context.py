"""Time the ScanContext kernels on the device.  Records, not gates.  Writes one JSON file.

  descriptor  egonn_scan_context (memset + cells kernel + ring-key kernel, 20 x 60) on B = 16 scans of 50 k points and on
              B = 1 scan of 120 k points (synth.lidar_scan): scans/s and the share of the 8 TB/s HBM roof, counting the bytes
              the algorithm needs: 12 B per point plus the descriptors and ring keys written once.  Timed as a replayed
              graph of the call (no host work between launches; the rates are computed from this) and as eager calls; a
              third row, B = 256 x 50 k, shows the rate once the device rather than the launch sequence sets the time.
  distance    egonn_scan_context_distance at Q = 1024 queries, k = 50 listed candidates out of 4096 map descriptors, 20 x 60:
              pairs/s, and the rerank of the same lists.
Timer: device events around `--inner` back-to-back calls (one call is far below the resolution that a pair of events
resolves well), after `--warmup` calls; the median over `--reps` such windows.  A call's time is its whole launch sequence,
not one kernel's begin-to-end.

    python tools/bench_scan_context.py --out profiles/scan_context_timing.json [--commit HASH]
"""
import argparse
import datetime
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

HBM_ROOF = 8.0e12          # B/s


def _time(call, warmup, reps, inner):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "windows": len(ms),
            "calls_per_window": inner}


def _time_graph(call, warmup, reps, inner):
    """the same call captured once and replayed: no host work between the launches"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = call()
    t = _time(graph.replay, warmup, reps, inner)
    del keep
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    from egonn_amd import scan_context as sc
    from egonn_amd.synth import lidar_scan

    R, S = 20, 60
    s = sc.ScanContext(S, R)
    rows = []
    for B, n_points in ((16, 50_000), (1, 120_000), (256, 50_000)):
        clouds = [lidar_scan(200 + i, n_points=n_points) for i in range(min(B, 4))]
        pts = torch.from_numpy(np.concatenate([clouds[i % len(clouds)] for i in range(B)])).cuda()
        off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * n_points
        eager = _time(lambda: s.batch(pts, off), args.warmup, args.reps, args.inner)
        t = _time_graph(lambda: s.batch(pts, off), args.warmup, args.reps, args.inner)
        nbytes = 12 * B * n_points + 4 * B * R * S + 4 * B * R
        sec = t["median_ms"] * 1e-3
        rows.append({"what": "descriptor", "batch": B, "points_per_scan": n_points, "shape": [R, S], "ms_per_call_eager": eager,
                     "ms_per_call": t,
                     "scans_per_s": B / sec, "algorithmic_bytes": nbytes, "bytes_per_s": nbytes / sec,
                     "share_of_hbm_roof": nbytes / sec / HBM_ROOF})
        print(json.dumps(rows[-1]), flush=True)

    Q, M, k = 1024, 4096, 50
    rng = np.random.default_rng(0)
    base = s.batch(torch.from_numpy(np.concatenate([lidar_scan(300 + i, n_points=20_000) for i in range(8)])).cuda(),
                   torch.arange(9, dtype=torch.int64, device="cuda") * 20_000)[0]
    # M distinct descriptors: the 8 real ones rolled by every multiple of a sector, scaled a little
    msc = torch.stack([torch.roll(base[i % 8], shifts=i // 8, dims=1) * (1.0 + 1e-3 * (i % 7)) for i in range(M)]).contiguous()
    qsc = msc[torch.from_numpy(rng.integers(0, M, Q)).cuda()].contiguous()
    cand = torch.from_numpy(rng.integers(0, M, (Q, k)).astype(np.int32)).cuda()
    t = _time(lambda: sc.distance_pairs(qsc, msc, cand), args.warmup, args.reps, max(1, args.inner // 5))
    sec = t["median_ms"] * 1e-3
    flops = 2.0 * Q * k * (R + 1) * S * S
    rows.append({"what": "distance", "queries": Q, "k": k, "map": M, "shape": [R, S], "ms_per_call": t, "pairs_per_s": Q * k / sec,
                 "flops": flops, "flops_per_s": flops / sec, "algorithmic_bytes": 4 * R * S * (Q * k + Q) + 12 * Q * k})
    print(json.dumps(rows[-1]), flush=True)
    dist, yaw = sc.distance_pairs(qsc, msc, cand)
    t = _time(lambda: sc.rerank(dist, yaw, cand), args.warmup, args.reps, args.inner)
    rows.append({"what": "rerank", "queries": Q, "k": k, "ms_per_call": t, "queries_per_s": Q / (t["median_ms"] * 1e-3)})
    print(json.dumps(rows[-1]), flush=True)

    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "date": datetime.date.today().isoformat(),
           "timer": "device events around back-to-back calls after warm-up calls; median over the windows; a call is its whole "
                    "launch sequence (descriptor: memset + cells kernel + ring-key kernel), allocation of its outputs included",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
