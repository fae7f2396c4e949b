"""Time the ICP refinement on the device: P = 1 and P = 16 pairs of 50 k-point planted scan pairs (downsample + ICP from the
perturbed init, 200 rounds allowed).  Per P: ms per pair from device events around whole calls, rounds run, the wall time
of the float64 restatement (tests/test_icp_host.py) on the same pairs for scale, and, with --kernel-split, the split of the
device time between the search kernel and the rest from a `rocprofv3 --kernel-trace --stats` run of this script in a child
process.  And voxel_downsample on its own: the 2 P raw clouds of each P as one batch, voxel 0.1.  Records, not gates.  Writes one
JSON file.

    python tools/time_icp.py --out profiles/icp_timing.json [--commit HASH] [--kernel-split]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

DISTINCT = 4


def _pairs(n_points):
    from egonn_amd.synth import planted_scan_pair
    return [planted_scan_pair(100 + i, n_points) for i in range(DISTINCT)]


def _device_rows(args, pairs):
    import egonn_amd
    rows = []
    for P in args.pairs:
        sel = [pairs[i % DISTINCT] for i in range(P)]
        T0 = torch.from_numpy(np.stack([p[3] for p in sel])).cuda()
        srcs, tgts = [torch.from_numpy(p[0]).cuda() for p in sel], [torch.from_numpy(p[1]).cuda() for p in sel]

        def call():
            return egonn_amd.refine_pairs(srcs, tgts, T0, None, 1.2, args.max_iteration)
        for _ in range(2):
            r = call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        a, b = r["_clouds"][:2]                     # (source, target, normals or None) since the point-to-plane estimator
        rows.append({"pairs": P, "raw_points_per_cloud": int(len(sel[0][0])), "max_iteration": args.max_iteration,
                     "downsampled_source_points": int(a["offsets"][-1]) // P, "downsampled_target_points": int(b["offsets"][-1]) // P,
                     "ms_per_call": {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "calls": len(ms)},
                     "ms_per_pair": float(np.median(ms)) / P, "rounds_run": r["iterations"].cpu().tolist(),
                     "status": r["status"].cpu().tolist(), "fitness": r["fitness"].cpu().tolist()})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def _downsample_rows(args, pairs):
    """voxel_downsample alone: the raw clouds of P pairs as one batch of 2 P clouds"""
    import egonn_amd
    rows = []
    for P in args.pairs:
        clouds = [c.astype(np.float32) for i in range(P) for c in pairs[i % DISTINCT][:2]]
        off = np.zeros(len(clouds) + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in clouds])
        pts, off = torch.from_numpy(np.concatenate(clouds)).cuda(), torch.from_numpy(off).cuda()
        for _ in range(3):
            r = egonn_amd.voxel_downsample(pts, off, 0.1)
        torch.cuda.synchronize()
        ms = []
        for _ in range(4 * args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = egonn_amd.voxel_downsample(pts, off, 0.1)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        rows.append({"clouds": len(clouds), "raw_points": int(len(pts)), "voxels": int(r["offsets"][-1]),
                     "ms_per_call": {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "calls": len(ms)}})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def _kernel_split(args):
    """this script again under rocprofv3 (a fresh child process; the program goes after `--`), P = the largest batch"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "icp", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--pairs", str(max(args.pairs)), "--reps", "2", "--n_points", str(args.n_points),
               "--max_iteration", str(args.max_iteration), "--out", os.path.join(d, "child.json")]
        pr = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if pr.returncode != 0 or not files:
            return {"error": "rocprofv3 run failed or wrote no kernel_stats.csv", "returncode": pr.returncode, "tail": pr.stdout[-600:]}
        search = rest = 0.0
        top = []
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0.0)
            if "icp_" in name or "ds_" in name or "sort_seg" in name:
                if "icp_search_kernel" in name:
                    search += ns
                else:
                    rest += ns
                top.append((ns, name.split("(")[0], int(float(row.get("Calls") or 0))))
        top.sort(reverse=True)
        return {"pairs": max(args.pairs), "search_ms": search * 1e-6, "rest_ms": rest * 1e-6,
                "search_share": search / (search + rest) if search + rest > 0 else None,
                "kernels": [{"kernel": n, "total_ms": t * 1e-6, "calls": c} for t, n, c in top[:12]],
                "note": "whole child run: 2 warm-up + 2 timed calls of downsample + ICP"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--n_points", type=int, default=50000)
    ap.add_argument("--max_iteration", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-split", action="store_true")
    ap.add_argument("--child", action="store_true", help="device calls only (the process rocprofv3 traces)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    pairs = _pairs(args.n_points)
    rows = _device_rows(args, pairs)
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit,
           "workload": f"planted_scan_pair(100 + i, {args.n_points}), {DISTINCT} distinct pairs tiled up to P; voxel 0.1, max_dist 1.2",
           "timer": "device events around one whole call (two downsamples + ICP, fixed launch sequence of max_iteration rounds); "
                    "median over the calls after 2 warm-up calls", "rows": rows,
           "voxel_downsample": _downsample_rows(args, pairs)}
    if not args.child:
        from tests.test_icp_host import downsample_f64, icp_f64
        t0 = time.perf_counter()
        ref = [icp_f64(downsample_f64(p[0])[0], downsample_f64(p[1])[0], p[3], 1.2, args.max_iteration) for p in pairs]
        wall = time.perf_counter() - t0
        out["float64_restatement"] = {"s_per_pair": wall / DISTINCT, "pairs": DISTINCT, "rounds_run": [r["iterations"] for r in ref],
                                      "search": "scipy cKDTree" if "scipy" in sys.modules else "brute force",
                                      "note": "host wall time of downsample_f64 + icp_f64, for scale"}
        if args.kernel_split:
            out["kernel_split"] = _kernel_split(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
