"""Time the device augmentation on the training batch shape: 32 scans of about 50 k points, both modes.  Device time per call
from windows of back-to-back calls between device events (median window after warm-up, divided by the calls in it), the
achieved bytes/s against the 24 B/point floor (12 B read + 12 B written), the voxelisation of the same batch by the same
protocol, their share of the 10.8 ms training step, the wall time of the NumPy restatement
(tests/augment_ref.py, fp32) of the same batch on the host (on one thread, and scan by scan on a pool of up to 16), and, with --kernel-split, the per-kernel device time from a
`rocprofv3 --kernel-trace --stats` run of this script in a child process.  Records, not gates.  Writes one JSON file.

    python tools/time_augment.py --out profiles/augment_timing.json [--commit HASH] [--kernel-split]
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
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

STEP_MS = 10.8


def _batch(scans, n_points):
    from tests import augment_ref as R
    rng = np.random.default_rng(32)
    sizes = rng.integers(int(0.96 * n_points), int(1.04 * n_points), scans).tolist()
    return R.batch(32, sizes)


def _windows(fn, calls, windows, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "windows": windows,
            "calls_per_window": calls}


def _device_rows(args, pts, off):
    import egonn_amd
    from egonn_amd import augment as A
    dev = torch.device("cuda", 0)
    d_pts = torch.from_numpy(pts).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    ids = torch.arange(len(off) - 1, dtype=torch.int32, device=dev)
    out = torch.empty_like(d_pts)
    scratch = torch.empty(A.scratch_bytes(len(pts), len(off) - 1) + 256, dtype=torch.uint8, device=dev)
    rows = []
    for mode in (1, 2):
        b = egonn_amd.TrainBatcher(egonn_amd.CartesianQuantizer(0.1), aug_mode=mode, seed=1)
        p = b.params()

        def call():
            A.augment_points(d_pts, d_off, ids, p, draw=1, set_id=1, out=out, scratch=scratch)
        t = _windows(call, args.calls, args.windows, args.warmup)
        rows.append({"mode": mode, "scans": len(off) - 1, "points": int(len(pts)), "ms_per_call": t,
                     "bytes_floor": 24 * int(len(pts)), "achieved_GBps_of_floor_bytes": 24e-6 * len(pts) / t["median"]})
        print(json.dumps(rows[-1]), flush=True)
    if args.child:
        return rows, None
    ctx = b.ctx

    def vox():
        ctx.voxelize(out, off.tolist(), b.quantizer.mode, b.quantizer.step)
    v = _windows(vox, max(args.calls // 4, 1), args.windows, 2)
    return rows, v


def _kernel_split(args):
    """this script again under rocprofv3 (a fresh child process; the program goes after `--`)"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "aug", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--calls", "10", "--windows", "2", "--warmup", "2", "--out",
               os.path.join(d, "child.json")]
        pr = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if pr.returncode != 0 or not files:
            return {"error": "rocprofv3 run failed or wrote no kernel_stats.csv", "returncode": pr.returncode, "tail": pr.stdout[-600:]}
        rows = []
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name") or row.get("KernelName") or ""
            if "aug_" in name:
                ns, calls = float(row.get("TotalDurationNs") or 0.0), int(float(row.get("Calls") or 0))
                rows.append({"kernel": name.split("(")[0], "calls": calls, "total_ms": ns * 1e-6, "us_per_launch": ns * 1e-3 / max(calls, 1)})
        return {"kernels": sorted(rows, key=lambda r: -r["total_ms"]), "note": "both modes together: mode 1 and mode 2 calls alternate "
                "in halves of the child run; us_per_launch is the mean over all launches of that kernel"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--scans", type=int, default=32)
    ap.add_argument("--n_points", type=int, default=50000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--kernel-split", action="store_true")
    ap.add_argument("--child", action="store_true", help="device calls only (the process rocprofv3 traces)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    pts, off = _batch(args.scans, args.n_points)
    rows, vox = _device_rows(args, pts, off)
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit,
           "workload": f"{args.scans} scans of about {args.n_points} points (tests/augment_ref.batch(32, sizes)), TrainTransform + "
                       "TrainSetTransform of the mode in one call",
           "timer": "device events around windows of back-to-back calls; median window after warm-up, per call", "rows": rows}
    if not args.child:
        from tests import augment_ref as R
        out["voxelize_ms_per_call"] = vox
        for r in rows:
            r["share_of_step"] = {"step_ms": STEP_MS, "augment": r["ms_per_call"]["median"] / STEP_MS,
                                  "augment_plus_voxelize": (r["ms_per_call"]["median"] + vox["median"]) / STEP_MS}
        threads = min(16, len(os.sched_getaffinity(0)))
        host = {}
        for mode in (1, 2):
            P = R.Params(seed=1, draw=1, set_id=1, stages=(R.MODE1 | R.SET1) if mode == 1 else (R.MODE2 | R.SET2))

            def one(b):      # a scan's augmentation does not depend on its batch, so the scans can run side by side
                return R.augment(pts[off[b]:off[b + 1]], [0, off[b + 1] - off[b]], [b], P, np.float32)["out"]
            t0 = time.perf_counter()
            R.augment(pts, off, list(range(len(off) - 1)), P, np.float32)
            host[f"mode{mode}_1_thread_s"] = time.perf_counter() - t0
            with ThreadPoolExecutor(threads) as pool:
                t0 = time.perf_counter()
                list(pool.map(one, range(len(off) - 1)))
                host[f"mode{mode}_{threads}_threads_s"] = time.perf_counter() - t0
        out["host_restatement"] = {**host, "threads": threads,
                                   "note": "wall time of tests/augment_ref.augment(float32), NumPy: the whole batch on one thread, "
                                           "and one scan per task on a pool of `threads` threads"}
        if args.kernel_split:
            out["kernel_split"] = _kernel_split(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
