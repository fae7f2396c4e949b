"""Time the point-to-plane ICP on the device next to the point-to-point one.  Records, not gates.  Writes one JSON file:

  estimate_normals   `estimate_normals` (knn = 20) of each case's downsampled target: device events around windows of repeated
                     calls, median over the windows
  cases              per case of tests/test_icp_host.py:ICP_CASES and per estimator: the rounds the loop ran, and the device time
                     of one `icp_pairs` call (max_iteration = the rounds that case needs + 2, so the fixed launch sequence is not
                     padded by 200 empty rounds), again device events, median of windows.  The plane row also carries the time
                     with the normals included.

    python tools/time_icp_plane.py --out profiles/icp_plane_timing.json [--commit HASH]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch


def _median(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "windows": len(v)}


def _windows(fn, windows, calls):
    """ms per call of fn(): device events around `calls` back-to-back calls, one value per window, after two warm-up calls"""
    for _ in range(2):
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
    return _median(ms)


def time_case(name, windows, calls, knn):
    from egonn_amd import estimate_normals, icp_pairs
    from tests.test_icp_host import icp_case
    c = icp_case(name)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                      # noqa: E731
    s, t, T0 = cu(c["src"]), cu(c["tgt"]), cu(c["T_init"][None])
    so = torch.tensor([0, len(c["src"])], dtype=torch.int64, device="cuda")
    to = torch.tensor([0, len(c["tgt"])], dtype=torch.int64, device="cuda")
    nrm = estimate_normals(t, to, knn)["normals"]
    row = {"source_points": len(c["src"]), "target_points": len(c["tgt"]),
           "estimate_normals_ms": _windows(lambda: estimate_normals(t, to, knn), windows, calls)}
    for est, tn in (("point_to_point", None), ("point_to_plane", nrm)):
        full = icp_pairs(s, so, t, to, T0, 1.2, 200, tgt_normals=tn)
        rounds, status = int(full["iterations"][0]), int(full["status"][0])
        limit = rounds + 2
        cut = icp_pairs(s, so, t, to, T0, 1.2, limit, tgt_normals=tn)
        assert torch.equal(cut["T"], full["T"]) and int(cut["iterations"][0]) == rounds, "the round limit must not change the result"
        row[est] = {"rounds": rounds, "status": status, "fitness": float(full["fitness"][0]), "inlier_rmse": float(full["inlier_rmse"][0]),
                    "max_iteration_timed": limit,
                    "ms_per_pair": _windows(lambda: icp_pairs(s, so, t, to, T0, 1.2, limit, tgt_normals=tn), windows, calls)}
    p = row["point_to_plane"]
    p["ms_per_pair_with_normals"] = p["ms_per_pair"]["median"] + row["estimate_normals_ms"]["median"]
    row["plane_over_point_time"] = p["ms_per_pair_with_normals"] / row["point_to_point"]["ms_per_pair"]["median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--knn", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    from tests.test_icp_host import ICP_CASES
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "knn": args.knn, "calls_per_window": args.calls,
           "timer": "device events around a window of whole calls (one pair per call, allocation of the outputs and scratch "
                    "included), median over the windows after two warm-up calls", "cases": {}}
    for name in ICP_CASES:
        out["cases"][name] = time_case(name, args.windows, args.calls, args.knn)
        print(name, json.dumps(out["cases"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
