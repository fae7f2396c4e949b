"""Time the three registration kernels on the device: seeded planted pairs, P = 1, 64, 4096 at n_k = 128 and 256,
H = 10000.  Per kernel: warm-up, then timed windows of back-to-back launches between device events (>= ~5 ms of work per
window for the small batches), time per launch = window / launches.  Writes one JSON file.

    python tools/time_registration.py --out profiles/registration_timing.json [--commit HASH] [--pairs 1 64 4096]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def _time(fn, warmup, reps, burst):
    """ms per launch: `reps` timed windows of `burst` back-to-back launches between one pair of device events, so that a window
    holds milliseconds of work and the bracket's own cost (a few microseconds) is spread over the burst"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(burst):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / burst)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 64, 4096])
    ap.add_argument("--n_k", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--hypotheses", type=int, default=10000)
    ap.add_argument("--distinct", type=int, default=64, help="distinct seeded pairs, tiled up to P")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    from egonn_amd.synth import pad_keypoint_pairs as pad_batch, planted_keypoint_pair as planted_pair
    lib = _lib.load()
    H = args.hypotheses
    rows = []
    for nk in args.n_k:
        base = pad_batch([planted_pair(nk, 5000 + i, 0.3 + 0.05 * (i % 7)) for i in range(args.distinct)])
        for P in args.pairs:
            rep = -(-P // args.distinct)
            F1, F2, K1, K2, n1, n2 = (torch.from_numpy(np.tile(x, (rep,) + (1,) * (x.ndim - 1))[:P].copy()).cuda() for x in base)
            pid = torch.arange(P, dtype=torch.int32, device="cuda")
            corr = torch.empty((P, nk, 2), dtype=torch.int32, device="cuda")
            ncorr = torch.empty(P, dtype=torch.int32, device="cuda")
            nb = lib.egonn_registration_scratch_bytes(P, nk, H)
            scratch = torch.empty(nb // 8 + 1, dtype=torch.int64, device="cuda")
            T = torch.empty((P, 4, 4), dtype=torch.float64, device="cuda")
            inl = torch.empty(P, dtype=torch.int32, device="cuda")
            fit, rmse = torch.empty(P, dtype=torch.float64, device="cuda"), torch.empty(P, dtype=torch.float64, device="cuda")
            st = _lib._stream()
            p = lambda t: t.data_ptr()                                     # noqa: E731

            mscratch = _lib.scratch(lib.egonn_match_mutual_scratch_bytes(P, nk), "cuda")

            def match():
                _lib.check(lib.egonn_match_mutual(p(F1), p(F2), p(n1), p(n2), P, nk, F1.shape[2], p(corr), p(ncorr), p(mscratch),
                                                  mscratch.numel() * 8, st))

            def ransac():
                _lib.check(lib.egonn_ransac_pairs(p(K1), p(K2), p(n1), p(n2), p(corr), p(ncorr), p(pid), P, nk, H, 0, 0.5,
                                                  p(scratch), scratch.numel() * 8, None, None, st))

            def finish():
                _lib.check(lib.egonn_registration_finish(p(K1), p(K2), p(n1), p(n2), p(corr), p(ncorr), p(pid), P, nk, H, 0, 0.5,
                                                         p(scratch), scratch.numel() * 8, None, 0.5, p(T), p(inl), p(fit), p(rmse),
                                                         None, None, None, None, None, None, None, st))

            reps, burst = (5, 2) if P >= 1024 else (10, 50)
            row = {"n_k": nk, "pairs": P, "hypotheses": H, "mean_n_corr": None}
            total = 0.0
            for name, fn in (("match_mutual", match), ("ransac_pairs", ransac), ("registration_finish", finish)):
                med, lo, hi = _time(fn, 3, reps, burst)
                row[name + "_us"] = {"median": med * 1e3, "min": lo * 1e3, "max": hi * 1e3, "windows": reps,
                                     "launches_per_window": burst}
                total += med
            row["mean_n_corr"] = float(ncorr.float().mean())
            row["inlier_share_of_keypoints"] = float(fit.mean())
            row["pairs_per_s"] = P / (total * 1e-3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "workload": "planted pairs, 30-60 % outliers, D = 128",
           "timer": "device events around a window of back-to-back launches of one kernel, per-launch time = window / launches; "
                    "median over the windows after 3 warm-up launches", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
