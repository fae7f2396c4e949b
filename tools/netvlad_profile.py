#!/usr/bin/env python
"""Time of MinkLoc's NetVLAD / NetVLAD-GC pooling (egonn_netvlad, four launches) at MinkLoc's default sizes:
feature_size = output_dim = 256, 64 clusters, batch 16 x 50 000-point scans, Cartesian 0.1 m (the metric stand-in of the
reference's normalised clouds, as in tools/bench_workloads.py).  The pooling runs on the backbone output of one MinkLoc
forward, --iters times per method; run it under the kernel tracer for per-launch figures:

    rocprofv3 --kernel-trace --stats -d OUT -o nv -- python tools/netvlad_profile.py

It prints the pooling level's rows, the algorithmic FLOP / bytes and the event-timed mean per call."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as g  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=50_000)
    args = ap.parse_args()
    g.build()
    import egonn_amd
    from egonn_amd.synth import lidar_scan, seeded_state_dict
    dev = torch.device("cuda", 0)
    res = {}
    for method in ("netvlad", "netvladgc"):
        mp = egonn_amd.ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=0.1, pooling=method,
                                   output_dim=256)
        m = egonn_amd.model_factory(mp)
        sd = seeded_state_dict(1, {k: tuple(v.shape) for k, v in m.state_dict().items()})
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m = m.to(dev).eval()
        m.coord_bits = 12
        cs = []
        for b in range(args.batch):
            c, _ = mp.quantizer(torch.from_numpy(lidar_scan(1000 + b, args.points)).to(dev))
            cs.append(torch.cat([torch.full((len(c), 1), b, dtype=torch.int32, device=dev), c.to(torch.int32)], 1))
        coords = torch.cat(cs)
        y = m({"coords": coords, "features": torch.ones((len(coords), 1), device=dev), "batch_size": args.batch})
        ctx = m.context()
        with torch.no_grad():
            level, x = m.backbone.run(ctx, ctx.gather_input(torch.ones((len(coords), 1), device=dev)))
            pool = m.pooling.pooling
            out = pool.run(ctx, level, x)
            assert torch.equal(out, y["global"])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                pool.run(ctx, level, x)
            e1.record()
            torch.cuda.synchronize()
        n, c = x.shape
        rows = np.diff(ctx.level_batch_offsets(level))
        flop = 4.0 * n * c * 64 + 2.0 * args.batch * c * 64 * 256
        res[method] = {"level": level, "rows": int(n), "rows_per_scan_max": int(rows.max()), "channels": int(c),
                       "ms_per_call_incl_bn_fold": round(e0.elapsed_time(e1) / args.iters, 4),
                       "assign_aggregate_gflop": round(4.0 * n * c * 64 / 1e9, 3), "total_gflop": round(flop / 1e9, 3),
                       "x_mb": round(n * c * 4 / 1e6, 2), "hidden1_mb": round(c * 64 * 256 * 4 / 1e6, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
