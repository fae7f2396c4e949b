#!/usr/bin/env python
"""Time of one MinkLoc train step (forward + backward of a linear functional of the descriptors, no optimiser) with NetVLAD-GC
pooling beside the same step with GeM pooling, on the same batch: --batch scans of --points points, Cartesian 0.3 m.
Information only (profiles/pooling_train_timing.json); nothing is gated on it.

    python tools/time_pooling_train.py --out profiles/pooling_train_timing.json
    rocprofv3 --kernel-trace --stats -d OUT -o pt -- python tools/time_pooling_train.py --trace     # per-kernel rows

Timing: --windows windows of --steps back-to-back steps between device events after --warmup steps; median and spread of
the windows."""
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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=20_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="a few NetVLAD-GC steps only (run under the kernel tracer)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    g.build()
    import egonn_amd
    from egonn_amd.synth import lidar_scan, seeded_state_dict
    dev = torch.device("cuda", 0)
    res = {"batch": args.batch, "points_per_scan": args.points, "quantization_step": 0.3, "device": torch.cuda.get_device_name(0),
           "steps_per_window": args.steps, "windows": args.windows}
    for method in (("netvladgc",) if args.trace else ("GeM", "netvladgc")):
        mp = egonn_amd.ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=0.3, pooling=method,
                                   output_dim=256)
        m = egonn_amd.model_factory(mp)
        sd = seeded_state_dict(1, {k: tuple(v.shape) for k, v in m.state_dict().items()})
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m = m.to(dev).train()
        cs = []
        for b in range(args.batch):
            c, _ = mp.quantizer(torch.from_numpy(lidar_scan(1000 + b, args.points)).to(dev))
            cs.append(torch.cat([torch.full((len(c), 1), b, dtype=torch.int32, device=dev), c.to(torch.int32)], 1))
        coords = torch.cat(cs)
        batch = {"coords": coords, "features": torch.ones((len(coords), 1), device=dev), "batch_size": args.batch}
        R = torch.randn((args.batch, 256), device=dev, generator=torch.Generator(device=dev).manual_seed(1))

        def step():
            m.zero_grad(set_to_none=True)
            (m(batch)["global"] * R).sum().backward()

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        if args.trace:
            continue
        ms = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
        res[method] = {"ms_per_step_median": round(float(np.median(ms)), 3), "ms_per_step_min": round(min(ms), 3),
                       "ms_per_step_max": round(max(ms), 3), "voxels": int(len(coords))}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
