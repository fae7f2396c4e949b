"""Time the MinkLoc-type models on the device: MinkLoc3D and MinkLoc(ECABasicBlock) on batches of 16 synthetic scans of 50 k
points at 0.3 m voxels.  Per model:

  eager            model(batch): the per-operator path (plan from coordinates + ~30 library calls), the baseline
  one_call         GlobalExtractor.extract_packed: voxelise + egonn_minkfpn_forward, eager plans
  forward_only     the forward alone on an existing plan: per-operator walk vs the one call, exact vs split top-down step
  replay_1 / _4    GlobalExtractor.graph replay with one batch and with four batches in flight (one context + stream each)
  topdown_step     egonn_topdown_step on the level-2 map of that batch, split vs exact arithmetic (the operator packs its
                   kernels per call in both modes; `forward_only` has the packed comparison)

Method: warm-up, then windows of back-to-back calls between two device events (replay_4: host clock around launches that end
in a device synchronise), median over the windows; the two sides of a comparison alternate window by window.  Every model
runs in a child process under its own time limit; a child that does not end cleanly stops the tool.  Records, not gates.

    python tools/time_minkloc.py --out profiles/minkloc_timing.json [--commit HASH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MODELS = {"MinkLoc3D": dict(model="MinkLoc3D"), "MinkLoc_ECABasicBlock": dict(model="MinkLoc", block="ECABasicBlock")}


def _windows(fn, calls, windows, stream=None):
    """median / min / max ms per call over `windows` windows of `calls` back-to-back calls"""
    import numpy as np
    import torch
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "windows": windows,
            "calls_per_window": calls}


def _alternate(fns, calls, windows):
    """{name: stats} with the windows of the named sides interleaved (A B A B ...)"""
    import numpy as np
    import torch
    ms = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / calls)
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "windows": windows,
                "calls_per_window": calls} for k, v in ms.items()}


def child(args):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    from egonn_amd import graph
    from egonn_amd.synth import lidar_scan, seeded_state_dict
    B, W, N = args.batch, args.calls, args.windows
    mp = egonn_amd.ModelParams(coordinates="cartesian", quantization_step=0.3, **MODELS[args.child])
    m = egonn_amd.model_factory(mp)
    sd = seeded_state_dict(17, {k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to("cuda").eval()
    ex = egonn_amd.GlobalExtractor(m)
    scans = [torch.from_numpy(lidar_scan(100 + i, n_points=args.n_points)) for i in range(B)]
    offsets = [0]
    for s in scans:
        offsets.append(offsets[-1] + len(s))
    points = torch.cat(scans).cuda().contiguous()
    ctx = m.context(0)
    q = ex.quantizer
    ctx.voxelize(points, offsets, q.mode, q.step)
    rows = [ctx.level_count(l) for l in range(8)]
    coords = ctx.level_coords(0).clone()
    batch = {"coords": coords, "features": torch.ones((len(coords), 1), device="cuda"), "batch_size": B}
    out = {"model": args.child, "batch": B, "points_per_scan": args.n_points, "rows_per_level": rows}

    # outputs first: the one call against the eager path on this batch
    with torch.no_grad():
        want = m(batch)["global"].clone()
    got = ex.extract_packed(points, offsets)["global"].clone()
    m.split_topdown = True
    got_split = ex.extract_packed(points, offsets)["global"].clone()
    m.split_topdown = False
    ctx.plan_status()
    cos = lambda a, b: float((1 - torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=1)).max())      # noqa: E731
    out["max_cosine_err_vs_eager"] = {"one_call": cos(got, want), "one_call_split_topdown": cos(got_split, want)}

    def eager():
        with torch.no_grad():
            m(batch)

    def one_call():
        ex.extract_packed(points, offsets)
    for fn in (eager, one_call):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out.update(_alternate({"eager": eager, "one_call": one_call}, W, N))

    # the forward alone on the plan the context holds (voxelised above)
    ctx.voxelize(points, offsets, q.mode, q.step)
    ones = torch.ones((rows[0], 1), device="cuda")
    pooling = m.pooling.pooling if hasattr(m.pooling, "pooling") else m.pooling
    outs = ex._outputs(ctx, B, False)

    def walk():
        with torch.no_grad():
            level, x = m.backbone.run(ctx, ones)
            graph.pool(graph.EvalOps(ctx), level, x, pooling, m.pooling_method)

    def call_exact():
        m.split_topdown = False
        ex._forward(ctx, outs)

    def call_split():
        m.split_topdown = True
        ex._forward(ctx, outs)
    for fn in (walk, call_exact, call_split):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out["forward_only"] = _alternate({"per_operator": walk, "one_call_exact_topdown": call_exact, "one_call_split_topdown": call_split},
                                     W, N)
    m.split_topdown = False

    # egonn_topdown_step on the level-2 map of this batch, kernels in reference layout (packed per call in both modes)
    gen = torch.Generator().manual_seed(3)
    F, lat = m.backbone.lateral_dim, m.backbone.conv1x1[1].kernel.shape[0]
    xc = torch.randn((rows[3], F), generator=gen).cuda()
    xl = torch.randn((rows[2], lat), generator=gen).cuda()
    wt, wl = m.backbone.tconvs[0].kernel.detach(), m.backbone.conv1x1[1].kernel.detach()

    def step_split():
        ctx.set_exact_fp32(False)
        ctx.topdown_step(2, xc, wt, xl, wl, rows=rows[2])

    def step_exact():
        ctx.set_exact_fp32(True)
        ctx.topdown_step(2, xc, wt, xl, wl, rows=rows[2])
    for fn in (step_split, step_exact):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out["topdown_step"] = dict(_alternate({"split": step_split, "exact": step_exact}, W, N), rows_out=rows[2], rows_coarse=rows[3], C=F,
                               Cl=lat, flop=2.0 * rows[2] * F * (F + lat))
    ctx.set_exact_fp32(False)

    # graph replay: one batch in flight, then four (a context and a stream each)
    caps = ex.calibrate(points, offsets, margin=1.3)
    gxs = [ex.graph(B, offsets[-1] + 1024, caps, slot=10 + i) for i in range(4)]
    for gx in gxs:
        gx.run(points, offsets)
        gx.status()
    g0 = gxs[0]
    with torch.cuda.stream(g0.stream):
        for _ in range(3):
            g0.replay()
        g0.stream.synchronize()
        out["replay_1"] = _windows(g0.replay, W, N, g0.stream)
    ms = []
    for _ in range(N):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(W):
            for gx in gxs:
                gx.replay()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / (W * len(gxs)))
    out["replay_4"] = {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "windows": N,
                       "calls_per_window": W * len(gxs), "note": "ms per batch, host clock around 4 x W replays + synchronise"}
    for gx in gxs:
        gx.status()
    assert torch.equal(gxs[0].out["global"], gxs[3].out["global"])
    out["replay_max_cosine_err_vs_eager"] = cos(gxs[0].out["global"], want)
    for k in ("eager", "one_call", "replay_1", "replay_4"):
        out[k]["scans_per_s"] = B / out[k]["median_ms"] * 1e3
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--n_points", type=int, default=50000)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds a model's child process may take")
    ap.add_argument("--child", default="", help="(internal) the model this process times")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in MODELS:
        part = os.path.abspath(args.out) + "." + name + ".part"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", part, "--batch", str(args.batch), "--n_points",
               str(args.n_points), "--calls", str(args.calls), "--windows", str(args.windows)]
        try:
            pr = subprocess.run(cmd, cwd=REPO, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"time_minkloc: {name} did not end within {args.limit} s; nothing more is started")
        if pr.returncode != 0:
            sys.exit(f"time_minkloc: {name} ended with status {pr.returncode}; nothing more is started")
        with open(part) as f:
            rows.append(json.load(f))
        os.remove(part)
    import torch
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit,
           "workload": f"egonn_amd.synth.lidar_scan(100 + i, {args.n_points}), batch {args.batch}, Cartesian 0.3 m voxels, seeded weights",
           "timer": "device events around windows of back-to-back calls, median over the windows after 3 warm-up calls; compared "
                    "sides alternate window by window; replay_4: host clock around launches that end in a device synchronise",
           "rows": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
