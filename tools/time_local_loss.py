"""Time the local phase of the training step: the per-pair driver `KeypointCorrLoss` against the one-call
`BatchedKeypointCorrLoss` on the same inputs (8 pairs, ~945 keypoints and 50 000 cloud points per scan, forward + backward),
and with --step the full step `EgoNNTrainStep` against the step assembled by hand on the per-pair driver (32 scans + 8 pairs).

Every variant runs in a fresh child process under its own time limit.  Per variant: the HOST WALL time per call with a final
synchronise (the per-pair driver is bound by host synchronisations, device events alone would flatter it) and the device-event
time, both as the median over the calls after the warm-up.  Records, not gates.  Writes one JSON file.

    python tools/time_local_loss.py --out profiles/local_loss_timing.json [--commit HASH] [--step]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def make_pair(rng, n1, n2, m1, m2, overlap=0.7, noise=0.05):
    """two clouds of a scene seen from two poses + regressed keypoints / saliencies / descriptors of both (the generator of
    tests/golden/make_golden_losses.py at the workload's sizes)"""
    ang = rng.uniform(-0.6, 0.6)
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    t = rng.uniform(-3, 3, 3) * np.array([1, 1, 0.1])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    sc = np.array([1, 1, 0.15])
    pc1 = rng.uniform(-30, 30, (m1, 3)) * sc
    pc2 = np.concatenate([pc1[: m2 // 2] @ R.T + t, rng.uniform(-30, 30, (m2 - m2 // 2, 3)) * sc])
    kp1 = pc1[rng.choice(m1, n1, replace=False)] + rng.normal(0, noise, (n1, 3))
    ns = int(overlap * min(n1, n2))
    kp2 = np.concatenate([kp1[:ns] @ R.T + t + rng.normal(0, noise, (ns, 3)),
                          pc2[rng.choice(m2, n2 - ns, replace=False)] + rng.normal(0, noise, (n2 - ns, 3))])
    d1 = _unit(rng.standard_normal((n1, 128)))
    d2 = _unit(np.concatenate([d1[:ns] + 0.4 * rng.standard_normal((ns, 128)), rng.standard_normal((n2 - ns, 128))]))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()      # noqa: E731
    return dict(pc1=f(pc1), pc2=f(pc2), kp1=f(kp1), kp2=f(kp2), sigma1=f(rng.uniform(0.05, 1.5, (n1, 1))),
                sigma2=f(rng.uniform(0.05, 1.5, (n2, 1))), desc1=f(d1), desc2=f(d2), M=f(M))


def _time(call, warmup, reps):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    wall, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    q = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "calls": len(v)}   # noqa: E731
    return {"wall_ms_per_call": q(wall), "device_ms_per_call": q(dev)}


def _child_loss(args):
    from egonn_amd import local_loss as L
    rng = np.random.default_rng(31)
    ps = [make_pair(rng, args.keypoints, args.keypoints, args.points, args.points) for _ in range(args.pairs)]
    for p in ps:
        for k in ("kp1", "kp2", "sigma1", "sigma2", "desc1", "desc2"):
            p[k].requires_grad_(True)
    fn = L.make_local_loss(batched=(args.child == "batched"))
    c1, c2 = torch.cat([p["pc1"] for p in ps]), torch.cat([p["pc2"] for p in ps])
    Ms = torch.stack([p["M"] for p in ps])
    Ms = Ms if args.child == "batched" else Ms.cpu()          # the per-pair driver takes host transforms (T_gt of the collate)
    lens = [(len(p["pc1"]), len(p["pc2"])) for p in ps]
    keep = {}

    def call():
        for p in ps:
            for k in ("kp1", "kp2", "sigma1", "sigma2", "desc1", "desc2"):
                p[k].grad = None
        loss, metrics = fn(c1, [p["kp1"] for p in ps], [p["sigma1"] for p in ps], [p["desc1"] for p in ps],
                           c2, [p["kp2"] for p in ps], [p["sigma2"] for p in ps], [p["desc2"] for p in ps], Ms, lens)
        loss.backward()
        keep["loss"] = loss
    row = _time(call, args.warmup, args.reps)
    row["loss"] = float(keep["loss"])
    return row


def _child_step(args):
    from egonn_amd import ModelParams, model_factory, local_loss as L
    from egonn_amd.synth import lidar_scan, planted_scan_pair, seeded_state_dict
    from egonn_amd.train import EgoNNTrainStep, TrainStep
    model = model_factory(ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.1))
    sd = seeded_state_dict(7, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to("cuda:0")
    q = model.quantizer

    def batch(clouds):
        cs = [q(torch.from_numpy(c))[0] for c in clouds]
        coords = torch.cat([torch.cat([torch.full((len(c), 1), b, dtype=torch.int32), c.int()], 1) for b, c in enumerate(cs)])
        return {"coords": coords.cuda(), "features": torch.ones((len(coords), 1), device="cuda"), "batch_size": len(cs)}
    B = args.scans
    g = batch([lidar_scan(200 + i, n_points=args.points) for i in range(B)])
    pos = torch.zeros((B, B), dtype=torch.bool)
    for i in range(0, B - 1, 2):
        pos[i, i + 1] = pos[i + 1, i] = True
    neg = ~(pos | torch.eye(B, dtype=torch.bool))
    pos, neg = pos.cuda(), neg.cuda()
    prs = [planted_scan_pair(300 + i, args.points) for i in range(args.pairs)]
    local = {"anc_batch": batch([p[0] for p in prs]), "pos_batch": batch([p[1] for p in prs]),
             "anc_pcd": torch.cat([torch.from_numpy(p[0]) for p in prs]).cuda(),
             "pos_pcd": torch.cat([torch.from_numpy(p[1]) for p in prs]).cuda(),
             "T_gt": torch.stack([torch.from_numpy(np.asarray(p[2])).float() for p in prs]),
             "len_batch": [[len(p[0]), len(p[1])] for p in prs]}
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    kw = dict(beta=2.0, dist_th=2.0)        # an untrained model's keypoints sit on the supervoxel grid: keep the correspondence term busy
    if args.child == "step_batched":
        local["T_gt"] = local["T_gt"].cuda()
        step = EgoNNTrainStep(model, opt, local_loss_fn=L.BatchedKeypointCorrLoss(**kw))
        call = lambda: step(g, pos, neg, local)      # noqa: E731
    else:
        gstep, fn = TrainStep(model, opt), L.KeypointCorrLoss(**kw)

        def call():
            gstep(g, pos, neg, step_optimizer=False)
            y1 = model(local["anc_batch"], context_slot=1)
            y2 = model(local["pos_batch"], context_slot=2)
            ll, _ = fn(local["anc_pcd"], y1["keypoints"], y1["sigma"], y1["descriptors"], local["pos_pcd"], y2["keypoints"],
                       y2["sigma"], y2["descriptors"], local["T_gt"], local["len_batch"])
            ll.backward()
            opt.step()
    return _time(call, args.warmup, args.reps)


def _spawn(args, variant, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", variant, "--pairs", str(args.pairs),
           "--keypoints", str(args.keypoints), "--points", str(args.points), "--scans", str(args.scans), "--warmup", str(args.warmup),
           "--reps", str(args.reps), "--out", "-"]
    pr = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if pr.returncode != 0:
        return {"error": f"child exited with {pr.returncode}", "tail": pr.stderr[-600:]}, pr.returncode
    return json.loads(pr.stdout.strip().splitlines()[-1]), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--keypoints", type=int, default=945)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--scans", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step", action="store_true", help="also time EgoNNTrainStep against the hand-assembled step")
    ap.add_argument("--child", default="", help="internal: run one variant in this process and print its JSON row")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    if args.child:
        row = _child_step(args) if args.child.startswith("step_") else _child_loss(args)
        print(json.dumps(row), flush=True)
        return
    import __graft_entry__ as g
    g.build()
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit,
           "workload": f"{args.pairs} pairs, {args.keypoints} keypoints and {args.points} cloud points per scan (make_pair generator, "
                       f"seed 31), forward + backward; step: {args.scans} lidar_scan scans + {args.pairs} planted_scan_pair pairs",
           "timer": f"fresh child process per variant; host wall time per call ending in a device synchronise, and device events "
                    f"around the call; median over {args.reps} calls after {args.warmup} warm-up calls", "rows": {}}
    for variant, limit in [("per_pair", 240), ("batched", 240)] + ([("step_per_pair", 400), ("step_batched", 400)] if args.step else []):
        row, rc = _spawn(args, variant, limit)
        out["rows"][variant] = row
        print(variant, json.dumps(row), flush=True)
        if rc != 0:          # a fault, an abort or a time limit: start nothing more on the device
            break
    r = out["rows"]
    if "batched" in r and "error" not in r["batched"] and "error" not in r["per_pair"]:
        out["speedup_wall"] = r["per_pair"]["wall_ms_per_call"]["median"] / r["batched"]["wall_ms_per_call"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
