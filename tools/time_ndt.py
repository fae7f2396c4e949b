"""Time the NDT layer on the device by the method of tools/time_voxel_map.py: device events around whole
calls, 3 warm-up calls, the median of --reps.  The scene is that tool's: --obs views of --points points each of one
synth.lidar_scan scene from poses on a gentle curve.  Timed: `NDTMap.accumulate` of all views, `finalize`, and
`NDTMap.register` of all views at once from perturbed start poses at neighbors 1 and 7; next to them, on the same scans and
start poses, `refine_against_map(method="icp")` against the 0.2 m voxel map: the yardstick, not a bar.  The mean Frobenius
distance of the end poses to the true ones is written next to each time.

    python tools/time_ndt.py --out profiles/ndt_timing.json [--commit HASH]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from time_pose_graph import _timed
from time_voxel_map import views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--obs", type=int, default=64)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--voxel", type=float, default=1.0)
    ap.add_argument("--icp_voxel", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd as ea
    dev = torch.device("cuda:0")
    bank_np, off_np, poses = views(args.obs, args.points)
    bank = ea.CloudBank()
    bank.points = torch.from_numpy(np.ascontiguousarray(bank_np)).to(dev)
    bank.host_offsets = [int(v) for v in off_np]
    pick = list(range(args.obs))
    rng = np.random.default_rng(7)
    starts = poses.copy()
    for k in range(args.obs):                                  # 0.01 rad about z, 0.1 m: what a GPS / odometry prior leaves
        a = rng.normal(0.0, 0.01)
        starts[k, :3, :3] = starts[k, :3, :3] @ np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        starts[k, :3, 3] += rng.normal(0.0, 0.1, 3)
    starts_dev = torch.from_numpy(starts).to(dev)
    origin = np.zeros(3)

    vm = ea.build_map(bank, poses, args.voxel, origin=origin)
    ndt = ea.NDTMap(vm)
    t_acc = _timed(lambda: ndt.accumulate(bank, poses), 3, args.reps)
    ndt = ea.NDTMap(vm).accumulate(bank, poses)                # the timed calls added their moments 23 times over
    t_fin = _timed(ndt.finalize, 3, args.reps)
    G = ndt.finalize()
    src = bank.gather(pick)

    def dist(p):
        return float(np.mean(np.linalg.norm((p.cpu().numpy() - poses).reshape(args.obs, -1), axis=1)))

    res = {"accumulate": {"ms": t_acc, "points": len(bank_np), "points_per_s": len(bank_np) / (t_acc["median"] * 1e-3)},
           "finalize": {"ms": t_fin, "voxels": ndt.n_voxels, "valid": int(G["n_valid"])},
           "start_distance": float(np.mean(np.linalg.norm((starts - poses).reshape(args.obs, -1), axis=1)))}
    for nb in (1, 7):
        r = ndt.register(src["points"], src["offsets"], starts_dev, neighbors=nb)
        t = _timed(lambda: ndt.register(src["points"], src["offsets"], starts_dev, neighbors=nb), 3, args.reps)
        res[f"register_neighbors_{nb}"] = {"ms": t, "scans": args.obs, "end_distance": dist(r["poses"]),
                                           "mean_iterations": float(r["iterations"].double().mean()),
                                           "mean_fitness": float(r["fitness"].mean()), "status_or": int(np.bitwise_or.reduce(r["status"].cpu().numpy()))}
        print(json.dumps(res[f"register_neighbors_{nb}"]), flush=True)
    vm_icp = ea.build_map(bank, poses, args.icp_voxel, origin=origin)
    r = ea.refine_against_map(vm_icp, bank, pick, starts_dev, method="icp")
    t = _timed(lambda: ea.refine_against_map(vm_icp, bank, pick, starts_dev, method="icp"), 3, args.reps)
    res["refine_against_map_icp"] = {"ms": t, "scans": args.obs, "map_voxels": vm_icp.n_voxels, "end_distance": dist(r["poses"]),
                                     "mean_fitness": float(r["fitness"].mean()), "status_or": int(np.bitwise_or.reduce(r["status"].cpu().numpy()))}
    print(json.dumps(res["refine_against_map_icp"]), flush=True)
    res.update({"device": torch.cuda.get_device_name(0), "commit": args.commit, "voxel_m": args.voxel, "icp_voxel_m": args.icp_voxel,
                "observations": args.obs, "points_per_view": args.points,
                "timer": "device events around one whole Python call, 3 warm-up calls, median, min and max of the calls; the ICP "
                         "yardstick is refine_against_map(method='icp') (submap crop with its sizing synchronisation, icp_pairs) on "
                         "the same scans and start poses; distances are mean Frobenius norms of pose differences"})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v["ms"]["median"] for k, v in res.items() if isinstance(v, dict) and "ms" in v}))


if __name__ == "__main__":
    main()
