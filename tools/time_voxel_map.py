"""Time the voxel map on the device by the method of tools/time_pose_graph.py: device events around whole
calls, warm-up calls first, the median of --reps.  Three workloads, each next to the plain torch composition on the same
device (keys by tensor arithmetic, torch.unique(return_inverse=True), index_add_); the composition is the yardstick, not a
bar, and it computes less: no observation counts, no status, no capacity rule.

  integrate   --obs observations of --points points each: views of one synth.lidar_scan scene from poses 1 m apart, 0.2 m voxels
  merge       a map of --map_voxels records (random cells of a 400 m x 400 m x 3.2 m slab) with --chunk_voxels records, half of
              whose keys are in the map already
  submaps     one select call of --boxes boxes of 30 m half extent on that map

    python tools/time_voxel_map.py --out profiles/voxel_map_timing.json [--commit HASH]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from time_pose_graph import _timed

BIAS, ONE = 1 << 20, 1 << 30


def views(n_obs, n_points, seed=1):
    """-> bank (n_obs * n_points, 3) f64 in the scan frames, offsets, poses (scan -> world): poses 1 m apart on a gentle curve"""
    from egonn_amd.synth import lidar_scan
    scene = lidar_scan(seed, n_points=4 * n_points).astype(np.float64)
    rng = np.random.default_rng(seed)
    poses = np.tile(np.eye(4), (n_obs, 1, 1))
    clouds = []
    for k in range(n_obs):
        a = 0.01 * k
        poses[k, :3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        poses[k, :3, 3] = [0.2 * k, 0.001 * k * k, 0.0]
        world = scene[rng.choice(len(scene), size=n_points, replace=False)] + rng.normal(0, 0.02, (n_points, 3))
        clouds.append((world - poses[k, :3, 3]) @ poses[k, :3, :3])
    off = np.arange(n_obs + 1, dtype=np.int64) * n_points
    return np.concatenate(clouds), off, poses


def random_records(n, seed, extent=(2000, 2000, 16)):
    """n records on random cells of a slab of `extent` voxels around the origin, sorted by key"""
    rng = np.random.default_rng(seed)
    cells = np.unique(rng.integers(0, extent[0] * extent[1] * extent[2], int(n * 1.03)))[:n]
    x, y, z = cells // (extent[1] * extent[2]), cells // extent[2] % extent[1], cells % extent[2]
    keys = ((x - extent[0] // 2 + BIAS) << 42) | ((y - extent[1] // 2 + BIAS) << 21) | (z - extent[2] // 2 + BIAS)
    count = rng.integers(1, 200, len(keys)).astype(np.int32)
    return {"keys": np.sort(keys.astype(np.int64)), "sums": rng.integers(0, ONE, (len(keys), 3)) * count[:, None].astype(np.int64),
            "count": count, "obs": np.minimum(count, rng.integers(1, 30, len(keys))).astype(np.int32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--obs", type=int, default=64)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--map_voxels", type=int, default=1000000)
    ap.add_argument("--chunk_voxels", type=int, default=200000)
    ap.add_argument("--boxes", type=int, default=64)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd as ea
    from egonn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)                          # noqa: E731
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    voxel = float(args.voxel)
    status = torch.zeros((), dtype=torch.int32, device=dev)

    def rec(rows):
        return {"keys": torch.empty(rows, dtype=torch.int64, device=dev), "sums": torch.empty((rows, 3), dtype=torch.int64, device=dev),
                "count": torch.empty(rows, dtype=torch.int32, device=dev), "obs": torch.empty(rows, dtype=torch.int32, device=dev),
                "n": torch.zeros((), dtype=torch.int64, device=dev)}

    def up(r):
        out = rec(len(r["keys"]))
        for f in ("keys", "sums", "count", "obs"):
            out[f].copy_(cu(r[f]))
        out["n"].fill_(len(r["keys"]))
        return out

    ptrs = lambda r: (r["keys"].data_ptr(), r["sums"].data_ptr(), r["count"].data_ptr(), r["obs"].data_ptr())     # noqa: E731

    # ------------------------------------------------------------------ integrate
    bank_np, off_np, poses_np = views(args.obs, args.points)
    n_pts = len(bank_np)
    bank, off, poses = cu(bank_np), cu(off_np), cu(poses_np)
    pick = torch.arange(args.obs, dtype=torch.int32, device=dev)
    chunk = rec(n_pts)
    s_int = _lib.scratch(lib.egonn_voxel_map_integrate_scratch_bytes(n_pts, args.obs), dev)

    def integrate():
        _lib.call(dev, lib.egonn_voxel_map_integrate, bank.data_ptr(), n_pts, off.data_ptr(), args.obs, pick.data_ptr(), poses.data_ptr(),
                  args.obs, org, voxel, n_pts, *ptrs(chunk), n_pts, chunk["n"].data_ptr(), status.data_ptr(), s_int.data_ptr(),
                  s_int.numel() * 8)

    obs_of = torch.arange(args.obs, device=dev).repeat_interleave(args.points)

    def torch_integrate():
        R, t = poses[obs_of, :3, :3], poses[obs_of, :3, 3]
        s = (((R[:, :, 0] * bank[:, 0:1] + R[:, :, 1] * bank[:, 1:2]) + R[:, :, 2] * bank[:, 2:3]) + t) / voxel      # origin = 0
        f = torch.floor(s)
        q = torch.clamp(torch.floor((s - f) * float(ONE)).to(torch.int64), max=ONE - 1)
        i = f.to(torch.int64) + BIAS
        keys = (i[:, 0] << 42) | (i[:, 1] << 21) | i[:, 2]
        uniq, inv = torch.unique(keys, return_inverse=True)
        sums = torch.zeros((len(uniq), 3), dtype=torch.int64, device=dev).index_add_(0, inv, q)
        count = torch.zeros(len(uniq), dtype=torch.int32, device=dev).index_add_(0, inv, torch.ones_like(inv, dtype=torch.int32))
        return uniq, sums, count

    integrate()
    uniq, sums, count = torch_integrate()
    torch.cuda.synchronize()
    n_chunk = int(chunk["n"])
    same = bool(n_chunk == len(uniq) and (chunk["keys"][:n_chunk] == uniq).all() and (chunk["count"][:n_chunk] == count).all())
    t_int, t_int_torch = _timed(integrate, 3, args.reps), _timed(torch_integrate, 3, args.reps)
    res_int = {"observations": args.obs, "points": n_pts, "voxels": n_chunk, "status": int(status),
               "same_keys_and_counts_as_torch": same, "scratch_bytes": int(s_int.numel() * 8), "ms": t_int, "torch_ms": t_int_torch,
               "points_per_s": n_pts / (t_int["median"] * 1e-3), "torch_points_per_s": n_pts / (t_int_torch["median"] * 1e-3)}
    print(json.dumps(res_int), flush=True)

    # ------------------------------------------------------------------ merge
    A_np = random_records(args.map_voxels, 2)
    B_np = random_records(args.chunk_voxels, 3)
    half = len(B_np["keys"]) // 2
    B_np["keys"] = np.sort(np.unique(np.concatenate([B_np["keys"][:half], A_np["keys"][:: max(1, len(A_np["keys"]) // half)][:half]])))
    B_np = {k: (v[: len(B_np["keys"])] if k != "keys" else v) for k, v in B_np.items()}
    A, B = up(A_np), up(B_np)
    n_a, n_b = len(A_np["keys"]), len(B_np["keys"])
    out = rec(n_a + n_b)
    s_mrg = _lib.scratch(lib.egonn_voxel_map_merge_scratch_bytes(n_a, n_b, n_a + n_b), dev)

    def merge():
        _lib.call(dev, lib.egonn_voxel_map_merge, *ptrs(A), A["n"].data_ptr(), n_a, *ptrs(B), B["n"].data_ptr(), n_b, *ptrs(out),
                  n_a + n_b, out["n"].data_ptr(), status.data_ptr(), s_mrg.data_ptr(), s_mrg.numel() * 8)

    def torch_merge():
        uniq, inv = torch.unique(torch.cat([A["keys"], B["keys"]]), return_inverse=True)
        sums = torch.zeros((len(uniq), 3), dtype=torch.int64, device=dev).index_add_(0, inv, torch.cat([A["sums"], B["sums"]]))
        count = torch.zeros(len(uniq), dtype=torch.int32, device=dev).index_add_(0, inv, torch.cat([A["count"], B["count"]]))
        obs = torch.zeros(len(uniq), dtype=torch.int32, device=dev).index_add_(0, inv, torch.cat([A["obs"], B["obs"]]))
        return uniq, sums, count, obs

    merge()
    uniq, sums, count, obs = torch_merge()
    torch.cuda.synchronize()
    n_u = int(out["n"])
    same = bool(n_u == len(uniq) and (out["keys"][:n_u] == uniq).all() and (out["sums"][:n_u] == sums).all() and
                (out["count"][:n_u] == count).all() and (out["obs"][:n_u] == obs).all())
    t_mrg, t_mrg_torch = _timed(merge, 3, args.reps), _timed(torch_merge, 3, args.reps)
    res_mrg = {"map_voxels": n_a, "chunk_voxels": n_b, "union": n_u, "same_records_as_torch": same, "ms": t_mrg, "torch_ms": t_mrg_torch,
               "voxels_per_s": (n_a + n_b) / (t_mrg["median"] * 1e-3), "torch_voxels_per_s": (n_a + n_b) / (t_mrg_torch["median"] * 1e-3)}
    print(json.dumps(res_mrg), flush=True)

    # ------------------------------------------------------------------ submaps
    vm = ea.VoxelMap(voxel, origin=(0.0, 0.0, 0.0), capacity=n_a + n_b)
    vm._ensure()
    vm._buf[0], vm._cur = out, 0
    rng = np.random.default_rng(4)
    centers = cu(np.stack([rng.uniform(-150, 150, args.boxes), rng.uniform(-150, 150, args.boxes), np.zeros(args.boxes)], axis=1))
    first = vm.submaps(centers, 30.0)                                       # sizes the output
    cap = first["points"].shape[0]
    offsets = first["offsets"].cpu().numpy()

    def torch_submaps():
        k = out["keys"][:n_u]
        i = torch.stack([(k >> 42) & 0x1FFFFF, (k >> 21) & 0x1FFFFF, k & 0x1FFFFF], dim=1) - BIAS
        c = (i.to(torch.float64) + out["sums"][:n_u].to(torch.float64) / (out["count"][:n_u].to(torch.float64) * float(ONE))[:, None]) * voxel
        parts = []
        for b in range(args.boxes):
            m = ((c >= centers[b] - 30.0) & (c < centers[b] + 30.0)).all(dim=1)
            parts.append(c[m] - centers[b])
        return torch.cat(parts)

    ref_pts = torch_submaps()
    torch.cuda.synchronize()
    same = bool(ref_pts.shape[0] == cap and (ref_pts == first["points"]).all())
    t_sub = _timed(lambda: vm.submaps(centers, 30.0, capacity=cap), 3, args.reps)
    t_sub_torch = _timed(torch_submaps, 2, max(3, args.reps // 4))
    res_sub = {"boxes": args.boxes, "half_extent_m": 30.0, "map_voxels": n_u, "selected": int(cap), "same_points_as_torch": same,
               "largest_box": int(np.diff(offsets).max()), "ms": t_sub, "torch_ms": t_sub_torch}
    print(json.dumps(res_sub), flush=True)

    res = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "voxel_m": voxel,
           "timer": "device events around one whole call, 3 warm-up calls, median, min and max of the calls; the torch composition "
                    "(tensor arithmetic, torch.unique(return_inverse=True), index_add_) on the same device and inputs, checked equal "
                    "first; it computes no observation counts, status or capacity rule",
           "integrate": res_int, "merge": res_mrg, "submaps": res_sub}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
