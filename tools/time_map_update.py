"""Time the map update on the device by the method of tools/time_voxel_map.py: device events around whole
calls, 3 warm-up calls, the median of --reps (20).  The inputs are that tool's: --obs (64) views of --points (10 000) points of
one synth.lidar_scan scene from poses on a gentle curve, 0.2 m voxels for the voxel map and 1.0 m for the NDT layer.

  repose      `VoxelMap.repose` of 1, 8 and all observations (each call moves them between two sets of poses 5 cm and 2 mrad
              apart, so every timed call does the same work) on a tracked map with a reserved capacity, with and without
              moments, next to `build_map` of all observations from scratch: the remedy without repose
  integrate   egonn_voxel_map_integrate_moments next to egonn_voxel_map_integrate followed by egonn_ndt_accumulate over its
              keys (with the memsets of the three moment arrays that accumulate adds into), on all observations at 1.0 m
  follow      `insert` of 8 observations into a moments map of the other 56 + `NDTMap.update` + `finalize`, next to
              `build_ndt_map` of all 64 (two passes over the points); the 8 are removed again outside the timed window

Latencies of single calls, host work and synchronisations of the Python layer included.  No test asserts any of them.

    python tools/time_map_update.py --out profiles/map_update_timing.json [--commit HASH]
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
from time_voxel_map import views


def _timed_after(prepare, fn, warmup, reps):
    """_timed with `prepare` run (and waited for) before every call, outside the events"""
    ms = []
    for k in range(warmup + reps):
        prepare()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "calls": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--obs", type=int, default=64)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--ndt_voxel", type=float, default=1.0)
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
    n_obs, zero = args.obs, np.zeros(3)
    bank_np, off_np, poses = views(n_obs, args.points)
    n_pts = len(bank_np)
    bank = ea.CloudBank()
    bank.points, bank.host_offsets = cu(bank_np), [int(v) for v in off_np]
    res = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "observations": n_obs, "points": n_pts,
           "timer": "device events around one whole call, 3 warm-up calls, median, min and max of the calls; latencies of single "
                    "calls with the host work of the Python layer; both sides of a row in the same process on the same inputs"}

    # ------------------------------------------------------------------ repose against a rebuild
    moved = poses.copy()
    a = 0.002
    turn = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    moved[:, :3, :3] = turn @ poses[:, :3, :3]
    moved[:, :3, 3] += [0.05, -0.03, 0.01]
    t_build = _timed(lambda: ea.build_map(bank, poses, args.voxel, origin=zero), 3, args.reps)
    n_vox = ea.build_map(bank, poses, args.voxel, origin=zero).n_voxels
    res["build_map"] = {"ms": t_build, "voxels": n_vox, "voxel_m": args.voxel}
    print(json.dumps(res["build_map"]), flush=True)
    res["repose"] = []
    for moments in (False, True):
        for k in sorted({1, min(8, n_obs), n_obs}):
            vm = ea.VoxelMap(args.voxel, zero, capacity=2 * n_vox, moments=moments, track=True).insert(bank, poses)
            targets = [np.concatenate([moved[:k], poses[k:]]), poses]
            state = {"at": 0}

            def repose():
                n = vm.repose(bank, targets[state["at"] % 2])
                assert n == k, (n, k)
                state["at"] += 1

            t = _timed(repose, 3, args.reps)                                # 3 + reps is odd for reps = 20: the map ends at `moved`
            if state["at"] % 2:
                repose()
            want = ea.build_map(bank, poses, args.voxel, origin=zero)
            same = bool(vm.n_voxels == n_vox and vm.status == 0 and
                        all(torch.equal(vm.records[f][:n_vox], want.records[f][:n_vox]) for f in ("keys", "sums", "count", "obs")))
            row = {"moved": k, "moments": moments, "ms": t, "same_records_as_build_map_afterwards": same,
                   "build_map_over_repose": t_build["median"] / t["median"]}
            res["repose"].append(row)
            print(json.dumps(row), flush=True)

    # ------------------------------------------------------------------ one pass against two
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    voxel = float(args.ndt_voxel)
    bank_d, off_d, poses_d = bank.points, cu(off_np), cu(poses)
    pick = torch.arange(n_obs, dtype=torch.int32, device=dev)
    status = torch.zeros((), dtype=torch.int32, device=dev)
    missed = torch.zeros((), dtype=torch.int64, device=dev)
    i64 = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)                           # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)                           # noqa: E731
    R = {"keys": i64(n_pts), "sums": i64(n_pts, 3), "count": i32(n_pts), "obs": i32(n_pts), "s1": i64(n_pts, 3), "s2": i64(n_pts, 6),
         "n": torch.zeros((), dtype=torch.int64, device=dev)}
    cnt, s1, s2 = i32(n_pts), i64(n_pts, 3), i64(n_pts, 6)
    s_int = _lib.scratch(lib.egonn_voxel_map_integrate_moments_scratch_bytes(n_pts, n_obs), dev)
    s_acc = _lib.scratch(lib.egonn_ndt_accumulate_scratch_bytes(n_pts, n_obs), dev)
    head = (bank_d.data_ptr(), n_pts, off_d.data_ptr(), n_obs, pick.data_ptr(), poses_d.data_ptr(), n_obs, org, voxel, n_pts)
    four = (R["keys"].data_ptr(), R["sums"].data_ptr(), R["count"].data_ptr(), R["obs"].data_ptr())

    def one_pass():
        _lib.call(dev, lib.egonn_voxel_map_integrate_moments, *head, *four, R["s1"].data_ptr(), R["s2"].data_ptr(), n_pts,
                  R["n"].data_ptr(), status.data_ptr(), s_int.data_ptr(), s_int.numel() * 8)

    def two_passes():
        _lib.call(dev, lib.egonn_voxel_map_integrate, *head, *four, n_pts, R["n"].data_ptr(), status.data_ptr(), s_int.data_ptr(),
                  s_int.numel() * 8)
        cnt.zero_(), s1.zero_(), s2.zero_()
        _lib.call(dev, lib.egonn_ndt_accumulate, *head, R["keys"].data_ptr(), R["n"].data_ptr(), n_pts, cnt.data_ptr(), s1.data_ptr(),
                  s2.data_ptr(), missed.data_ptr(), status.data_ptr(), s_acc.data_ptr(), s_acc.numel() * 8)

    two_passes()
    one_pass()
    torch.cuda.synchronize()
    n = int(R["n"])
    same = bool(torch.equal(cnt[:n], R["count"][:n]) and torch.equal(s1[:n], R["s1"][:n]) and torch.equal(s2[:n], R["s2"][:n]))
    t_one, t_two = _timed(one_pass, 3, args.reps), _timed(two_passes, 3, args.reps)
    res["integrate"] = {"voxel_m": voxel, "voxels": n, "same_moments": same, "status": int(status), "integrate_moments_ms": t_one,
                        "integrate_then_ndt_accumulate_ms": t_two, "two_over_one": t_two["median"] / t_one["median"]}
    print(json.dumps(res["integrate"]), flush=True)

    # ------------------------------------------------------------------ following a growing map against a rebuild
    late = min(8, n_obs - 1)
    first, last = np.arange(n_obs - late), np.arange(n_obs - late, n_obs)
    t_two_pass = _timed(lambda: ea.build_ndt_map(bank, poses, voxel, origin=zero), 3, args.reps)
    t_one_pass = _timed(lambda: ea.build_ndt_map(bank, poses, voxel, origin=zero, moments=True), 3, args.reps)
    whole = ea.build_ndt_map(bank, poses, voxel, origin=zero)
    for reserved in (False, True):
        vm = ea.VoxelMap(voxel, zero, capacity=2 * whole.n_voxels if reserved else None, moments=True, track=True)
        vm.insert(bank, poses[first], first)
        ndt = ea.NDTMap.from_map(vm)

        def follow():
            vm.insert(bank, poses[last], last)
            ndt.update(vm).finalize()

        follow()
        torch.cuda.synchronize()
        n = whole.n_voxels
        same = bool(ndt.n_voxels == n and all(torch.equal(getattr(ndt, f)[:n], getattr(whole, f)[:n]) for f in ("keys", "cnt", "s1", "s2"))
                    and all(torch.equal(ndt.gaussians[f][:n], whole.gaussians[f][:n]) for f in ("mean", "info", "valid")))
        t = _timed_after(lambda: vm.remove(bank, poses[last], last), follow, 3, args.reps)
        row = {"reserved_capacity": reserved, "inserted": int(late), "held": int(len(first)), "voxels": n, "same_layer_as_build_ndt_map": same,
               "insert_update_finalize_ms": t, "build_ndt_map_ms": t_two_pass, "build_ndt_map_moments_ms": t_one_pass,
               "rebuild_over_follow": t_two_pass["median"] / t["median"]}
        res.setdefault("follow", []).append(row)
        print(json.dumps(row), flush=True)
        vm.remove(bank, poses[last], last)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
