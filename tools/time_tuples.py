"""Time the training-tuple path on the device.  Records, not gates.  Writes one JSON file with three measurements:

  radius_join        count sweep + scan + fill of `radius_neighbors` at N positions of a synthetic drive for the two default
                     radii (2 m and 10 m): device events around windows of repeated calls, median over the windows
  generate           `generate_training_tuples` on S synthetic scans of one scene (tests/tuples_data.py:planted_sequence, 50 k
                     points each): the bank (filter + downsample, once per scan) and the refinement (relative poses, gather, ICP in
                     chunks of 16 pairs, one copy back), host clock around calls that end in a device-to-host copy; pairs / s
  one_pair_icp       the same pairs through the existing one-pair `registration.icp()` (downsamples both clouds per pair, as
                     the reference's script does), on the same machine, for the ratio

    python tools/time_tuples.py --out profiles/tuples_timing.json [--commit HASH]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch


def _median(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "windows": len(v)}


def time_radius_join(n, radii, windows, calls):
    from egonn_amd import radius_neighbors
    from tests.tuples_data import trajectory
    xy = torch.from_numpy(trajectory(n, 1)).cuda()
    for _ in range(2):
        out = radius_neighbors(xy, None, list(radii), exclude_self=[True, False])
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            out = radius_neighbors(xy, None, list(radii), exclude_self=[True, False], check=False)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return {"positions": n, "radii": list(radii), "neighbours": [int(o["indices"].numel()) for o in out],
            "ms_per_join": _median(ms), "calls_per_window": calls,
            "timer": "device events around a window of whole radius_neighbors calls (count sweep for both radii, cumsum, the one "
                     "host read of the totals, two fills)"}


def time_generate(n_scans, n_points, pairs_per_call, reps, one_pair_limit):
    from egonn_amd import CloudBank, generate_training_tuples, icp, relative_poses
    from egonn_amd.tuples import MULRAN_CROP
    from tests.tuples_data import planted_sequence, zero_filtered
    raws, _, gps = planted_sequence(n_scans=n_scans, n_points=n_points)
    CloudBank().add(raws[:2])                                 # warm-up: code objects, allocator
    torch.cuda.synchronize()
    bank_s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        bank = CloudBank().add(raws)
        torch.cuda.synchronize()
        bank_s.append(time.perf_counter() - t0)
    generate_training_tuples(gps[:4], CloudBank().add(raws[:4]), negate_translation=False, pairs_per_call=pairs_per_call)
    gen_s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        tuples, stats = generate_training_tuples(gps, bank, negate_translation=False, pairs_per_call=pairs_per_call)
        gen_s.append(time.perf_counter() - t0)                # ends in the one device-to-host copy
    pairs = stats["pairs"]
    row = {"scans": n_scans, "raw_points_per_scan": n_points, "downsampled_points_per_scan": float(bank.sizes().mean()),
           "pairs": pairs, "pairs_per_call": pairs_per_call, "bank_s": _median(bank_s), "generate_s": _median(gen_s),
           "pairs_per_s_refinement": pairs / float(np.median(gen_s)),
           "pairs_per_s_with_bank": pairs / (float(np.median(gen_s)) + float(np.median(bank_s))),
           "fitness": stats["fitness"], "inlier_rmse": stats["inlier_rmse"], "status_counts": stats["status_counts"],
           "timer": "host clock around whole calls that end in a device synchronise; median of the repeats after a warm-up call"}
    # the same pairs, one at a time, through registration.icp() on crop-filtered clouds (what the reference's loop does per pair)
    ia = np.concatenate([np.full(len(tuples[i].positives), i) for i in range(n_scans)]).astype(np.int32)
    ib = np.concatenate([tuples[i].positives for i in range(n_scans)]).astype(np.int32)
    T0 = relative_poses(gps, ia, ib, negate_translation=False).cpu().numpy()
    lo, hi = (MULRAN_CROP[0], MULRAN_CROP[2], MULRAN_CROP[4]), (MULRAN_CROP[1], MULRAN_CROP[3])

    def load_pc(raw):
        pc = zero_filtered(raw)
        keep = (pc[:, 0] > lo[0]) & (pc[:, 0] <= hi[0]) & (pc[:, 1] > lo[1]) & (pc[:, 1] <= hi[1]) & (pc[:, 2] > lo[2])
        return pc[keep]
    clouds = [load_pc(r) for r in raws]
    sel = list(range(min(pairs, one_pair_limit)))
    icp(clouds[ia[0]], clouds[ib[0]], T0[0])
    t0 = time.perf_counter()
    worst = 0.0
    for p in sel:
        T, _, _ = icp(clouds[ia[p]], clouds[ib[p]], T0[p])    # copies the result back: a device synchronise per pair
        worst = max(worst, float(np.abs(T - tuples[int(ia[p])].positives_poses[int(ib[p])]).max()))
    one_s = time.perf_counter() - t0
    one = {"pairs": len(sel), "s_total": one_s, "ms_per_pair": 1e3 * one_s / len(sel), "pairs_per_s": len(sel) / one_s,
           "max_abs_difference_to_generate": worst,
           "note": "registration.icp() per pair on host clouds cropped as load_pc does: upload, two downsamples and the ICP per pair"}
    return row, one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--positions", type=int, default=20000)
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--n_points", type=int, default=50000)
    ap.add_argument("--pairs_per_call", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--one_pair_limit", type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit}
    out["radius_join"] = time_radius_join(args.positions, (2.0, 10.0), args.windows, args.calls)
    print(json.dumps(out["radius_join"]), flush=True)
    out["generate"], out["one_pair_icp"] = time_generate(args.scans, args.n_points, args.pairs_per_call, args.reps, args.one_pair_limit)
    out["speedup_refinement_vs_one_pair"] = out["generate"]["pairs_per_s_refinement"] / out["one_pair_icp"]["pairs_per_s"]
    print(json.dumps({k: out[k] for k in ("generate", "one_pair_icp", "speedup_refinement_vs_one_pair")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
