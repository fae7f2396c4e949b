"""Time the relocalisation path on the device (method of tools/time_registration.py: device events around windows of
back-to-back calls, median of the windows after warm-up; two forms that are compared are ALTERNATED window by window in the
same run, so both see the same machine).

  1. matching  egonn_match_candidates (candidates read from the resident map by index) against torch gather of both
               operands + egonn_match_mutual, at (Q, k) = (1, 20), (16, 20), (256, 20), n_k = 128, D = 128.  Both entry points
               run the same tile / merge kernels (csrc/match.hip), so the "gather + match_mutual" column now times those
               kernels on gathered operands: the difference is the cost of the gather alone.  (Up to commit a2c5576
               egonn_match_mutual ran a kernel of its own, one workgroup per pair; DESIGN.md 3.14 keeps those figures.)
               The two forms must agree bit for bit.
  2. the whole verify_candidates call at the same points (default call, and with its buffers reused through out=)
  3. Relocalizer.localize at batch 1 and 16 on 50 k-point synthetic scans (seeded weights, a map of --map_scans scans)
  4. --spectral: the two geometric checks at the same points, on the same operands (the matcher's correspondences and the
               gathered keypoints of the call's pairs): egonn_ransac_pairs + egonn_registration_finish against
               egonn_spectral_verify, and the whole verify_candidates (buffers reused) under method="ransac" and "spectral".
               With this flag only these are measured, and the rows are APPENDED to the "spectral_rows" of an existing --out
               file, whose other content is kept.

    python tools/time_relocalize.py --out profiles/relocalize_timing.json [--commit HASH] [--spectral]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def _window(fn, burst):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(burst):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / burst


def _time_alternated(forms, warmup, reps, burst):
    """forms: {name: fn}.  -> {name: {median, min, max} in microseconds per call}; window i of every form before window i + 1"""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ms[name].append(_window(fn, burst))
    return {name: {"median": float(np.median(v)) * 1e3, "min": float(np.min(v)) * 1e3, "max": float(np.max(v)) * 1e3,
                   "windows": reps, "calls_per_window": burst} for name, v in ms.items()}


def _overlap(a, b):
    return not (a["max"] < b["min"] or b["max"] < a["min"])


def _spectral_row(ea, _lib, lib, km, qf, qk, qn, nn, H, row):
    """the operator against RANSAC + finish on one set of operands, then verify_candidates under both methods"""
    from egonn_amd import registration as reg
    dev = qf.device
    base = ea.verify_candidates(qf, qk, qn, km, nn, ransac_max_it=H)          # its buffers hold corr / n_corr / pair_ids
    spec = ea.verify_candidates(qf, qk, qn, km, nn, method="spectral")
    torch.cuda.synchronize()
    Q, k = nn.shape
    P, nk = Q * k, qf.shape[1]
    # the keypoint operands of all P pairs at once (verify_candidates gathers them chunk by chunk)
    kp1, kp2 = (torch.empty((P, nk, 3), dtype=torch.float32, device=dev) for _ in range(2))
    n1, n2, pids = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
    _lib.call(dev, lib.egonn_gather_candidates, qk.data_ptr(), qn.data_ptr(), km.keypoints.data_ptr(), km.counts.data_ptr(),
              nn.data_ptr(), None, Q, k, len(km), nk, kp1.data_ptr(), kp2.data_ptr(), n1.data_ptr(), n2.data_ptr(), pids.data_ptr())
    ops = (kp1.data_ptr(), kp2.data_ptr(), n1.data_ptr(), n2.data_ptr(), base["corr"].data_ptr(), base["n_corr"].data_ptr())
    scr_r = _lib.scratch(lib.egonn_registration_scratch_bytes(P, nk, H), dev)
    scr_s = _lib.scratch(lib.egonn_spectral_verify_scratch_bytes(P, nk), dev)
    from egonn_amd.relocalize import pair_keys
    flat = lambda d, m: {n: d[key].reshape(P, *d[key].shape[2:]) for n, key in pair_keys(m).items() if key in d}      # noqa: E731
    out_r, out_s = flat(base, "ransac"), flat(spec, "spectral")
    pid = pids.data_ptr()

    def ransac():
        reg.enqueue_ransac(dev, (*ops, pid), P, nk, H, 0, 0.5, scr_r, None, 0.5, out_r)

    def spectral():
        reg.enqueue_spectral(dev, ops, P, nk, reg.SPECTRAL_D_THR, reg.SPECTRAL_ITERATIONS, reg.SPECTRAL_SEED_RATIO, 0.5,
                             scr_s, None, 0.5, out_s)

    reps, burst = (7, 2) if P >= 1024 else (10, 40)
    row["operator_us"] = t = _time_alternated({"ransac_plus_finish": ransac, "spectral_verify": spectral}, 3, reps, burst)
    row["operator_ranges_overlap"] = _overlap(t["ransac_plus_finish"], t["spectral_verify"])

    def verify_ransac():
        ea.verify_candidates(qf, qk, qn, km, nn, ransac_max_it=H, out=base)

    def verify_spectral():
        ea.verify_candidates(qf, qk, qn, km, nn, method="spectral", out=spec)

    reps, burst = (5, 2) if P >= 1024 else (8, 10)
    row["verify_candidates_us"] = t = _time_alternated({"ransac": verify_ransac, "spectral": verify_spectral}, 2, reps, burst)
    row["verify_candidates_ranges_overlap"] = _overlap(t["ransac"], t["spectral"])
    torch.cuda.synchronize()
    row["verified_share"] = {"ransac": float((base["best_index"] >= 0).float().mean()),
                             "spectral": float((spec["best_index"] >= 0).float().mean())}
    row["rank0_won"] = {"ransac": float((base["best_rank"] == 0).float().mean()),
                               "spectral": float((spec["best_rank"] == 0).float().mean())}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="")
    ap.add_argument("--points", type=int, nargs="+", default=[1, 16, 256], help="queries per call, k candidates each")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--n_k", type=int, default=128)
    ap.add_argument("--map_entries", type=int, default=512)
    ap.add_argument("--hypotheses", type=int, default=10000)
    ap.add_argument("--map_scans", type=int, default=32)
    ap.add_argument("--scan_points", type=int, default=50000)
    ap.add_argument("--skip_localize", action="store_true")
    ap.add_argument("--spectral", action="store_true", help="time only the spectral check against RANSAC and append the rows")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd as ea
    from egonn_amd import _lib
    from egonn_amd.synth import lidar_scan, planted_keypoint_pair as planted_pair, seeded_state_dict
    lib = _lib.load()
    nk, k, M, H, D = args.n_k, args.k, args.map_entries, args.hypotheses, 128
    distinct = 64
    pairs = [planted_pair(nk, 5000 + i, 0.3 + 0.05 * (i % 7)) for i in range(distinct)]
    tile = lambda i, n: np.stack([pairs[j % distinct][i] for j in range(n)])      # noqa: E731
    km = ea.KeypointMap(n_k=nk, dim=D, global_dim=8)
    poses = np.tile(np.eye(4), (M, 1, 1))
    km.add({"global": torch.zeros(M, 8), "keypoints": torch.from_numpy(tile(3, M)), "descriptors": torch.from_numpy(tile(1, M))},
           poses)
    rng = np.random.default_rng(0)
    rows = []
    p = lambda t: t.data_ptr()                                                 # noqa: E731
    for Q in args.points:
        P = Q * k
        qf, qk = torch.from_numpy(tile(0, Q)).cuda(), torch.from_numpy(tile(2, Q)).cuda()
        qn = torch.full((Q,), nk, dtype=torch.int32, device="cuda")
        nn_host = rng.integers(0, M, size=(Q, k)).astype(np.int32)
        nn_host[:, 0] = np.arange(Q) % distinct + distinct * rng.integers(0, M // distinct, Q)     # the true entry at rank 0
        nn = torch.from_numpy(nn_host).cuda()
        corr = torch.empty((P, nk, 2), dtype=torch.int32, device="cuda")
        ncorr, stat = torch.empty(P, dtype=torch.int32, device="cuda"), torch.empty(P, dtype=torch.int32, device="cuda")
        corr2, ncorr2 = torch.empty_like(corr), torch.empty_like(ncorr)
        nb = lib.egonn_match_candidates_scratch_bytes(Q, k, nk)
        assert nb == lib.egonn_match_mutual_scratch_bytes(P, nk)
        scratch, scratch2 = _lib.scratch(nb, "cuda"), _lib.scratch(nb, "cuda")
        bank_f, bank_n = km.descriptors, km.counts
        st = _lib._stream()
        if args.spectral:
            rows.append(_spectral_row(ea, _lib, lib, km, qf, qk, qn, nn, H, {"queries": Q, "k": k, "pairs": P, "n_k": nk, "dim": D,
                                                                            "map_entries": M, "hypotheses": H}))
            print(json.dumps(rows[-1]), flush=True)
            continue
        flat = nn.reshape(-1).long()
        qidx = torch.arange(Q, device="cuda").repeat_interleave(k)

        def indexed():
            _lib.check(lib.egonn_match_candidates(p(qf), p(qn), p(bank_f), p(bank_n), p(nn), Q, k, M, nk, D, p(corr), p(ncorr), p(stat),
                                                  p(scratch), nb, st))

        def gathered():
            f1, f2 = qf[qidx], bank_f[flat]                        # (P, n_k, D) copies of both operands, as a host-side glue does
            n1, n2 = qn[qidx], bank_n[flat]
            _lib.check(lib.egonn_match_mutual(p(f1), p(f2), p(n1), p(n2), P, nk, D, p(corr2), p(ncorr2), p(scratch2), nb, st))

        reps, burst = (7, 2) if P >= 1024 else (10, 40)
        row = {"queries": Q, "k": k, "pairs": P, "n_k": nk, "dim": D, "map_entries": M}
        row["matching_us"] = _time_alternated({"match_candidates": indexed, "gather_plus_match_mutual": gathered}, 3, reps, burst)
        assert torch.equal(corr, corr2) and torch.equal(ncorr, ncorr2), "the two forms must agree bit for bit"
        a, b = row["matching_us"]["match_candidates"], row["matching_us"]["gather_plus_match_mutual"]
        row["matching_speedup_median"] = b["median"] / a["median"]
        row["matching_ranges_overlap"] = not (a["max"] < b["min"] or b["max"] < a["min"])
        keep = {}

        def verify():
            keep["r"] = ea.verify_candidates(qf, qk, qn, km, nn, ransac_max_it=H)

        def verify_reused():
            ea.verify_candidates(qf, qk, qn, km, nn, ransac_max_it=H, out=keep["r"])

        verify()
        reps, burst = (5, 2) if P >= 1024 else (8, 10)
        row["verify_candidates_us"] = _time_alternated({"default": verify, "buffers_reused": verify_reused}, 2, reps, burst)
        r = keep["r"]
        row["verified_share"] = float((r["best_index"] >= 0).float().mean())
        row["hypotheses"] = H
        rows.append(row)
        print(json.dumps(row), flush=True)

    if args.spectral:
        out = json.load(open(args.out)) if os.path.exists(args.out) else {}
        for row in rows:
            row.update(device=torch.cuda.get_device_name(0), commit=args.commit)
        out.setdefault("spectral_rows", []).extend(rows)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        return

    loc = []
    if not args.skip_localize:
        mp = ea.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.1)
        model = ea.model_factory(mp)
        sd = seeded_state_dict(7, {n: tuple(v.shape) for n, v in model.state_dict().items()})
        model.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
        model = model.to("cuda:0").eval()
        ex = ea.DescriptorExtractor(model, n_k=nk)
        scans = [torch.from_numpy(lidar_scan(100 + i, n_points=args.scan_points)) for i in range(args.map_scans)]
        kmap = ea.KeypointMap(n_k=nk, dim=model.local_descriptor_size, global_dim=model.global_descriptor_size)
        for lo in range(0, len(scans), 16):
            kmap.add(ex.extract(scans[lo:lo + 16]), np.tile(np.eye(4), (len(scans[lo:lo + 16]), 1, 1)))
        reloc = ea.Relocalizer(ex, kmap, k=min(k, len(scans)), ransac_max_it=H)
        for B in (1, 16):
            batch = [s.cuda() for s in scans[:B]]
            res = {}

            def localize():
                res["r"] = reloc.localize(batch)

            def extract_only():
                ex.extract(batch)

            t = _time_alternated({"localize": localize, "extract_only": extract_only}, 2, 6, 2)
            loc.append({"batch": B, "scan_points": args.scan_points, "map_scans": len(scans), "k": reloc.k, "hypotheses": H,
                        "us": t, "self_retrieved": bool((res["r"]["best_index"].cpu() == torch.arange(B)).all())})
            print(json.dumps(loc[-1]), flush=True)

    out = {"device": torch.cuda.get_device_name(0), "commit": args.commit,
           "workload": "planted keypoint pairs (30-60 % outliers, D = 128) tiled into a map; the true entry at rank 0, random "
                       "entries behind it; localize: seeded weights on synthetic scans",
           "timer": "device events around a window of back-to-back calls, per-call time = window / calls; median over the "
                    "windows after warm-up; compared forms alternated window by window in one run",
           "rows": rows, "localize": loc}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
