"""Digests of what the scan registration entry points return on the committed small cases, for comparing two builds of the
library bit for bit (a refactor of csrc/icp.hip, csrc/ndt.hip or csrc/pair_loop.h must not change one).  Only the public Python
API is used, so the same file runs against an older checkout's library.  Entry points, all with their debug outputs on:
  voxel_downsample         the raw clouds of every ICP_CASES entry of tests/test_icp_host.py except scan_50k, one batch; cropped
  estimate_normals         their downsampled targets, knn 20 and 32
  icp_pairs                the cases as one batch from their T_init, and every case alone
  icp_plane_pairs          the same with the knn-20 normals
  NDTMap.register          the planted scans of tests/ndt_ref.py, each against the map of the other five from its "GPS" pose, and
                           one batch with an empty scan in it; neighbors 1 and 7
and what the files that carve a caller's scratch span or compact rows return (csrc/common.h: Carve, csrc/compact.h), each on the
small inputs that its GPU test builds:
  voxel_map_*              VoxelMap.insert eager and reserved (in two batches), points, submaps; the scene of tests/voxel_map_ref.py
  ndt_accumulate/finalize  NDTMap over that map
  cloud_bank_gather        CloudBank.gather of that scene's clouds
  pr_curve                 evaluate_loop_closure on the 257- and 4097-scan trajectories of tests/test_gpu_loop_closure.py
  pose_graph_optimize      the 129-pose trajectory of tests/test_gpu_pose_graph.py, with a fixed mask
  loop_consistency         filter_loops on the mixed planted loops of tests/test_gpu_loop_consistency.py
  local_loss               local_loss_packed, loss, statistics and the six gradients, on the edge batches of tests/local_loss_ref.py
  augment_points           a batch of tests/augment_ref.py under both modes
One line `DIGEST <entry point> <sha256>` per entry point over the raw bytes of every output tensor, in a fixed order.  With
--scratch, on any machine: one line `SCRATCH <function> <shape> <bytes>` per *_scratch_bytes function and shape of a fixed table.

    python tools/check_bitwise_registration.py > a.txt          # in each checkout
    python tools/check_bitwise_registration.py --scratch >> a.txt
    python tools/check_bitwise_registration.py --compare a.txt b.txt
"""
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


# --scratch: every egonn_*_scratch_bytes of the files that carve a caller's span, over a fixed table of shapes.  One argument
# moves at a time over its values (zero, one, one short of a multiple of 256, a multiple, one over, one large), the others rest
# at the first value of `base`; then every argument at its large value.  No device is needed.
_SIZES = (0, 1, 255, 256, 257, 1000003)
_COUNTS = (0, 1, 255, 256, 257, 4096)
_SCRATCH = [       # function, the values of every argument, the resting values
    ("voxel_map_integrate", (_SIZES, _COUNTS), (1000, 3)),
    ("voxel_map_merge", (_SIZES, _SIZES, _SIZES + (2000006,)), (1000, 1000, 2000006)),
    ("voxel_map_select", (_SIZES + (4097,), _COUNTS), (1000, 3)),
    ("voxel_downsample", (_SIZES, _COUNTS), (1000, 3)),
    ("icp", (_SIZES, _SIZES, _COUNTS), (1000, 900, 3)),
    ("icp_plane", (_SIZES, _SIZES, _COUNTS), (1000, 900, 3)),
    ("estimate_normals", (_SIZES, _COUNTS), (1000, 3)),
    ("ndt_accumulate", (_SIZES, _COUNTS), (1000, 3)),
    ("ndt_register", (_SIZES, _COUNTS), (1000, 3)),
    ("knn_window", (_SIZES, (0, 1, 25, 64)), (1000, 25)),
    ("pr_curve", (_SIZES,), (1000,)),
    ("loop_consistency", (_SIZES, (0, 63, 64, 128, 256, 320, 65536)), (1000, 64)),
    ("pose_graph", (_SIZES, _SIZES, (0, 1, 16)), (1000, 1500, 16)),
    ("local_loss", (_COUNTS, _SIZES, _SIZES, (128,)), (3, 1000, 900, 128)),
    ("augment", (_SIZES, _COUNTS), (1000, 3)),
]


def scratch_table():
    from egonn_amd import _lib
    lib = _lib.load()
    for name, values, base in _SCRATCH:
        fn = getattr(lib, f"egonn_{name}_scratch_bytes")
        shapes = [base] + [base[:a] + (v,) + base[a + 1:] for a in range(len(base)) for v in values[a]] + [tuple(v[-1] for v in values)]
        for shape in dict.fromkeys(shapes):
            print("SCRATCH", name, "x".join(str(v) for v in shape), fn(*shape), flush=True)
    return 0


def _digests(path):
    """the DIGEST and SCRATCH lines of a file: name (and shape) -> value"""
    out = {}
    for l in open(path):
        w = l.split()
        if w and w[0] == "DIGEST":
            out[w[1]] = w[2]
        elif w and w[0] == "SCRATCH":
            out[f"scratch_bytes {w[1]} {w[2]}"] = w[3]
    return out


def compare(a, b):
    da, db = _digests(a), _digests(b)
    ok = bool(da) and sorted(da) == sorted(db)
    for k in sorted(set(da) | set(db)):
        same = da.get(k) == db.get(k)
        ok &= same
        print("equal    " if same else "DIFFERENT", k, da.get(k), db.get(k))
    print("every line equal:", ok)
    return 0 if ok else 1


def span_users(add, cu, ea):
    """the entry points that carve a caller's span or compact rows, beyond the registration: see the module docstring"""
    import numpy as np
    import torch
    from tests import augment_ref, helpers, local_loss_ref, voxel_map_ref
    from tests.test_gpu_local_loss_batch import GAMMA_ORDER, PACK_ORDER
    from tests.test_gpu_loop_closure import _trajectory_case
    from tests.test_gpu_loop_consistency import KW, _mixed
    from tests.test_gpu_pose_graph import _trajectory
    from tests.test_gpu_voxel_map import ORIGIN, VOXEL

    bank_np, off, poses = voxel_map_ref.random_scene()
    bank = ea.CloudBank()
    bank.points = cu(bank_np)
    bank.host_offsets = [int(v) for v in off]
    pick = np.array([0, 1, 2, 3, 4, 5, 6, 2, 0])
    records = lambda vm: {f: vm.records[f][:vm.n_voxels] for f in ("keys", "sums", "count", "obs")}       # noqa: E731
    vm = ea.VoxelMap(VOXEL, ORIGIN).insert(bank, poses[pick], pick)
    add("voxel_map_insert_eager", records(vm))
    held = ea.VoxelMap(VOXEL, ORIGIN, capacity=vm.n_voxels + 9)
    for part in np.array_split(np.arange(len(pick)), 2):
        held.insert(bank, poses[pick[part]], pick[part])
    add("voxel_map_insert_reserved", records(held))
    for mc, mo in ((1, 1), (2, 1), (1, 2)):
        add("voxel_map_points", vm.points(mc, mo))
    centers = np.array([[0.0, 0.0, 0.0], [1.5, 0.5, 0.0], [900.0, 0.0, 0.0], [-3.0, 2.0, 1.0]])
    for half in (3.0, (2.0, 4.0, 1.0)):
        for relative in (True, False):
            add("voxel_map_submaps", held.submaps(centers, half, min_count=2, relative=relative))
    ndt = ea.NDTMap(vm).accumulate(bank, poses[pick], pick)
    add("ndt_accumulate", {"cnt": ndt.cnt, "s1": ndt.s1, "s2": ndt.s2})
    add("ndt_finalize", ndt.finalize(debug=True))
    add("cloud_bank_gather", bank.gather([3, 0, 6, 3]))

    for n in (257, 4097):
        pos64, _, lo, hi, nn, score = _trajectory_case(n, 40 + n)
        res = ea.evaluate_loop_closure(cu(nn), cu(score), pos64, cu(lo), cu(hi), 1.25)
        add("pr_curve", {k: v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v)) for k, v in res.items()})

    _, X0, edges, Z, w = _trajectory(n=129, seed=12)
    mask = np.zeros(len(X0), np.int32)
    mask[[0, 50]] = 7
    add("pose_graph_optimize", ea.optimize_pose_graph(cu(X0), cu(edges.astype(np.int64)), cu(Z), cu(w.astype(np.float32)), cu(mask),
                                                      max_iterations=3, pcg_iterations=40))

    _, X0, ei, Z, w, _ = _mixed()
    add("loop_consistency", ea.filter_loops(cu(X0), {"edge_index": cu(ei), "Z": cu(Z), "weights": cu(w)}, min_support=2, **KW))

    from egonn_amd import local_loss as L
    for name, (pairs, _) in sorted(local_loss_ref.edge_batches(helpers.kernel_constant("LL_CLOUD_CHUNK")).items()):
        t = {k: torch.from_numpy(v).cuda() for k, v in local_loss_ref.pack(pairs).items()}
        for k in local_loss_ref.GRAD_KEYS:
            t[k].requires_grad_(True)
        loss, stats, ps = L.local_loss_packed(*[t[k] for k in PACK_ORDER], [local_loss_ref.GAMMAS[k] for k in GAMMA_ORDER],
                                              return_pair_stats=True)
        loss.backward()
        add("local_loss", {"loss": loss.detach(), "stats": stats.detach(), "pair_stats": ps.detach(),
                           **{"grad_" + k: t[k].grad for k in local_loss_ref.GRAD_KEYS}})

    from egonn_amd import augment as aug
    sizes = [3000, 1, 257, 5000]
    pts, aoff = augment_ref.batch(8, sizes)
    for stages in (augment_ref.MODE1 | augment_ref.SET1, augment_ref.MODE2 | augment_ref.SET1):
        P = augment_ref.Params(seed=4, draw=5, set_id=1, stages=stages, block_p=1.0)
        params = aug.AugmentParams(seed=P.seed, stages=P.stages, sigma=P.sigma, clip=P.clip if P.stages & augment_ref.JITTER_CLIP else None,
                                   r_min=P.r_min, r_max=P.r_max, max_delta=P.max_delta, max_theta=P.max_theta, block_p=P.block_p,
                                   scale=P.scale, ratio=P.ratio, set_max_theta=P.set_max_theta, flip_p=P.flip_p, rot_max=P.rot_max,
                                   trans_max=P.trans_max)
        r = aug.augment_points(cu(np.asarray(pts, np.float32)), cu(np.asarray(aoff, np.int64)), cu(np.arange(len(sizes), dtype=np.int32)),
                               params, draw=P.draw, set_id=P.set_id, record=True, flags=True)
        add("augment_points", {k: v for k, v in vars(r).items() if torch.is_tensor(v)})


def main():
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "the digests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd as ea
    from tests import ndt_ref
    from tests.test_icp_host import ICP_CASES, icp_case

    hashes = {}

    def add(entry, out, rows=None):
        """every tensor of a result dict, by key; rows: the valid rows of a downsample's points and counts"""
        torch.cuda.synchronize()
        h = hashes.setdefault(entry, hashlib.sha256())
        for k in sorted(out):
            if k.startswith("_") or not torch.is_tensor(out[k]):
                continue
            t = out[k][:rows] if rows is not None and k in ("points", "counts") else out[k]
            h.update(k.encode())
            h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())

    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731

    def offsets(clouds):
        off = np.zeros(len(clouds) + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in clouds])
        return off

    cat = lambda clouds, dt: np.concatenate([np.asarray(c, dt).reshape(-1, 3) for c in clouds])      # noqa: E731
    cases = [icp_case(n) for n in ICP_CASES if n != "scan_50k"]

    raws = [c[k] for c in cases for k in ("raw_src", "raw_tgt")]
    for crop in (None, (-80.0, 80.0, -80.0, 80.0, -0.9, None)):
        d = ea.voxel_downsample(cu(cat(raws, np.float32)), cu(offsets(raws)), 0.1, crop)
        add("voxel_downsample", d, int(d["offsets"][-1]))

    srcs, tgts, T0 = [c["src"] for c in cases], [c["tgt"] for c in cases], np.stack([c["T_init"] for c in cases])
    nrm = {}
    for knn in (20, 32):
        nrm[knn] = ea.estimate_normals(cu(cat(tgts, np.float64)), cu(offsets(tgts)), knn, True)
        add("estimate_normals", nrm[knn])
    normals = nrm[20]["normals"].cpu().numpy()
    to = offsets(tgts)
    for entry, plane in (("icp_pairs", False), ("icp_plane_pairs", True)):
        for sel in [list(range(len(cases)))] + [[i] for i in range(len(cases))]:
            s, t = [srcs[i] for i in sel], [tgts[i] for i in sel]
            n = cu(np.concatenate([normals[to[i]:to[i + 1]] for i in sel])) if plane else None
            add(entry, ea.icp_pairs(cu(cat(s, np.float64)), cu(offsets(s)), cu(cat(t, np.float64)), cu(offsets(t)), cu(T0[sel]), 1.2, 200,
                                    True, n))

    c = ndt_ref.planted_case()
    bank = ea.CloudBank()
    bank.points = cu(c["bank"])
    bank.host_offsets = [int(v) for v in c["off"]]
    maps = []
    for k in range(6):
        others = [j for j in range(6) if j != k]
        vm = ea.VoxelMap(1.0, origin=c["origin"]).insert(bank, c["planted"][others], others)
        m = ea.NDTMap(vm).accumulate(bank, c["planted"][others], others)
        m.finalize()
        maps.append(m)
    for nb in (1, 7):
        for k in range(6):
            add(f"ndt_register_neighbors_{nb}", maps[k].register(cu(c["clouds"][k]), cu(offsets([c["clouds"][k]])), cu(c["gps"][k:k + 1]), nb,
                                                                debug=True))
        batch = [c["clouds"][0], c["clouds"][0][:0], c["clouds"][0][100:357], c["clouds"][1]]
        add(f"ndt_register_neighbors_{nb}", maps[0].register(cu(cat(batch, np.float64)), cu(offsets(batch)), cu(c["gps"][[0, 0, 0, 1]]), nb,
                                                            debug=True))
    span_users(add, cu, ea)
    for entry in hashes:
        print("DIGEST", entry, hashes[entry].hexdigest(), flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(scratch_table() if sys.argv[1:] == ["--scratch"] else main())
