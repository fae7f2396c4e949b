"""Digests of what the scan registration entry points return on the committed small cases, for comparing two builds of the
library bit for bit (a refactor of csrc/icp.hip, csrc/ndt.hip or csrc/pair_loop.h must not change one).  Only the public Python
API is used, so the same file runs against an older checkout's library.  Entry points, all with their debug outputs on:
  voxel_downsample         the raw clouds of every ICP_CASES entry of tests/test_icp_host.py except scan_50k, one batch; cropped
  estimate_normals         their downsampled targets, knn 20 and 32
  icp_pairs                the cases as one batch from their T_init, and every case alone
  icp_plane_pairs          the same with the knn-20 normals
  NDTMap.register          the planted scans of tests/ndt_ref.py, each against the map of the other five from its "GPS" pose, and
                           one batch with an empty scan in it; neighbors 1 and 7
One line `DIGEST <entry point> <sha256>` per entry point over the raw bytes of every output tensor, in a fixed order.

    python tools/check_bitwise_registration.py > a.txt          # in each checkout
    python tools/check_bitwise_registration.py --compare a.txt b.txt
"""
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _digests(path):
    return {l.split()[1]: l.split()[2] for l in open(path) if l.startswith("DIGEST ")}


def compare(a, b):
    da, db = _digests(a), _digests(b)
    ok = bool(da) and sorted(da) == sorted(db)
    for k in sorted(set(da) | set(db)):
        same = da.get(k) == db.get(k)
        ok &= same
        print("equal    " if same else "DIFFERENT", k, da.get(k), db.get(k))
    print("every line equal:", ok)
    return 0 if ok else 1


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
    for entry in hashes:
        print("DIGEST", entry, hashes[entry].hexdigest(), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(compare(sys.argv[2], sys.argv[3]) if len(sys.argv) == 4 and sys.argv[1] == "--compare" else main())
