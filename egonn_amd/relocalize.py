"""Relocalisation: place query scans in the frame of a map of scans with known poses.

The global descriptor retrieves the top-k map entries (`retrieval.knn`), every (query, candidate) pair is registered from
its keypoints (mutual matching, RANSAC, final evaluation: csrc/relocalize.hip + csrc/registration.hip) and the candidate
with the most inliers gives the pose: P_query = P_map[best] @ T, T = the registration's transform, which maps query
keypoints into the candidate's frame (the reference's T_gt = inv(P_map) @ P_query, misc/poses.py).  Verifying the top k
instead of trusting rank 0 is what turns recall@k into recall@1.

`KeypointMap` holds the map resident on the device, `verify_candidates` is the sync-free call sequence
egonn_match_candidates -> egonn_gather_candidates -> egonn_ransac_pairs -> egonn_registration_finish ->
egonn_pick_candidates (with method="spectral": egonn_spectral_verify, csrc/spectral.hip, in place of the two RANSAC
calls), `Relocalizer` is the product call from raw scans and `evaluate_relocalization` its metrics.
All arithmetic runs in libegonn_hip; there is no torch or numpy fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib, registration as _reg, retrieval as _ret
from ._lib import as_dev as _dev
from .tuples import CloudBank, relative_poses

RELOC_NO_CANDIDATE, RELOC_BAD_INDEX, RELOC_UNVERIFIED = 1, 2, 4
MAX_PAIRS = _reg.MAX_PAIRS     # pairs per call sequence of verify_candidates


class KeypointMap:
    """The map side of relocalisation, resident on one device: globals (M, G) f32, keypoints (M, n_k, 3) f32, descriptors
    (M, n_k, D) f32, counts (M,) int32, poses (M,4,4) f64; `clouds`: an optional `CloudBank` with the same M scans, for the
    ICP refinement.  `add` appends a batch; the buffers grow geometrically (by half at least), so an entry is copied O(1) times."""

    def __init__(self, n_k: int = 128, dim: int = 128, global_dim: int = 256, device=None):
        if not 1 <= int(n_k) <= _reg.N_MAX:
            raise ValueError(f"KeypointMap: n_k must be in [1, {_reg.N_MAX}], got {n_k}")
        if int(dim) < 4 or int(dim) > 256 or int(dim) % 4:
            raise ValueError(f"KeypointMap: dim must be a multiple of 4 in [4, 256], got {dim}")
        self.n_k, self.dim, self.global_dim = int(n_k), int(dim), int(global_dim)
        if device is None:
            device = _lib.require_gpu()
        self.device = torch.device(device)
        self.clouds: Optional[CloudBank] = None
        self._n = 0
        self._buf: Dict[str, torch.Tensor] = {}
        self._alloc(0)

    _SPEC = (("globals", torch.float32), ("keypoints", torch.float32), ("descriptors", torch.float32), ("counts", torch.int32),
             ("poses", torch.float64))

    def _shape(self, name, rows):
        return {"globals": (rows, self.global_dim), "keypoints": (rows, self.n_k, 3), "descriptors": (rows, self.n_k, self.dim),
                "counts": (rows,), "poses": (rows, 4, 4)}[name]

    def _alloc(self, cap: int):
        for name, dt in self._SPEC:
            new = torch.zeros(self._shape(name, cap), dtype=dt, device=self.device)
            if self._n:
                new[: self._n] = self._buf[name][: self._n]
            self._buf[name] = new

    def __len__(self):
        return self._n

    globals = property(lambda self: self._buf["globals"][: self._n])
    keypoints = property(lambda self: self._buf["keypoints"][: self._n])
    descriptors = property(lambda self: self._buf["descriptors"][: self._n])
    counts = property(lambda self: self._buf["counts"][: self._n])
    poses = property(lambda self: self._buf["poses"][: self._n])

    def add(self, out: Dict[str, torch.Tensor], poses) -> "KeypointMap":
        """out: the dict of DescriptorExtractor.extract*, StreamingExtractor.run or build_database_streaming(keep_local=True)
        ('global' (b, G), 'keypoints' (b, n_k, 3), 'descriptors' (b, n_k, D), 'count' (b,), absent = every row valid);
        poses (b,4,4).  Tensors on any device."""
        g = torch.as_tensor(out["global"])
        b = g.shape[0]
        kp, desc = torch.as_tensor(out["keypoints"]), torch.as_tensor(out["descriptors"])
        ps = torch.as_tensor(np.asarray(poses, dtype=np.float64) if not torch.is_tensor(poses) else poses)
        if tuple(g.shape) != (b, self.global_dim) or tuple(kp.shape) != (b, self.n_k, 3) or \
                tuple(desc.shape) != (b, self.n_k, self.dim) or tuple(ps.shape) != (b, 4, 4):
            raise ValueError(f"KeypointMap.add: expected global ({b}, {self.global_dim}), keypoints ({b}, {self.n_k}, 3), "
                             f"descriptors ({b}, {self.n_k}, {self.dim}), poses ({b}, 4, 4); got {tuple(g.shape)}, "
                             f"{tuple(kp.shape)}, {tuple(desc.shape)}, {tuple(ps.shape)}")
        cnt = out.get("count")
        cnt = torch.full((b,), self.n_k, dtype=torch.int32) if cnt is None else torch.as_tensor(cnt)
        if tuple(cnt.shape) != (b,):
            raise ValueError(f"KeypointMap.add: count must have shape ({b},), got {tuple(cnt.shape)}")
        need, have = self._n + b, self._buf["counts"].shape[0]
        if need > have:
            self._alloc(max(need, have + have // 2))
        for name, src in (("globals", g), ("keypoints", kp), ("descriptors", desc), ("counts", cnt), ("poses", ps)):
            buf = self._buf[name]
            buf[self._n: need] = src.to(device=self.device, dtype=buf.dtype)
        self._n = need
        return self

    def to(self, device) -> "KeypointMap":
        """the map on another device (a copy; `clouds` is shared)"""
        m = KeypointMap(self.n_k, self.dim, self.global_dim, device)
        if self._n:
            m.add({"global": self.globals, "keypoints": self.keypoints, "descriptors": self.descriptors, "count": self.counts},
                  self.poses)
        m.clouds = self.clouds
        return m

    def save(self, path: str) -> None:
        """everything into one .npz (the attached CloudBank included)"""
        a = {name: getattr(self, name).cpu().numpy() for name, _ in self._SPEC}
        a["shape"] = np.array([self.n_k, self.dim, self.global_dim], dtype=np.int64)
        if self.clouds is not None:
            c = self.clouds
            a["cloud_points"] = (c.points[: c.n_points].cpu().numpy() if c.n_points else np.zeros((0, 3), np.float64))
            a["cloud_offsets"] = np.asarray(c.host_offsets, dtype=np.int64)
            a["cloud_status"] = np.asarray(c.status, dtype=np.int32)
            a["cloud_voxel"] = np.array([c.voxel_size], dtype=np.float64)
            a["cloud_crop"] = np.array([np.nan] * 6 if c.crop is None else [np.nan if v is None else float(v) for v in c.crop])
        with open(path, "wb") as f:
            np.savez(f, **a)

    @classmethod
    def load(cls, path: str, device=None) -> "KeypointMap":
        with np.load(path) as z:
            n_k, dim, gdim = (int(v) for v in z["shape"])
            m = cls(n_k, dim, gdim, device)
            if len(z["counts"]):
                m.add({"global": torch.from_numpy(z["globals"]), "keypoints": torch.from_numpy(z["keypoints"]),
                       "descriptors": torch.from_numpy(z["descriptors"]), "count": torch.from_numpy(z["counts"])},
                      torch.from_numpy(z["poses"]))
            if "cloud_offsets" in z.files:
                crop = z["cloud_crop"]
                crop = None if np.isnan(crop).all() else tuple(None if np.isnan(v) else float(v) for v in crop)
                c = CloudBank(crop=crop, voxel_size=float(z["cloud_voxel"][0]), device=m.device)
                c.points = torch.from_numpy(z["cloud_points"]).to(m.device)
                c.host_offsets = [int(v) for v in z["cloud_offsets"]]
                c.status = [int(v) for v in z["cloud_status"]]
                m.clouds = c
        return m


_NOT_KEPT = ("correspondence_set", "repeatability")     # per-pair outputs of `registration.PAIR_OUTPUTS` not computed per candidate


def pair_keys(method):
    """{name in `registration.PAIR_OUTPUTS`: per-pair key of `verify_candidates`}: `status` is the per-query word here"""
    return {r[0]: "pair_status" if r[0] == "status" else r[0] for r in _reg.pair_outputs(method, skip=_NOT_KEPT)}


def _verify_buffers(dev, Q, k, n_max, Pc, with_gt, nb_match, nb_reg, method="ransac"):
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)          # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)            # noqa: E731
    keys, own = pair_keys(method), _reg.pair_buffers(dev, (Q, k), n_max, with_gt, method, skip=_NOT_KEPT)
    out = {**{keys[n]: t for n, t in own.items()}, "match_status": i32(Q, k), "corr": i32(Q, k, n_max, 2), "n_corr": i32(Q, k),
           "pair_ids": i32(Q, k), "best_rank": i32(Q), "best_index": i32(Q), "reranked": i32(Q, k), "T_rel": f64(Q, 4, 4),
           "pose": f64(Q, 4, 4), "safe_pick": i32(Q), "best_inliers": i32(Q), "status": i32(Q)}
    if with_gt:
        out.update({"best_rte": f64(Q), "best_rre": f64(Q), "best_success": i32(Q)})
    out["_work"] = {"kp1": torch.empty((Pc, n_max, 3), dtype=torch.float32, device=dev),
                    "kp2": torch.empty((Pc, n_max, 3), dtype=torch.float32, device=dev), "n1": i32(Pc), "n2": i32(Pc),
                    "match": _lib.scratch(nb_match, dev), "reg": _lib.scratch(nb_reg, dev)}
    return out


def verify_candidates(q_desc, q_kp, q_count, kmap: KeypointMap, nn_index, query_ids=None, T_gt=None, min_inliers: int = 0,
                      ransac_dist_th: float = 0.5, ransac_max_it: int = 10000, seed: int = 0, chunk_pairs: int = MAX_PAIRS,
                      out: Optional[Dict[str, torch.Tensor]] = None, method: str = "ransac", d_thr: float = _reg.SPECTRAL_D_THR,
                      iterations: int = _reg.SPECTRAL_ITERATIONS,
                      seed_ratio: float = _reg.SPECTRAL_SEED_RATIO) -> Dict[str, torch.Tensor]:
    """Register Q queries against k map entries each and pick the best candidate per query.

    q_desc (Q, n_k, D), q_kp (Q, n_k, 3), q_count (Q,) or None (= n_k): what the extractors return; nn_index (Q, k) int32 map
    entries (-1 = none, as `retrieval.knn` pads); query_ids (Q,) int32 or None (= position): the pair id of the RANSAC draws
    is (query_ids[q] * 1000003 + map index) mod 2^30, so a pair's result does not depend on the candidate's rank nor on the
    batch; T_gt (Q, k, 4, 4) or None: the true relative pose per pair, for rte / rre / success.

    Returns device tensors.  Per pair, (Q, k, ...): T (4,4) f64, inliers, fitness, inlier_rmse, best_t, pair_status
    (EGONN_REG_STATUS_* bits), match_status (RELOC_NO_CANDIDATE / RELOC_BAD_INDEX), corr (n_k, 2), n_corr, pair_ids, with T_gt
    also rte, rre, success.  Per query, (Q, ...): best_rank, best_index (-1 = unverified), reranked (k) map indices by most
    inliers, then lowest inlier_rmse, then lowest rank (invalid ones last, as -1), T_rel, pose = map pose @ T_rel (identity
    when unverified), safe_pick (best_index, or the clamped first candidate: a pick `CloudBank.gather` accepts),
    best_inliers, status (OR of the RELOC_* bits), with T_gt also best_rte, best_rre (-1 when unverified), best_success.

    min_inliers = 0 means: the best candidate with a model wins.  No threshold for real data can be derived here (there are
    neither trained weights nor a dataset in this project); pick one from the inlier counts of wrong candidates on your data.

    method="spectral": egonn_spectral_verify (`registration.spectral_verify`: d_thr, iterations, seed_ratio; ransac_dist_th
    is its dist_th) takes the place of the two RANSAC calls.  The pick order is the same; per pair eigenvalue, score (Q, k),
    weights (Q, k, n_k) and n_seeds replace best_t; ransac_max_it and seed are ignored and pair_ids enter nothing.

    No host synchronisation when the inputs are device tensors.  Queries are chunked so that a call sequence covers at most
    `chunk_pairs` (<= 4096) pairs.  `out`: the dict of an earlier call with the same shapes and method; its buffers (scratch
    included) are used again and nothing is allocated, which a graph capture through egonn_graph_begin / egonn_graph_end needs."""
    spectral = _reg.check_method("verify_candidates", method) == "spectral"
    dev = q_desc.device if torch.is_tensor(q_desc) and q_desc.is_cuda else _lib.require_gpu()
    lib = _lib.load()
    qf = _dev(q_desc, dev, torch.float32)
    if qf.dim() != 3:
        raise ValueError(f"verify_candidates: q_desc must be (Q, n_k, D), got {tuple(qf.shape)}")
    Q, n_max, D = qf.shape
    if (n_max, D) != (kmap.n_k, kmap.dim):
        raise ValueError(f"verify_candidates: queries are ({n_max}, {D}) per scan, the map holds ({kmap.n_k}, {kmap.dim})")
    if kmap.device != dev:
        raise ValueError(f"verify_candidates: the map lives on {kmap.device}, the queries on {dev}")
    M = len(kmap)
    if M < 1:
        raise ValueError("verify_candidates: the map is empty")
    qk = _dev(q_kp, dev, torch.float32)
    if tuple(qk.shape) != (Q, n_max, 3):
        raise ValueError(f"verify_candidates: q_kp must be ({Q}, {n_max}, 3), got {tuple(qk.shape)}")
    qn = torch.full((Q,), n_max, dtype=torch.int32, device=dev) if q_count is None else _dev(q_count, dev, torch.int32)
    nn = _dev(nn_index, dev, torch.int32)
    if nn.dim() != 2 or nn.shape[0] != Q or nn.shape[1] < 1 or qn.shape != (Q,):
        raise ValueError(f"verify_candidates: nn_index must be ({Q}, k >= 1) and q_count ({Q},), got {tuple(nn.shape)}, "
                         f"{tuple(qn.shape)}")
    k = nn.shape[1]
    qid = None if query_ids is None else _dev(query_ids, dev, torch.int32)
    if qid is not None and qid.shape != (Q,):
        raise ValueError(f"verify_candidates: query_ids must have shape ({Q},)")
    gt = None if T_gt is None else _dev(T_gt, dev, torch.float64)
    if gt is not None and tuple(gt.shape) != (Q, k, 4, 4):
        raise ValueError(f"verify_candidates: T_gt must be ({Q}, {k}, 4, 4), got {tuple(gt.shape)}")
    chunk_pairs = max(1, min(int(chunk_pairs), MAX_PAIRS))
    qc = max(1, min(max(Q, 1), chunk_pairs // k))                 # queries per call sequence
    if qid is None and Q > qc:       # query_ids = None means the position in the whole call, not in its chunk
        qid = torch.arange(Q, dtype=torch.int32, device=dev)
    H = int(ransac_max_it)
    nb_match = int(lib.egonn_match_candidates_scratch_bytes(qc, k, n_max))     # -1 on bad arguments: the calls below raise
    nb_reg = int(lib.egonn_spectral_verify_scratch_bytes(qc * k, n_max) if spectral else
                 lib.egonn_registration_scratch_bytes(qc * k, n_max, H))
    if out is None:
        out = _verify_buffers(dev, Q, k, n_max, qc * k, gt is not None, nb_match, nb_reg, method)
    else:
        w = out.get("_work", {})
        if ("eigenvalue" in out) != spectral:
            raise ValueError(f"verify_candidates: `out` was made by a call with the other method, not {method!r}")
        if tuple(out["corr"].shape) != (Q, k, n_max, 2) or ("rte" in out) != (gt is not None) or out["T"].device != dev or \
                w["kp1"].shape[0] != qc * k or w["match"].numel() * 8 < nb_match or w["reg"].numel() * 8 < nb_reg:
            raise ValueError("verify_candidates: `out` was made by a call with other shapes")
    w = out["_work"]
    km = (kmap.descriptors, kmap.keypoints, kmap.counts, kmap.poses)
    for lo in range(0, Q, qc):
        hi = min(Q, lo + qc)
        n, P = hi - lo, (hi - lo) * k
        s = lambda name: _lib._ptr(out[name][lo:hi]) if name in out else None        # noqa: E731
        _lib.call(dev, lib.egonn_match_candidates, qf[lo:hi].data_ptr(), qn[lo:hi].data_ptr(), km[0].data_ptr(), km[2].data_ptr(),
                  nn[lo:hi].data_ptr(), n, k, M, n_max, D, s("corr"), s("n_corr"), s("match_status"), w["match"].data_ptr(),
                  w["match"].numel() * 8)
        _lib.call(dev, lib.egonn_gather_candidates, qk[lo:hi].data_ptr(), qn[lo:hi].data_ptr(), km[1].data_ptr(), km[2].data_ptr(),
                  nn[lo:hi].data_ptr(), None if qid is None else qid[lo:hi].data_ptr(), n, k, M, n_max, w["kp1"].data_ptr(),
                  w["kp2"].data_ptr(), w["n1"].data_ptr(), w["n2"].data_ptr(), s("pair_ids"))
        operands = (w["kp1"].data_ptr(), w["kp2"].data_ptr(), w["n1"].data_ptr(), w["n2"].data_ptr(), s("corr"), s("n_corr"))
        pair_out = {name: out[key][lo:hi] for name, key in pair_keys(method).items() if key in out}
        if spectral:
            _reg.enqueue_spectral(dev, operands, P, n_max, d_thr, iterations, seed_ratio, ransac_dist_th, w["reg"],
                                  None if gt is None else gt[lo:hi], 0.5, pair_out)
        else:
            _reg.enqueue_ransac(dev, (*operands, s("pair_ids")), P, n_max, H, seed, ransac_dist_th, w["reg"],
                                None if gt is None else gt[lo:hi], 0.5, pair_out)
        _lib.call(dev, lib.egonn_pick_candidates, nn[lo:hi].data_ptr(), n, k, M, km[3].data_ptr(), s("T"), s("inliers"),
                  s("inlier_rmse"), s("pair_status"), s("rte"), s("rre"), s("success"), int(min_inliers), s("best_rank"),
                  s("best_index"), s("reranked"), s("T_rel"), s("pose"), s("safe_pick"), s("best_inliers"), s("status"),
                  s("best_rte"), s("best_rre"), s("best_success"))
    out["_keep"] = (qf, qk, qn, nn, qid, gt) + km          # inputs of enqueued work stay alive with the result
    return out


def _pose_product(map_poses: torch.Tensor, pick: torch.Tensor, T: torch.Tensor) -> torch.Tensor:
    """map_poses[pick[q]] @ T[q] on the device, by the pose product of egonn_pick_candidates (one candidate per query that
    always wins): the same fixed order of operations as `pose`."""
    dev, Q = T.device, T.shape[0]
    lib = _lib.load()
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)            # noqa: E731
    zero, zf = i32(Q), torch.zeros((Q,), dtype=torch.float64, device=dev)
    pose = torch.empty((Q, 4, 4), dtype=torch.float64, device=dev)
    junk_i, junk_T = torch.empty((6, Q), dtype=torch.int32, device=dev), torch.empty((Q, 4, 4), dtype=torch.float64, device=dev)
    pk, Tc = pick.contiguous(), T.contiguous()
    _lib.call(dev, lib.egonn_pick_candidates, pk.data_ptr(), Q, 1, map_poses.shape[0], map_poses.data_ptr(), Tc.data_ptr(),
              zero.data_ptr(), zf.data_ptr(), zero.data_ptr(), None, None, None, 0, junk_i[0].data_ptr(), junk_i[1].data_ptr(),
              junk_i[2].data_ptr(), junk_T.data_ptr(), pose.data_ptr(), junk_i[3].data_ptr(), junk_i[4].data_ptr(),
              junk_i[5].data_ptr(), None, None, None)
    return pose


class Relocalizer:
    """`localize(scans)`: extract -> `retrieval.knn` on the map's global descriptors -> `verify_candidates` [-> ICP].

    extractor: a `DescriptorExtractor` (or any object whose `extract(scans)` returns its dict); kmap: a `KeypointMap` on the
    extractor's device; k: candidates per query.  refine=True needs `kmap.clouds` and polishes the winner's T_rel by
    point-to-point ICP of the query's downsampled cloud against the winner's cloud of the bank; icp_point2plane=True uses the
    point-to-plane estimator instead, on normals of the gathered winners' clouds.  method, d_thr, iterations, seed_ratio: the
    geometric check of `verify_candidates` ("ransac" or "spectral").  ndt_map: a finalized `NDTMap` in the frame of the map's
    poses; the winner's pose `map_pose[best] @ T_rel` then starts an NDT registration of the query's downsampled cloud against
    it (ndt_neighbors 1 or 7).  `refine` keeps its meaning and the two can be combined."""

    def __init__(self, extractor, kmap: KeypointMap, k: int = 20, min_inliers: int = 0, ransac_dist_th: float = 0.5,
                 ransac_max_it: int = 10000, seed: int = 0, refine: bool = False, icp_dist_th: float = 1.2,
                 icp_max_it: int = 200, chunk_pairs: int = MAX_PAIRS, icp_point2plane: bool = False, method: str = "ransac",
                 d_thr: float = _reg.SPECTRAL_D_THR, iterations: int = _reg.SPECTRAL_ITERATIONS,
                 seed_ratio: float = _reg.SPECTRAL_SEED_RATIO, ndt_map=None, ndt_neighbors: int = 1):
        if int(k) < 1:
            raise ValueError("Relocalizer: k must be positive")
        if int(ndt_neighbors) not in (1, 7):
            raise ValueError("Relocalizer: ndt_neighbors is 1 or 7")
        if ndt_map is not None and getattr(ndt_map, "gaussians", None) is None:
            raise ValueError("Relocalizer: ndt_map must be a finalized NDTMap")
        self.ndt_map, self.ndt_neighbors = ndt_map, int(ndt_neighbors)
        if refine and kmap.clouds is None:
            raise ValueError("Relocalizer: refine=True needs kmap.clouds (a CloudBank of the map's scans)")
        self.extractor, self.kmap, self.k = extractor, kmap, int(k)
        self.min_inliers, self.ransac_dist_th, self.ransac_max_it, self.seed = int(min_inliers), ransac_dist_th, ransac_max_it, seed
        self.refine, self.icp_dist_th, self.icp_max_it, self.chunk_pairs = bool(refine), icp_dist_th, icp_max_it, chunk_pairs
        self.icp_point2plane = bool(icp_point2plane)
        self.method = _reg.check_method("Relocalizer", method)
        self.d_thr, self.iterations, self.seed_ratio = d_thr, iterations, seed_ratio

    def _extract(self, scans):
        """-> (extractor dict, deferred status check or None)"""
        ex = self.extractor
        if not hasattr(ex, "extract_packed"):
            return ex.extract(scans), None
        ctx = ex.model.context()
        pts = [torch.as_tensor(s, dtype=torch.float32).to(ctx.device)[:, :3] for s in scans]
        offsets = [0]
        for p in pts:
            offsets.append(offsets[-1] + p.shape[0])
        allpts = pts[0].contiguous() if len(pts) == 1 else torch.cat(pts, dim=0)
        return ex.extract_packed(allpts, offsets), ctx.plan_status

    def _enqueue(self, y, scans, query_ids, nn_index, query_poses):
        km, dev = self.kmap, self.kmap.device
        if nn_index is None:
            nn, _ = _ret.knn(y["global"], km.globals, self.k)
        else:
            nn = _dev(nn_index, dev, torch.int32)
        Q, k = nn.shape
        gt = None
        if query_poses is not None:      # inv(P_map[candidate]) @ P_query per pair; an invalid candidate gets entry 0's (unused)
            qp = _dev(query_poses, dev, torch.float64).reshape(Q, 4, 4)
            allp = torch.cat([km.poses, qp])
            a = (len(km) + torch.arange(Q, dtype=torch.int32, device=dev)).repeat_interleave(k)
            b = nn.reshape(-1).clamp(0, len(km) - 1)
            gt = relative_poses(allp, a, b, negate_translation=False).reshape(Q, k, 4, 4)
        r = verify_candidates(y["descriptors"], y["keypoints"], y.get("count"), km, nn, query_ids, gt, self.min_inliers,
                              self.ransac_dist_th, self.ransac_max_it, self.seed, self.chunk_pairs, method=self.method,
                              d_thr=self.d_thr, iterations=self.iterations, seed_ratio=self.seed_ratio)
        r["nn_index"], r["global"] = nn, y["global"]
        bank = km.clouds
        if self.refine or self.ndt_map is not None:      # the query's downsampled cloud, by the bank's rule where there is one
            pts = [torch.as_tensor(s, dtype=torch.float32).to(dev)[:, :3] for s in scans]
            off = np.zeros(Q + 1, dtype=np.int64)
            off[1:] = np.cumsum([p.shape[0] for p in pts])
            qd = _reg.voxel_downsample(torch.cat(pts).contiguous(), torch.from_numpy(off).to(dev),
                                       bank.voxel_size if bank is not None else _reg.ICP_VOXEL_SIZE, bank.crop if bank is not None else None)
        if self.ndt_map is not None:                     # the verified winner's pose starts a registration against the NDT map
            ndt = self.ndt_map.register(qd["points"], qd["offsets"], r["pose"], neighbors=self.ndt_neighbors)
            r.update({"pose_ndt": ndt["poses"], "ndt_fitness": ndt["fitness"], "ndt_score": ndt["score"],
                      "ndt_iterations": ndt["iterations"], "ndt_status": ndt["status"], "_ndt": (qd, ndt)})
        if self.refine:
            g = bank.gather(r["safe_pick"], capacity=Q * int(bank.sizes().max()) if len(bank) else 0)
            nrm = _reg.estimate_normals(g["points"], g["offsets"])["normals"] if self.icp_point2plane else None
            icp = _reg.icp_pairs(qd["points"], qd["offsets"], g["points"], g["offsets"], r["T_rel"], self.icp_dist_th,
                                 self.icp_max_it, tgt_normals=nrm)
            r.update({"T_icp": icp["T"], "icp_fitness": icp["fitness"], "icp_inlier_rmse": icp["inlier_rmse"],
                      "icp_status": icp["status"], "pose_refined": _pose_product(km.poses, r["safe_pick"], icp["T"]),
                      "_refine": (qd, g, icp)})
        return r

    @torch.no_grad()
    def localize(self, scans: Sequence, query_ids=None, nn_index=None, query_poses=None) -> Dict[str, torch.Tensor]:
        """scans: list of (n, 3 | 4) float32 point arrays.  Returns the dict of `verify_candidates` plus nn_index (Q, k) and
        global (Q, G); with query_poses (Q,4,4) the per-pair and the winner's rte / rre / success against
        inv(P_map[candidate]) @ P_query.  With refine also T_icp, pose_refined = map pose[best] @ T_icp, icp_fitness,
        icp_inlier_rmse (the per-pair registration already owns `fitness` / `inlier_rmse`) and icp_status, meaningful only
        where best_index >= 0.  With ndt_map also pose_ndt (Q,4,4), ndt_fitness, ndt_score, ndt_iterations and ndt_status (the
        result of `NDTMap.register` started at `pose`), meaningful under the same condition.  nn_index (Q, k): candidates from
        elsewhere instead of the global retrieval.

        Everything is enqueued without host synchronisation; the ONE synchronisation is the extractor's range check at the
        end (a flagged batch is extracted again on the exact kernels and verified again), after which the results are valid."""
        y, check = self._extract(scans)
        r = self._enqueue(y, scans, query_ids, nn_index, query_poses)
        if check is not None:
            try:
                check()                                        # [SYNC]
            except _lib.Fp16RangeError:
                r = self._enqueue(self.extractor.extract(scans), scans, query_ids, nn_index, query_poses)
                torch.cuda.synchronize(self.kmap.device)
        else:
            torch.cuda.synchronize(self.kmap.device)           # [SYNC]
        return r


def evaluate_relocalization(reloc: Relocalizer, query_scans: Sequence, query_poses, radius: Sequence[float] = (5, 20),
                            batch_size: int = 16) -> Dict:
    """Metrics of `reloc` on queries with known poses (Q,4,4), map poses from its KeypointMap:
      recall, recall_reranked   {r: [recall@1 .. recall@k]} of the retrieved lists and of the lists after verification
                                (egonn_recall_counts on the x, y of the poses' translations, offset by a common float64 origin
                                as `retrieval.recall_at_k` does)
      success                   share of queries whose verified pose meets the reference's rule rte <= 2 m and rre <= 5 deg
                                against inv(P_map[best]) @ P_query; an unverified query is a failure
      unverified                share of queries without a verified candidate
      rte, rre                  means over the successes (0. when there is none)
      success_inliers, failure_inliers   mean inliers of the winner over successes / over the other queries (0 for unverified)"""
    km, dev, lib = reloc.kmap, reloc.kmap.device, _lib.load()
    qp64 = torch.as_tensor(np.asarray(query_poses, dtype=np.float64)).reshape(-1, 4, 4)
    Q = qp64.shape[0]
    if len(query_scans) != Q:
        raise ValueError("evaluate_relocalization: one pose per query scan")
    parts = []
    for lo in range(0, Q, int(batch_size)):
        hi = min(Q, lo + int(batch_size))
        r = reloc.localize(query_scans[lo:hi], query_ids=torch.arange(lo, hi, dtype=torch.int32), query_poses=qp64[lo:hi])
        parts.append({n: r[n] for n in ("nn_index", "reranked", "best_index", "best_inliers", "best_success", "best_rte",
                                        "best_rre")})
    cat = {n: torch.cat([p[n] for p in parts]).contiguous() for n in parts[0]} if parts else {}
    k = reloc.k
    mp64 = km.poses[:, :2, 3].cpu()
    origin = mp64.mean(dim=0, keepdim=True) if len(km) else torch.zeros((1, 2), dtype=torch.float64)
    mp = (mp64 - origin).to(device=dev, dtype=torch.float32).contiguous()
    qp = (qp64[:, :2, 3] - origin).to(device=dev, dtype=torch.float32).contiguous()
    rad = torch.tensor([float(r) for r in radius], dtype=torch.float32, device=dev)
    res = {}
    for name, key in (("recall", "nn_index"), ("recall_reranked", "reranked")):
        tp = torch.zeros((len(radius), k), dtype=torch.int32, device=dev)
        if Q:
            _lib.call(dev, lib.egonn_recall_counts, cat[key].data_ptr(), qp.data_ptr(), mp.data_ptr(), Q, k, 2, rad.data_ptr(),
                      len(radius), tp.data_ptr())
        tpl = tp.cpu().tolist()
        res[name] = {r: [c / max(Q, 1) for c in tpl[i]] for i, r in enumerate(radius)}
    if not Q:
        res.update(success=0., unverified=0., rte=0., rre=0., success_inliers=0., failure_inliers=0.)
        return res
    suc = cat["best_success"].cpu().numpy().astype(bool)
    inl = cat["best_inliers"].cpu().numpy()
    mean = lambda v: float(np.mean(v)) if len(v) else 0.                     # noqa: E731
    res.update(success=float(suc.mean()), unverified=float((cat["best_index"].cpu().numpy() < 0).mean()),
               rte=mean(cat["best_rte"].cpu().numpy()[suc]), rre=mean(cat["best_rre"].cpu().numpy()[suc]),
               success_inliers=mean(inl[suc]), failure_inliers=mean(inl[~suc]))
    return res
