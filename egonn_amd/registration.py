"""6-DoF registration of keypoint sets on the device: the consumer of the local half of the descriptor path.

Mirrors the reference's names (eval/evaluate.py): `get_ransac_result` (:381-399), `calculate_repeatability` (:402-411),
plus `register_pairs` (batched) and `evaluate_local`, the per-n_k metric bookkeeping of
`MinkLocGLEvaluator.evaluate` (:188-292).  Matching, RANSAC, the final evaluation and the metrics run in libegonn_hip
(egonn_match_mutual / egonn_ransac_pairs / egonn_registration_finish); there is no torch or numpy fallback for the
arithmetic.

ICP refinement (misc/point_clouds.py:31-62: `icp`) runs on the full clouds in libegonn_hip as well (egonn_voxel_downsample /
egonn_icp_pairs, csrc/icp.hip): `voxel_downsample`, `icp_pairs` (batched) and `icp` (the reference's signature).  With
`query_clouds` / `map_clouds`, `evaluate_local` computes `T_refined` from `T_gt` on the device and reports the whole
`*_refined` family (:261-275); without them only `repeatability_refined`, computed with the caller's `T_refined`.
"""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import as_dev as _dev, check_cloud as _check_cloud, check_offsets as _check_offsets, concat_clouds as _concat_clouds

N_MAX = 256
MAX_PAIRS = 4096          # pairs per matching call (and per call sequence of relocalize.verify_candidates): the matching scratch
                          # is 9-36 KB per pair, and pairs are independent, so chunking cannot change a bit
STATUS_CLIPPED, STATUS_FEW_CORR, STATUS_NO_MODEL, STATUS_BAD_INDEX = 1, 2, 4, 8
ICP_FEW_CORR, ICP_MAX_ITER, ICP_EMPTY, ICP_RANGE = 1, 2, 4, 8
ICP_SINGULAR = 16                          # point-to-plane: the 6 x 6 solve met a pivot at rounding level (one plane, a corridor)
NORMALS_FEW_POINTS, NORMALS_RANGE = 1, 2
NORMALS_KNN = 20                           # misc/point_clouds.py:44-45: KDTreeSearchParamKNN(knn=20)
ICP_VOXEL_SIZE = 0.1                       # misc/point_clouds.py:37
ICP_EPS_FITNESS = ICP_EPS_RMSE = 1e-6      # Open3D's ICPConvergenceCriteria defaults [recall]


class RegistrationResult:
    """one pair's result with the attribute names of Open3D's RegistrationResult"""

    def __init__(self, transformation, correspondence_set, fitness, inlier_rmse, status):
        self.transformation = transformation            # (4,4) numpy float64
        self.correspondence_set = correspondence_set    # (inliers, 2) numpy int32
        self.fitness = fitness
        self.inlier_rmse = inlier_rmse
        self.status = status

    def __repr__(self):
        return (f"RegistrationResult(fitness={self.fitness:.6f}, inlier_rmse={self.inlier_rmse:.6f}, "
                f"correspondence_set={len(self.correspondence_set)}, status={self.status})")


def _counts(n, P, n_rows, dev):
    if n is None:
        return torch.full((P,), n_rows, dtype=torch.int32, device=dev)
    n = _dev(n, dev, torch.int32)
    assert n.shape == (P,), "per-pair counts must have shape (P,)"
    return n


def match_mutual(feat1: torch.Tensor, feat2: torch.Tensor, n1=None, n2=None, chunk_pairs: int = MAX_PAIRS):
    """(P, n_max, D) x 2 -> corr (P, n_max, 2) int32 compacted in ascending source index (unused rows -1), n_corr (P,).
    Issued in chunks of at most `chunk_pairs` (<= 4096) pairs on one scratch buffer."""
    dev = feat1.device if feat1.is_cuda else _lib.require_gpu()
    lib = _lib.load()
    f1, f2 = _dev(feat1, dev, torch.float32), _dev(feat2, dev, torch.float32)
    assert f1.dim() == 3 and f1.shape == f2.shape, "descriptors: (P, n_max, D), both sides padded alike"
    P, n_max, D = f1.shape
    c1, c2 = _counts(n1, P, n_max, dev), _counts(n2, P, n_max, dev)
    corr = torch.empty((P, n_max, 2), dtype=torch.int32, device=dev)
    n_corr = torch.empty((P,), dtype=torch.int32, device=dev)
    pc = max(1, min(int(chunk_pairs), MAX_PAIRS, P))
    scratch = _lib.scratch(lib.egonn_match_mutual_scratch_bytes(pc, n_max), dev)     # -1 on bad arguments: the call raises
    for lo in range(0, max(P, 1), pc):                                               # (P = 0: one call, for its checks)
        s = slice(lo, min(P, lo + pc))
        _lib.call(dev, lib.egonn_match_mutual, f1[s].data_ptr(), f2[s].data_ptr(), c1[s].data_ptr(), c2[s].data_ptr(),
                  s.stop - s.start, n_max, D, corr[s].data_ptr(), n_corr[s].data_ptr(), scratch.data_ptr(), scratch.numel() * 8)
    return corr, n_corr


METHODS = ("ransac", "spectral")
SPECTRAL_D_THR, SPECTRAL_ITERATIONS, SPECTRAL_SEED_RATIO = 0.6, 32, 0.5      # choices, not tuned values (`spectral_verify`)
# The per-pair outputs of egonn_registration_finish and egonn_spectral_verify, in the order of the C prototypes: name, dtype,
# trailing shape ("n" = n_max), only with T_gt, the method that owns it (None = both: PairOut of csrc/pair_eval.h).
_F, _I = torch.float64, torch.int32
PAIR_OUTPUTS = (
    ("eigenvalue", _F, (), False, "spectral"), ("score", _F, (), False, "spectral"), ("weights", _F, ("n",), False, "spectral"),
    ("n_seeds", _I, (), False, "spectral"),
    ("T", _F, (4, 4), False, None), ("inliers", _I, (), False, None), ("fitness", _F, (), False, None),
    ("inlier_rmse", _F, (), False, None), ("correspondence_set", _I, ("n", 2), False, None),
    ("best_t", _I, (), False, "ransac"),
    ("rte", _F, (), True, None), ("rre", _F, (), True, None), ("success", _I, (), True, None), ("repeatability", _F, (), True, None),
    ("status", _I, (), False, None))


def check_method(who, method):
    if method not in METHODS:
        raise ValueError(f"{who}: method must be one of {METHODS}, got {method!r}")
    return method


def pair_outputs(method, with_gt=True, skip=()):
    """the rows of PAIR_OUTPUTS that `method` writes, in the order its C entry point takes them"""
    return tuple(r for r in PAIR_OUTPUTS if r[4] in (None, method) and (with_gt or not r[3]) and r[0] not in skip)


def pair_buffers(dev, lead, n_max, with_gt, method, skip=()):
    """{name: empty tensor of shape lead + trailing shape} for those rows"""
    return {name: torch.empty((*lead, *(n_max if s == "n" else s for s in shape)), dtype=dt, device=dev)
            for name, dt, shape, _, _ in pair_outputs(method, with_gt, skip)}


def _out_ptrs(method, out):
    return [_lib._ptr(out.get(r[0])) for r in pair_outputs(method)]


def enqueue_ransac(dev, operands, P, n_max, H, seed, dist_th, scratch, T_gt, repeat_th, out):
    """egonn_ransac_pairs + egonn_registration_finish of P pairs.  operands: the pointers (kp1, kp2, n1, n2, corr, n_corr,
    pair_id) both calls start with; scratch: `_lib.scratch` of egonn_registration_scratch_bytes; T_gt: (P,4,4) f64 tensor or
    None; out: the outputs by the names of `register_pairs` (an absent one is not computed).  Nothing is allocated and
    nothing synchronises, so the pair can be captured; the caller keeps the operands alive."""
    lib = _lib.load()
    head = (*operands, P, n_max, H, int(seed) & 0xFFFFFFFFFFFFFFFF, float(dist_th), scratch.data_ptr(), scratch.numel() * 8)
    _lib.call(dev, lib.egonn_ransac_pairs, *head, _lib._ptr(out.get("hyp_count")), _lib._ptr(out.get("hyp_err2")))
    _lib.call(dev, lib.egonn_registration_finish, *head, _lib._ptr(T_gt), float(repeat_th), *_out_ptrs("ransac", out))


def enqueue_spectral(dev, operands, P, n_max, d_thr, iterations, seed_ratio, dist_th, scratch, T_gt, repeat_th, out):
    """egonn_spectral_verify of P pairs.  operands: the pointers (kp1, kp2, n1, n2, corr, n_corr); scratch: `_lib.scratch` of
    egonn_spectral_verify_scratch_bytes; T_gt: (P,4,4) f64 tensor or None; out: the outputs by the names of `spectral_verify`
    (an absent one is not computed).  Nothing is allocated and nothing synchronises, so the call can be captured; the caller
    keeps the operands alive."""
    lib = _lib.load()
    _lib.call(dev, lib.egonn_spectral_verify, *operands, P, n_max, float(d_thr), int(iterations), float(seed_ratio),
              float(dist_th), _lib._ptr(T_gt), float(repeat_th), scratch.data_ptr(), scratch.numel() * 8,
              *_out_ptrs("spectral", out))


def spectral_verify(kp1, kp2, corr, n_corr, n1=None, n2=None, T_gt=None, d_thr: float = SPECTRAL_D_THR,
                    iterations: int = SPECTRAL_ITERATIONS, seed_ratio: float = SPECTRAL_SEED_RATIO, dist_th: float = 0.5,
                    out=None, repeat_dist_th: float = 0.5) -> Dict[str, torch.Tensor]:
    """Spectral geometric verification of P pairs (egonn_spectral_verify, csrc/spectral.hip): no hypotheses, no seed.

    kp (P, n_max, 3), corr (P, n_max, 2) int32 with n_corr (P,) valid rows (what `match_mutual` returns), n1 / n2 (P,) keypoint
    counts (None = n_max), T_gt (P,4,4) or None.  The pairwise length-consistency matrix M_ij = max(0, 1 - d_ij^2 / d_thr^2)
    of the correspondences, `iterations` power iterations from the uniform vector, eigenvalue = v^T M v (about the size of the
    consistent set minus 1), score = eigenvalue / (n_max - 1), seeds = correspondences with v_i >= seed_ratio * max v, a rigid
    fit on the seeds, its inliers under dist_th, a refit on them, then the final evaluation of `register_pairs`.

    Returns device tensors: eigenvalue, score (P,) f64, weights (P, n_max) f64 (v, zero beyond n_corr), n_seeds (P,) i32, and
    with the meaning they have in `register_pairs`: T, inliers, fitness, inlier_rmse, correspondence_set, status, with T_gt
    also rte, rre, success, repeatability.

    d_thr = 0.6 m, 32 iterations and seed_ratio = 0.5 are choices, not tuned values: there are neither trained weights nor
    data to tune on in this project.

    No host synchronisation when the inputs are device tensors.  `out`: the dict of an earlier call with the same shapes; its
    buffers (scratch included) are used again and nothing is allocated, which a graph capture needs."""
    dev = kp1.device if torch.is_tensor(kp1) and kp1.is_cuda else _lib.require_gpu()
    k1, k2 = _dev(kp1, dev, torch.float32), _dev(kp2, dev, torch.float32)
    if k1.dim() != 3 or k1.shape[2] != 3 or k1.shape != k2.shape:
        raise ValueError(f"spectral_verify: keypoints must be (P, n_max, 3) on both sides, got {tuple(k1.shape)}, {tuple(k2.shape)}")
    P, n_max = k1.shape[0], k1.shape[1]
    c, nc = _dev(corr, dev, torch.int32), _dev(n_corr, dev, torch.int32)
    if tuple(c.shape) != (P, n_max, 2) or tuple(nc.shape) != (P,):
        raise ValueError(f"spectral_verify: corr must be ({P}, {n_max}, 2) and n_corr ({P},), got {tuple(c.shape)}, {tuple(nc.shape)}")
    c1, c2 = _counts(n1, P, n_max, dev), _counts(n2, P, n_max, dev)
    gt = None if T_gt is None else _dev(T_gt, dev, torch.float64).reshape(P, 4, 4)
    if out is None:
        out = pair_buffers(dev, (P,), n_max, gt is not None, "spectral")
        out["_scratch"] = _lib.scratch(_lib.load().egonn_spectral_verify_scratch_bytes(P, n_max), dev)   # -1: the call raises
    elif "weights" not in out or tuple(out["weights"].shape) != (P, n_max) or ("rte" in out) != (gt is not None) or \
            out["weights"].device != dev:
        raise ValueError("spectral_verify: `out` was made by a call with other shapes")
    enqueue_spectral(dev, (k1.data_ptr(), k2.data_ptr(), c1.data_ptr(), c2.data_ptr(), c.data_ptr(), nc.data_ptr()), P, n_max,
                     d_thr, iterations, seed_ratio, dist_th, out["_scratch"], gt, repeat_dist_th, out)
    out["_keep"] = (k1, k2, c1, c2, c, nc, gt)             # inputs of enqueued work stay alive with the result
    return out


def register_pairs(feat1, feat2, kp1, kp2, n1=None, n2=None, T_gt=None, ransac_dist_th: float = 0.5,
                   ransac_max_it: int = 10000, seed: int = 0, pair_ids=None, repeat_dist_th: float = 0.5,
                   debug: bool = False, method: str = "ransac", d_thr: float = SPECTRAL_D_THR,
                   iterations: int = SPECTRAL_ITERATIONS, seed_ratio: float = SPECTRAL_SEED_RATIO) -> Dict[str, torch.Tensor]:
    """P pairs at once.  feat (P, n_max, D), kp (P, n_max, 3), n1 / n2 (P,) row counts (None = n_max), T_gt (P,4,4) or None.
    Returns device tensors: T (P,4,4) f64, inliers (P,) i32, fitness, inlier_rmse (P,) f64, correspondence_set
    (P, n_max, 2) i32 (rows beyond `inliers` are -1), best_t, status (P,) i32, corr, n_corr; with T_gt also rte, rre (f64),
    success (i32), repeatability (f64); with debug the per-hypothesis tables hyp_count (P,H) i32 and hyp_err2 (P,H) f64.
    pair_ids (P,) int32: the id that enters the draws, its low 30 bits (None = position in the batch).
    No host synchronisation when every array argument is a device tensor (host arrays or lists are copied over first); such a
    call can be captured into a graph.
    method="spectral": the same matching, then `spectral_verify` (d_thr, iterations, seed_ratio; ransac_dist_th is its
    dist_th) instead of RANSAC: the same keys plus eigenvalue, score, weights and n_seeds, without best_t; ransac_max_it, seed,
    pair_ids and debug are accepted and ignored."""
    check_method("register_pairs", method)
    dev = feat1.device if torch.is_tensor(feat1) and feat1.is_cuda else _lib.require_gpu()
    lib = _lib.load()
    f1 = _dev(feat1, dev, torch.float32)
    assert f1.dim() == 3, "descriptors: (P, n_max, D)"
    P, n_max = f1.shape[0], f1.shape[1]
    c1, c2 = _counts(n1, P, n_max, dev), _counts(n2, P, n_max, dev)          # converted once: host counts cost one copy each
    corr, n_corr = match_mutual(f1, _dev(feat2, dev, torch.float32), c1, c2)
    k1, k2 = _dev(kp1, dev, torch.float32), _dev(kp2, dev, torch.float32)
    assert k1.shape == (P, n_max, 3) and k2.shape == (P, n_max, 3), "keypoints: (P, n_max, 3), padded like the descriptors"
    if method == "spectral":
        out = spectral_verify(k1, k2, corr, n_corr, c1, c2, T_gt, d_thr, iterations, seed_ratio, ransac_dist_th,
                              repeat_dist_th=repeat_dist_th)
        out.update(corr=corr, n_corr=n_corr)
        return out
    H = int(ransac_max_it)
    pid = None if pair_ids is None else _dev(pair_ids, dev, torch.int32)
    gt = None if T_gt is None else _dev(T_gt, dev, torch.float64).reshape(P, 4, 4)
    scratch = _lib.scratch(lib.egonn_registration_scratch_bytes(P, n_max, H), dev)   # -1 on bad arguments: the call raises
    out = pair_buffers(dev, (P,), n_max, gt is not None, "ransac")
    out.update(corr=corr, n_corr=n_corr)
    if debug:
        out.update({"hyp_count": torch.empty((P, max(H, 0)), dtype=torch.int32, device=dev),
                    "hyp_err2": torch.empty((P, max(H, 0)), dtype=torch.float64, device=dev)})
    enqueue_ransac(dev, (k1.data_ptr(), k2.data_ptr(), c1.data_ptr(), c2.data_ptr(), corr.data_ptr(), n_corr.data_ptr(),
                         _lib._ptr(pid)), P, n_max, H, seed, ransac_dist_th, scratch, gt, repeat_dist_th, out)
    out["_keep"] = (k1, k2, c1, c2, pid, gt, scratch)      # inputs of enqueued work stay alive with the result
    return out


def get_ransac_result(feat1, feat2, kp1, kp2, ransac_dist_th: float = 0.5, ransac_max_it: int = 10000, seed: int = 0):
    """eval/evaluate.py:381-399 for one pair: feat (n, D), kp (n, 3); n1 != n2 allowed.  [SYNC] copies the result back."""
    dev = _lib.require_gpu() if not (torch.is_tensor(feat1) and feat1.is_cuda) else feat1.device
    f1, f2 = torch.as_tensor(feat1), torch.as_tensor(feat2)
    k1, k2 = torch.as_tensor(kp1), torch.as_tensor(kp2)
    assert f1.dim() == 2 and f2.dim() == 2 and f1.shape[1] == f2.shape[1] and k1.shape == (f1.shape[0], 3) \
        and k2.shape == (f2.shape[0], 3), "feat (n, D) and kp (n, 3) per side"
    n_max = max(f1.shape[0], f2.shape[0], 1)
    if n_max > N_MAX:
        raise ValueError(f"get_ransac_result: at most {N_MAX} keypoints per side, got {n_max}")

    def pad(x, w):
        o = torch.zeros((1, n_max, w), dtype=torch.float32, device=dev)
        o[0, :x.shape[0]] = x.to(device=dev, dtype=torch.float32)
        return o

    r = register_pairs(pad(f1, f1.shape[1]), pad(f2, f1.shape[1]), pad(k1, 3), pad(k2, 3), n1=[f1.shape[0]], n2=[f2.shape[0]],
                       ransac_dist_th=ransac_dist_th, ransac_max_it=ransac_max_it, seed=seed)
    n_in = int(r["inliers"][0])
    return RegistrationResult(r["T"][0].cpu().numpy(), r["correspondence_set"][0, :n_in].cpu().numpy(), float(r["fitness"][0]),
                              float(r["inlier_rmse"][0]), int(r["status"][0]))


def repeatability_pairs(kp1, kp2, T, threshold: float, n1=None, n2=None) -> torch.Tensor:
    """batched calculate_repeatability: kp (P, n_max, 3), T (P,4,4) -> (P,) f64 on the device"""
    dev = kp1.device if torch.is_tensor(kp1) and kp1.is_cuda else _lib.require_gpu()
    lib = _lib.load()
    k1, k2 = _dev(kp1, dev, torch.float32), _dev(kp2, dev, torch.float32)
    P, n_max = k1.shape[0], k1.shape[1]
    assert k1.dim() == 3 and k1.shape == k2.shape and k1.shape[2] == 3
    c1, c2 = _counts(n1, P, n_max, dev), _counts(n2, P, n_max, dev)
    gt = _dev(T, dev, torch.float64).reshape(P, 4, 4)
    rep = torch.empty((P,), dtype=torch.float64, device=dev)
    _lib.call(dev, lib.egonn_registration_finish, k1.data_ptr(), k2.data_ptr(), c1.data_ptr(), c2.data_ptr(), None, None, None,
              P, n_max, 0, 0, 0.0, None, 0, gt.data_ptr(), float(threshold), *_out_ptrs("ransac", {"repeatability": rep}))
    return rep


def calculate_repeatability(kp1, kp2, T_gt, threshold: float) -> float:
    """eval/evaluate.py:402-411 for one pair (kp1 (n1,3), kp2 (n2,3)); the transform is applied in float64 on the device."""
    dev = _lib.require_gpu() if not (torch.is_tensor(kp1) and kp1.is_cuda) else kp1.device
    k1, k2 = torch.as_tensor(kp1), torch.as_tensor(kp2)
    n_max = max(k1.shape[0], k2.shape[0], 1)
    if n_max > N_MAX:
        raise ValueError(f"calculate_repeatability: at most {N_MAX} keypoints per side, got {n_max}")
    a = torch.zeros((1, n_max, 3), dtype=torch.float32, device=dev)
    b = torch.zeros((1, n_max, 3), dtype=torch.float32, device=dev)
    a[0, :k1.shape[0]] = k1.to(device=dev, dtype=torch.float32)
    b[0, :k2.shape[0]] = k2.to(device=dev, dtype=torch.float32)
    rep = repeatability_pairs(a, b, np.asarray(T_gt, dtype=np.float64).reshape(1, 4, 4), threshold, [k1.shape[0]], [k2.shape[0]])
    return float(rep[0])


# ------------------------------------------------------------------ ICP refinement on the full clouds
def _check_crop(crop):
    if crop is None:
        return None
    c = [float("nan") if v is None else float(v) for v in crop]
    if len(c) != 6:
        raise ValueError("crop: (min_x, max_x, min_y, max_y, min_z, max_z), None or NaN = no bound")
    import ctypes
    return (ctypes.c_float * 6)(*c)


def voxel_downsample(points, offsets, voxel_size: float = ICP_VOXEL_SIZE, crop=None) -> Dict[str, torch.Tensor]:
    """Voxel-grid downsample (Open3D voxel_down_sample, restated in csrc/icp.hip) of concatenated clouds: points (n,3),
    cloud c = rows [offsets[c], offsets[c+1]).  crop = (min_x, max_x, min_y, max_y, min_z, max_z) with None / NaN = no bound,
    applied first by the rules of preprocess_pointcloud (> min, <= max).  Returns device tensors: points (n,3) f64 (the first
    offsets[-1] rows valid, ascending voxel index inside a cloud), offsets (n_clouds+1,) int64, counts (n,) int32 points per
    voxel, status (n_clouds,) int32 (ICP_RANGE: a voxel index beyond 21 bits, nothing written for the cloud).
    No host synchronisation when points and offsets are device tensors."""
    _check_cloud("voxel_downsample", points)
    C = _check_offsets("voxel_downsample", offsets)
    if not float(voxel_size) > 0.0:
        raise ValueError("voxel_downsample: voxel_size must be positive")
    cr = _check_crop(crop)
    dev = points.device if torch.is_tensor(points) and points.is_cuda else _lib.require_gpu()
    lib = _lib.load()
    pts, off = _dev(points, dev, torch.float32), _dev(offsets, dev, torch.int64)
    n = pts.shape[0]
    scratch = _lib.scratch(lib.egonn_voxel_downsample_scratch_bytes(n, C), dev)
    out = {"points": torch.empty((n, 3), dtype=torch.float64, device=dev),
           "offsets": torch.empty((C + 1,), dtype=torch.int64, device=dev),
           "counts": torch.zeros((n,), dtype=torch.int32, device=dev),
           "status": torch.empty((C,), dtype=torch.int32, device=dev)}
    _lib.call(dev, lib.egonn_voxel_downsample, _lib._ptr(pts) if n else None, n, off.data_ptr(), C, float(voxel_size), cr,
              out["points"].data_ptr() if n else None, out["offsets"].data_ptr(), out["counts"].data_ptr() if n else None,
              out["status"].data_ptr(), scratch.data_ptr(), scratch.numel() * 8)
    out["_keep"] = (pts, off, scratch)
    return out


def estimate_normals(points, offsets, knn: int = NORMALS_KNN, debug: bool = False) -> Dict[str, torch.Tensor]:
    """Surface normals of concatenated clouds (Open3D estimate_normals(KDTreeSearchParamKNN(knn)), restated in csrc/icp.hip):
    points (n,3) float64 (what `voxel_downsample` returns) with (n_clouds+1,) offsets, knn in [3, 32].  Per point the exact
    min(knn, cloud size) nearest points of its cloud (itself included, by (d2, index)), their covariance, the unit eigenvector
    of its smallest eigenvalue, oriented toward the origin of the cloud's frame.  Returns device tensors normals (n,3) f64 and
    status (n_clouds,) int32 (NORMALS_* bits); with debug also neighbors (n, knn) int32 (index inside the cloud, -1 beyond
    the count) and eigenvalues (n,3) ascending.  No host synchronisation when the arguments are device tensors."""
    _check_cloud("estimate_normals", points)
    C = _check_offsets("estimate_normals", offsets)
    knn = int(knn)
    if not 3 <= knn <= 32:
        raise ValueError(f"estimate_normals: knn must be in [3, 32], got {knn}")
    dev = points.device if torch.is_tensor(points) and points.is_cuda else _lib.require_gpu()
    lib = _lib.load()
    pts, off = _dev(points, dev, torch.float64), _dev(offsets, dev, torch.int64)
    n = pts.shape[0]
    scratch = _lib.scratch(lib.egonn_estimate_normals_scratch_bytes(n, C), dev)
    out = {"normals": torch.empty((n, 3), dtype=torch.float64, device=dev), "status": torch.empty((C,), dtype=torch.int32, device=dev)}
    if debug:
        out.update({"neighbors": torch.empty((n, knn), dtype=torch.int32, device=dev),
                    "eigenvalues": torch.empty((n, 3), dtype=torch.float64, device=dev)})
    _lib.call(dev, lib.egonn_estimate_normals, pts.data_ptr() if n else None, n, off.data_ptr(), C, knn,
              out["normals"].data_ptr() if n else None, out["status"].data_ptr(), _lib._ptr(out.get("neighbors")) if n else None,
              _lib._ptr(out.get("eigenvalues")) if n else None, scratch.data_ptr(), scratch.numel() * 8)
    out["_keep"] = (pts, off, scratch)
    return out


def icp_pairs(src, src_offsets, tgt, tgt_offsets, T_init=None, inlier_dist_threshold: float = 1.2, max_iteration: int = 200,
              debug: bool = False, tgt_normals=None) -> Dict[str, torch.Tensor]:
    """Point-to-point ICP of P (source, target) pairs (Open3D registration_icp, restated in csrc/icp.hip): src / tgt (n,3)
    float64 concatenated clouds (what `voxel_downsample` returns) with (P+1,) offsets, T_init (P,4,4) or None = identity.
    Returns device tensors T (P,4,4) f64, fitness, inlier_rmse (P,) f64, iterations, status (P,) int32 (ICP_* bits); with
    debug also T_trace (P, max_iteration+1, 4, 4), eval_trace (P, max_iteration+1, 3) = (n_corr, sum d2, stop) and corr
    (n_src,) int32 = j(i) of the last evaluation or -1.  No host synchronisation when the arguments are device tensors: the
    call enqueues a fixed launch sequence and can be captured into a graph.
    tgt_normals (n_tgt,3) float64 (`estimate_normals` of tgt) switches to the point-to-plane estimator (egonn_icp_plane_pairs):
    same evaluation, stop rule and tables; fewer than 6 correspondences give ICP_FEW_CORR, a rank-deficient scene
    ICP_SINGULAR.  None is the point-to-point call, unchanged."""
    _check_cloud("icp_pairs: src", src)
    _check_cloud("icp_pairs: tgt", tgt)
    P = _check_offsets("icp_pairs: src_offsets", src_offsets)
    if _check_offsets("icp_pairs: tgt_offsets", tgt_offsets) != P:
        raise ValueError("icp_pairs: src_offsets and tgt_offsets must describe the same number of pairs")
    if T_init is not None and tuple(T_init.shape) != (P, 4, 4):
        raise ValueError(f"icp_pairs: T_init must have shape ({P}, 4, 4), got {tuple(T_init.shape)}")
    if int(max_iteration) < 0 or not float(inlier_dist_threshold) > 0.0:
        raise ValueError("icp_pairs: max_iteration >= 0 and inlier_dist_threshold > 0 required")
    if tgt_normals is not None and tuple(tgt_normals.shape) != (tgt.shape[0], 3):
        raise ValueError(f"icp_pairs: tgt_normals must have shape ({tgt.shape[0]}, 3), got {tuple(tgt_normals.shape)}")
    dev = src.device if torch.is_tensor(src) and src.is_cuda else _lib.require_gpu()
    lib = _lib.load()
    s, t = _dev(src, dev, torch.float64), _dev(tgt, dev, torch.float64)       # fp32 inputs convert exactly
    so, to = _dev(src_offsets, dev, torch.int64), _dev(tgt_offsets, dev, torch.int64)
    ti = None if T_init is None else _dev(T_init, dev, torch.float64)
    ns, nt, K = s.shape[0], t.shape[0], int(max_iteration)
    tn = None if tgt_normals is None else _dev(tgt_normals, dev, torch.float64)
    scratch = _lib.scratch((lib.egonn_icp_scratch_bytes if tn is None else lib.egonn_icp_plane_scratch_bytes)(ns, nt, P), dev)
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)        # noqa: E731
    i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)          # noqa: E731
    out = {"T": f64(P, 4, 4), "fitness": f64(P), "inlier_rmse": f64(P), "iterations": i32(P), "status": i32(P)}
    if debug:
        out.update({"T_trace": f64(P, K + 1, 4, 4), "eval_trace": f64(P, K + 1, 3), "corr": i32(ns)})
    p = lambda k: _lib._ptr(out.get(k))                                       # noqa: E731
    head = (s.data_ptr() if ns else None, ns, so.data_ptr(), t.data_ptr() if nt else None, nt, to.data_ptr())
    tail = (P, _lib._ptr(ti), float(inlier_dist_threshold), K, ICP_EPS_FITNESS, ICP_EPS_RMSE, p("T"), p("fitness"),
            p("inlier_rmse"), p("iterations"), p("status"), p("T_trace"), p("eval_trace"), p("corr") if ns else None,
            scratch.data_ptr(), scratch.numel() * 8)
    if tn is None:
        _lib.call(dev, lib.egonn_icp_pairs, *head, *tail)
    else:
        _lib.call(dev, lib.egonn_icp_plane_pairs, *head, tn.data_ptr() if nt else None, *tail)
    out["_keep"] = (s, t, so, to, ti, tn, scratch)
    return out


def refine_pairs(src_clouds, tgt_clouds, T_init=None, crop=None, inlier_dist_threshold: float = 1.2, max_iteration: int = 200,
                 debug: bool = False, point2plane: bool = False, knn: int = NORMALS_KNN) -> Dict[str, torch.Tensor]:
    """icp() for P pairs of full clouds (lists of (n,3) arrays): crop, downsample both sides, ICP.  The `icp_pairs` result.
    point2plane: normals of the downsampled target side (`estimate_normals`, knn neighbours), then the point-to-plane
    estimator.  (The reference estimates the source's normals as well; point-to-plane never reads them.)"""
    if len(src_clouds) != len(tgt_clouds):
        raise ValueError("refine_pairs: as many source as target clouds")
    for c in list(src_clouds) + list(tgt_clouds):
        _check_cloud("refine_pairs", c)
    dev = _lib.require_gpu()
    a = voxel_downsample(*_concat_clouds(src_clouds, dev), crop=crop)
    b = voxel_downsample(*_concat_clouds(tgt_clouds, dev), crop=crop)
    nrm = estimate_normals(b["points"], b["offsets"], knn) if point2plane else None
    r = icp_pairs(a["points"], a["offsets"], b["points"], b["offsets"], T_init, inlier_dist_threshold, max_iteration, debug,
                  None if nrm is None else nrm["normals"])
    r["_clouds"] = (a, b, nrm)
    return r


def icp(anchor_pc, positive_pc, transform=None, point2plane: bool = False, inlier_dist_threshold: float = 1.2,
        max_iteration: int = 200):
    """misc/point_clouds.py:31-62 for one pair: -> (T (4,4) numpy float64, fitness, inlier_rmse).  [SYNC] copies the result
    back.  point2plane=True still raises NotImplementedError: the tests of the point-to-point pull request pin that refusal
    (tests/test_icp_host.py, tests/test_gpu_icp.py).  The point-to-plane estimator is `icp_point_to_plane`; a change that may
    touch those tests can route the flag there."""
    if point2plane:
        raise NotImplementedError("icp: point2plane=True is refused here; call icp_point_to_plane for the point-to-plane estimation")
    return _icp_one("icp", anchor_pc, positive_pc, transform, inlier_dist_threshold, max_iteration, False, NORMALS_KNN)


def icp_point_to_plane(anchor_pc, positive_pc, transform=None, inlier_dist_threshold: float = 1.2, max_iteration: int = 200,
                       knn: int = NORMALS_KNN):
    """icp(..., point2plane=True) of misc/point_clouds.py:31-62 for one pair: normals of the downsampled target from its knn
    nearest neighbours, then point-to-plane ICP -> (T (4,4) numpy float64, fitness, inlier_rmse).  [SYNC] copies the result
    back.  The one-pair form of `refine_pairs(point2plane=True)`."""
    return _icp_one("icp_point_to_plane", anchor_pc, positive_pc, transform, inlier_dist_threshold, max_iteration, True, knn)


def _icp_one(who, anchor_pc, positive_pc, transform, inlier_dist_threshold, max_iteration, point2plane, knn):
    _check_cloud(f"{who}: anchor_pc", anchor_pc)
    _check_cloud(f"{who}: positive_pc", positive_pc)
    if not 3 <= int(knn) <= 32:
        raise ValueError(f"{who}: knn must be in [3, 32], got {knn}")
    ti = None
    if transform is not None:
        ti = torch.as_tensor(np.asarray(transform, dtype=np.float64))
        if tuple(ti.shape) != (4, 4):
            raise ValueError(f"{who}: transform must be (4, 4), got {tuple(ti.shape)}")
        ti = ti.reshape(1, 4, 4)
    r = refine_pairs([anchor_pc], [positive_pc], ti, None, inlier_dist_threshold, max_iteration, False, point2plane, knn)
    return r["T"][0].cpu().numpy(), float(r["fitness"][0]), float(r["inlier_rmse"][0])


def _metrics_against(r, T_ref, n_max, ransac_max_it, seed, ransac_dist_th, repeat_dist_th):
    """rte / rre / success / repeatability of a `register_pairs` result against another pose T_ref (P,4,4) on the device:
    egonn_registration_finish again, on the scratch the result still holds (same winner, same bits)."""
    lib = _lib.load()
    k1, k2, c1, c2, pid, _, scratch = r["_keep"]
    dev, P = k1.device, k1.shape[0]
    ref = _dev(T_ref, dev, torch.float64).reshape(P, 4, 4)
    out = pair_buffers(dev, (P,), n_max, True, "ransac", skip=("correspondence_set", "best_t", "status"))
    _lib.call(dev, lib.egonn_registration_finish, k1.data_ptr(), k2.data_ptr(), c1.data_ptr(), c2.data_ptr(),
              r["corr"].data_ptr(), r["n_corr"].data_ptr(), _lib._ptr(pid), P, n_max, int(ransac_max_it),
              int(seed) & 0xFFFFFFFFFFFFFFFF, float(ransac_dist_th), scratch.data_ptr(), scratch.numel() * 8, ref.data_ptr(),
              float(repeat_dist_th), *_out_ptrs("ransac", out))
    out["_keep"] = (ref,)
    return out


def _stack(items, idx, key, n_k, width, dev):
    """pad the first n_k rows of items[i][key] for i in idx to (len(idx), n_k, width) + counts"""
    out = torch.zeros((len(idx), n_k, width), dtype=torch.float32, device=dev)
    cnt = []
    for r, i in enumerate(idx):
        x = torch.as_tensor(items[i][key])[:n_k]
        out[r, :x.shape[0]] = x.to(device=dev, dtype=torch.float32)
        cnt.append(x.shape[0])
    return out, cnt


def evaluate_local(local_query: Sequence[dict], local_map: Sequence[dict], nn_index, T_gt, n_k: Sequence[int] = (128,),
                   euclid_dist=None, T_refined=None, ransac_dist_th: float = 0.5, ransac_max_it: int = 10000,
                   repeat_dist_th: float = 0.5, seed: int = 0, query_clouds=None, map_clouds=None, crop=None,
                   icp_dist_th: float = 1.2, icp_max_it: int = 200, icp_point2plane: bool = False) -> Dict[int, Dict[str, float]]:
    """The local-descriptor half of MinkLocGLEvaluator.evaluate (eval/evaluate.py:188-292) for all queries at once.

    local_query / local_map: per scan {'keypoints': (n,3), 'features': (n,D)} (compute_embeddings, :323); nn_index (Q,) or
    (Q,k): the retrieved map element per query (column 0 is used, :197); T_gt (Q,4,4): relative pose of query and that
    element; euclid_dist (Q,) or (Q,k): when given, queries whose first neighbour is farther than 20 m are skipped (:192).
    Returns {n_k: {'rre', 'rte', 'repeatability', 'success', 'success_inliers', 'failure_inliers', 'repeatability_refined',
    't_ransac', 't_ransac_sd'}} with the reference's conventions (rre / rte averaged over successes, empty lists -> 0.;
    t_ransac = the device time of the batched call divided by its pairs: ONE measurement, so 't_ransac_sd' is reported as 0.
    rather than computed).  The pair id of the draws is the query index.

    query_clouds / map_clouds (per-scan (n,3) arrays, indexed like local_query / local_map) switch the ICP refinement on
    (icp_refine, :215-236): T_refined = icp(query cloud, map cloud, T_gt) on the device, after the optional `crop` (min_x,
    max_x, min_y, max_y, min_z, max_z) on both clouds; a caller's T_refined is then not used.  The dict then also carries
    'rre_refined', 'rte_refined', 'success_refined', 'success_inliers_refined', 'failure_inliers_refined' (:261-275).
    icp_point2plane refines with the point-to-plane estimator (`refine_pairs(point2plane=True)`)."""
    if (query_clouds is None) != (map_clouds is None):
        raise ValueError("evaluate_local: query_clouds and map_clouds go together")
    refine = query_clouds is not None
    dev = _lib.require_gpu()
    nn = torch.as_tensor(nn_index).reshape(len(local_query), -1)[:, 0].tolist()
    sel = list(range(len(local_query)))
    if euclid_dist is not None:
        ed = torch.as_tensor(euclid_dist, dtype=torch.float64).reshape(len(local_query), -1)[:, 0].tolist()
        sel = [q for q in sel if not ed[q] > 20]
    gt_all = torch.as_tensor(np.asarray(T_gt, dtype=np.float64)).reshape(-1, 4, 4)
    ref_all = None if T_refined is None else torch.as_tensor(np.asarray(T_refined, dtype=np.float64)).reshape(-1, 4, 4)
    keys = ('rre', 'rte', 'repeatability', 'success', 'success_inliers', 'failure_inliers', 'repeatability_refined')
    if refine:
        keys += ('rre_refined', 'rte_refined', 'success_refined', 'success_inliers_refined', 'failure_inliers_refined')
    mean_metrics = {}
    icp_res = None
    if refine and sel:                                    # one batched call for every n_k: the clouds do not depend on it
        icp_res = refine_pairs([query_clouds[q] for q in sel], [map_clouds[nn[q]] for q in sel], gt_all[sel], crop,
                               icp_dist_th, icp_max_it, point2plane=bool(icp_point2plane))
    for nk in n_k:
        if nk > N_MAX:
            raise ValueError(f"evaluate_local: n_k {nk} exceeds {N_MAX}")
        m = {k: [] for k in keys}
        t_pair = 0.
        if sel:
            D = int(torch.as_tensor(local_query[sel[0]]['features']).shape[1])
            f1, c1 = _stack(local_query, sel, 'features', nk, D, dev)
            k1, _ = _stack(local_query, sel, 'keypoints', nk, 3, dev)
            mi = [nn[q] for q in sel]
            f2, c2 = _stack(local_map, mi, 'features', nk, D, dev)
            k2, _ = _stack(local_map, mi, 'keypoints', nk, 3, dev)
            gt = gt_all[sel]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = register_pairs(f1, f2, k1, k2, n1=c1, n2=c2, T_gt=gt, ransac_dist_th=ransac_dist_th, ransac_max_it=ransac_max_it,
                               seed=seed, pair_ids=sel, repeat_dist_th=repeat_dist_th)
            e1.record()
            rr = None
            if refine:       # the estimate against T_refined: the finish kernel once more on the same hypotheses' bests
                rr = _metrics_against(r, icp_res["T"], nk, ransac_max_it, seed, ransac_dist_th, repeat_dist_th)
                rep_ref = rr["repeatability"]
            else:
                ref = gt if ref_all is None else ref_all[sel]
                rep_ref = r["repeatability"] if ref_all is None else repeatability_pairs(k1, k2, ref, repeat_dist_th, c1, c2)
            e1.synchronize()
            t_pair = e0.elapsed_time(e1) * 1e-3 / len(sel)
            rte, rre, suc, inl = (r[k].cpu().tolist() for k in ("rte", "rre", "success", "inliers"))
            m['repeatability'] = r["repeatability"].cpu().tolist()
            m['repeatability_refined'] = rep_ref.cpu().tolist()
            for i in range(len(sel)):
                if suc[i]:
                    m['success'].append(1.)
                    m['rte'].append(rte[i])
                    m['rre'].append(rre[i])
                    m['success_inliers'].append(inl[i])
                else:
                    m['success'].append(0.)
                    m['failure_inliers'].append(inl[i])
            if refine:
                rte_r, rre_r, suc_r = (rr[k].cpu().tolist() for k in ("rte", "rre", "success"))
                for i in range(len(sel)):
                    if suc_r[i]:
                        m['rte_refined'].append(rte_r[i])
                        m['rre_refined'].append(rre_r[i])
                        m['success_refined'].append(1.)
                        m['success_inliers_refined'].append(inl[i])
                    else:
                        m['success_refined'].append(0.)
                        m['failure_inliers_refined'].append(inl[i])
        mean_metrics[nk] = {k: (float(np.mean(v)) if len(v) else 0.) for k, v in m.items()}
        mean_metrics[nk]['t_ransac'] = t_pair
        if sel:
            mean_metrics[nk]['t_ransac_sd'] = 0.
    return mean_metrics
