"""Training tuples on the device: from "a sequence of scans with poses" to what TrainStep / EgoNNTrainStep consume.

Mirrors the reference's generators and loaders: datasets/mulran/generate_training_tuples.py (radius search, one ICP per
(anchor, positive) pair), datasets/mulran/generate_evaluation_sets.py + filter_query_elements (datasets/dataset_utils.py:
210-232), the data classes of datasets/base_datasets.py:15-49,86-129, the mask loops of make_collate_fn (:83-88) and
datasets/samplers.py:47-137.  The radius join, the pair masks, the relative poses and the cloud gather run in libegonn_hip
(csrc/tuples.hip); the refinement is `registration.icp_pairs` on clouds that are filtered and downsampled ONCE per scan
(`CloudBank`) instead of once per pair.  File parsing and pose-CSV matching are not here: the entry point is
"poses (n,4,4) float64 + a way to load scan i".  There is no torch or numpy fallback for the device arithmetic."""
from __future__ import annotations

import ctypes
import io
import pickle
import random
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from . import registration as _reg

MAX_POSITIONS = 1 << 24
MAX_RADII = 4
MAX_PICK = 4096
MAX_BATCH = 4096
STATUS_CAPACITY, STATUS_BAD_OFFSETS, STATUS_BAD_INDEX = 1, 2, 4
POSE_BAD_ROW, POSE_SINGULAR, POSE_BAD_INDEX = 1, 2, 4
MULRAN_CROP = (-80., 80., -80., 80., -0.9, None)        # load_pc, generate_training_tuples.py:17-38


# ------------------------------------------------------------------ data classes (datasets/base_datasets.py)
class TrainingTuple:
    """datasets/base_datasets.py:15-32: one element for training / validation"""

    def __init__(self, id: int, timestamp: int, rel_scan_filepath: str, positives: np.ndarray, non_negatives: np.ndarray,
                 pose, positives_poses: Optional[Dict[int, np.ndarray]] = None):
        self.id = id
        self.timestamp = timestamp
        self.rel_scan_filepath = rel_scan_filepath
        self.positives = positives                  # sorted ndarray of positive element ids
        self.non_negatives = non_negatives          # sorted ndarray of element ids
        self.pose = pose                            # (4,4)
        self.positives_poses = positives_poses      # {positive id: (4,4) relative pose refined by ICP}


class EvaluationTuple:
    """datasets/base_datasets.py:35-48"""

    def __init__(self, timestamp: int, rel_scan_filepath: str, position: np.ndarray, pose: Optional[np.ndarray] = None):
        assert position.shape == (2,)
        assert pose is None or pose.shape == (4, 4)
        self.timestamp = timestamp
        self.rel_scan_filepath = rel_scan_filepath
        self.position = position
        self.pose = pose

    def to_tuple(self):
        return self.timestamp, self.rel_scan_filepath, self.position, self.pose


class EvaluationSet:
    """datasets/base_datasets.py:86-129; save / load use its plain-tuple pickle layout, so the files are interchangeable"""

    def __init__(self, query_set: Optional[List[EvaluationTuple]] = None, map_set: Optional[List[EvaluationTuple]] = None):
        self.query_set = query_set
        self.map_set = map_set

    def save(self, pickle_filepath: str):
        with open(pickle_filepath, 'wb') as f:
            pickle.dump([[e.to_tuple() for e in self.query_set], [e.to_tuple() for e in self.map_set]], f)

    def load(self, pickle_filepath: str):
        with open(pickle_filepath, 'rb') as f:
            query_l, map_l = pickle.load(f)
        self.query_set = [EvaluationTuple(e[0], e[1], e[2], e[3]) for e in query_l]
        self.map_set = [EvaluationTuple(e[0], e[1], e[2], e[3]) for e in map_l]

    def _positions(self, s):
        positions = np.zeros((len(s), 2), dtype=s[0].position.dtype)
        for ndx, e in enumerate(s):
            positions[ndx] = e.position
        return positions

    def get_map_positions(self):
        return self._positions(self.map_set)

    def get_query_positions(self):
        return self._positions(self.query_set)


class _TupleUnpickler(pickle.Unpickler):
    """reads the reference's pickles without its modules: datasets.base_datasets.TrainingTuple -> ours"""
    _MAP = {("datasets.base_datasets", "TrainingTuple"): TrainingTuple,
            ("datasets.base_datasets", "EvaluationTuple"): EvaluationTuple}

    def find_class(self, module, name):
        cls = self._MAP.get((module, name))
        return cls if cls is not None else super().find_class(module, name)


def save_training_tuples(path: str, tuples: Dict[int, TrainingTuple]) -> None:
    with open(path, 'wb') as f:
        pickle.dump(tuples, f)


def load_training_tuples(path: str) -> Dict[int, TrainingTuple]:
    """our pickles and the reference's ({ndx: TrainingTuple}, datasets/base_datasets.py:61)"""
    with open(path, 'rb') as f:
        data = f.read()
    tuples = _TupleUnpickler(io.BytesIO(data)).load()
    if not isinstance(tuples, dict) or not all(isinstance(t, TrainingTuple) for t in tuples.values()):
        raise ValueError(f"{path}: not a dictionary of training tuples")
    return tuples


# ------------------------------------------------------------------ argument checks (before any device work)
def _check_xy(name, xy):
    shape = tuple(getattr(xy, "shape", ()))
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError(f"{name}: expected (n, 2) positions, got shape {shape}")
    if shape[0] > MAX_POSITIONS:
        raise ValueError(f"{name}: at most 2^24 positions, got {shape[0]}")


def _check_radii(radius) -> List[float]:
    radii = [float(r) for r in (radius if isinstance(radius, (list, tuple, np.ndarray)) else [radius])]
    if not 1 <= len(radii) <= MAX_RADII:
        raise ValueError(f"radius: 1 to {MAX_RADII} radii per sweep, got {len(radii)}")
    for r in radii:
        if not (np.isfinite(r) and r >= 0.0):
            raise ValueError(f"radius: finite and >= 0 required, got {r}")
    return radii


def _check_exclude(exclude_self, n_radius: int, same: bool) -> List[bool]:
    ex = [bool(e) for e in exclude_self] if isinstance(exclude_self, (list, tuple)) else [bool(exclude_self)] * n_radius
    if len(ex) != n_radius:
        raise ValueError("exclude_self: one flag, or one per radius")
    if any(ex) and not same:
        raise ValueError("exclude_self is defined only when the query positions are the reference positions (ref_xy=None)")
    return ex


# ------------------------------------------------------------------ radius join
def _radius_counts(q, m, radii, ex) -> torch.Tensor:
    lib = _lib.load()
    dev = q.device
    counts = torch.empty((len(radii), q.shape[0]), dtype=torch.int32, device=dev)
    rad = (ctypes.c_double * len(radii))(*radii)
    mask = sum(1 << r for r, e in enumerate(ex) if e)
    _lib.call(dev, lib.egonn_radius_count, q.data_ptr() if q.shape[0] else None, q.shape[0], m.data_ptr() if m.shape[0] else None,
              m.shape[0], rad, len(radii), mask, counts.data_ptr() if q.shape[0] else None)
    return counts


def radius_neighbors(query_xy, ref_xy=None, radius: Union[float, Sequence[float]] = 10., exclude_self=False,
                     check: bool = True):
    """Neighbours of every query position among the reference positions (ref_xy=None: among the queries themselves) within
    each radius: j is a neighbour of i iff dx*dx + dy*dy <= r*r in float64, the rule of sklearn's KDTree.query_radius that
    `find_neighbours_ndx` calls.  radius: one value or up to 4 (one sweep counts them all); exclude_self: one flag or one per
    radius, drops j == i only.  Returns, per radius (a dict for a scalar radius, a list of dicts otherwise),
    {'offsets': int64 (Q+1), 'indices': int32, 'counts': int32 (Q), 'status': int32 ()} as device tensors, every row ascending.
    [SYNC] once: the totals of all radii come back in one copy to size the index buffers (with check=True the status words
    ride on a second copy at the end and a non-zero one raises)."""
    _check_xy("radius_neighbors: query_xy", query_xy)
    if ref_xy is not None:
        _check_xy("radius_neighbors: ref_xy", ref_xy)
    radii = _check_radii(radius)
    ex = _check_exclude(exclude_self, len(radii), ref_xy is None)
    dev = query_xy.device if torch.is_tensor(query_xy) and query_xy.is_cuda else _lib.require_gpu()
    lib = _lib.load()
    q = _lib.as_dev(query_xy, dev, torch.float64)
    m = q if ref_xy is None else _lib.as_dev(ref_xy, dev, torch.float64)
    Q = q.shape[0]
    counts = _radius_counts(q, m, radii, ex)
    offsets = torch.zeros((len(radii), Q + 1), dtype=torch.int64, device=dev)
    offsets[:, 1:] = torch.cumsum(counts, dim=1, dtype=torch.int64)
    totals = offsets[:, -1].tolist()                     # [SYNC] the one host read: sizes of the index buffers
    out = []
    for r, radius_r in enumerate(radii):
        idx = torch.empty((int(totals[r]),), dtype=torch.int32, device=dev)
        status = torch.empty((), dtype=torch.int32, device=dev)
        _lib.call(dev, lib.egonn_radius_fill, q.data_ptr() if Q else None, Q, m.data_ptr() if m.shape[0] else None, m.shape[0],
                  radius_r, int(ex[r]), offsets[r].data_ptr(), idx.data_ptr() if idx.numel() else None, idx.numel(),
                  status.data_ptr())
        out.append({"offsets": offsets[r], "indices": idx, "counts": counts[r], "status": status, "_keep": (q, m)})
    if check:
        bad = torch.stack([o["status"] for o in out]).tolist()
        if any(bad):
            raise _lib.EgonnError(f"radius_neighbors: device status {bad} (1 = capacity, 2 = offsets)", 5)
    return out if isinstance(radius, (list, tuple, np.ndarray)) else out[0]


def count_within(query_xy, ref_xy, radius: float) -> torch.Tensor:
    """(Q,) int32 on the device: reference positions within `radius` of every query (query_radius(..., count_only=True)).
    No host synchronisation when the positions are device tensors."""
    _check_xy("count_within: query_xy", query_xy)
    _check_xy("count_within: ref_xy", ref_xy)
    radii = _check_radii(radius)
    if len(radii) != 1:
        raise ValueError("count_within: one radius")
    dev = query_xy.device if torch.is_tensor(query_xy) and query_xy.is_cuda else _lib.require_gpu()
    return _radius_counts(_lib.as_dev(query_xy, dev, torch.float64), _lib.as_dev(ref_xy, dev, torch.float64), radii, [False])[0]


# ------------------------------------------------------------------ relative poses
def _check_poses(name, poses):
    shape = tuple(getattr(poses, "shape", ()))
    if len(shape) != 3 or shape[1:] != (4, 4):
        raise ValueError(f"{name}: expected (n, 4, 4) poses, got shape {shape}")


def relative_poses(poses, idx_a, idx_b, negate_translation: bool = True, return_status: bool = False):
    """out[p] = inv(poses[idx_b[p]]) @ poses[idx_a[p]] as the affine inverse with the translation difference taken first
    (csrc/tuples.hip): the pose of a in the frame of b.  negate_translation=True is datasets/mulran/utils.py:relative_pose
    (its "fix" negates the translation), False is misc/poses.py:relative_pose.  Returns (P,4,4) float64 on the device, with
    return_status also (P,) int32 of POSE_* bits (a flagged pair is the identity).  No host synchronisation when the
    arguments are device tensors."""
    _check_poses("relative_poses", poses)
    la, lb = tuple(getattr(idx_a, "shape", (len(idx_a),))), tuple(getattr(idx_b, "shape", (len(idx_b),)))
    if len(la) != 1 or la != lb:
        raise ValueError(f"relative_poses: idx_a and idx_b must be 1-D and equally long, got {la} and {lb}")
    dev = poses.device if torch.is_tensor(poses) and poses.is_cuda else _lib.require_gpu()
    lib = _lib.load()
    ps, a, b = _lib.as_dev(poses, dev, torch.float64), _lib.as_dev(idx_a, dev, torch.int32), _lib.as_dev(idx_b, dev, torch.int32)
    P = a.shape[0]
    out = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    status = torch.empty((P,), dtype=torch.int32, device=dev)
    _lib.call(dev, lib.egonn_relative_poses, ps.data_ptr() if ps.shape[0] else None, ps.shape[0], _lib._ptr(a) if P else None,
              _lib._ptr(b) if P else None, P, int(bool(negate_translation)), out.data_ptr() if P else None,
              status.data_ptr() if P else None)
    return (out, status) if return_status else out


# ------------------------------------------------------------------ resident downsampled clouds
class CloudBank:
    """Every scan's ICP cloud, resident on the device ONCE: `add` runs load_pc (generate_training_tuples.py:17-38: all-zero
    returns dropped, crop) and the voxel downsample that `icp` (misc/point_clouds.py:31-62) applies to both sides, per scan
    instead of per pair; `gather` lines picked clouds up as `icp_pairs` takes them."""

    def __init__(self, crop=MULRAN_CROP, voxel_size: float = _reg.ICP_VOXEL_SIZE, chunk_points: int = 4_000_000, device=None):
        if not float(voxel_size) > 0.0:
            raise ValueError("CloudBank: voxel_size must be positive")
        _reg._check_crop(crop)
        if int(chunk_points) < 1:
            raise ValueError("CloudBank: chunk_points must be positive")
        self.crop, self.voxel_size, self.chunk_points = crop, float(voxel_size), int(chunk_points)
        self.device = device
        self.points: Optional[torch.Tensor] = None        # (capacity, 3) f64, the first sizes-sum rows valid
        self.host_offsets: List[int] = [0]
        self.status: List[int] = []                        # ICP_RANGE per cloud whose voxel index left 21 bits
        self._offsets_dev: Optional[torch.Tensor] = None

    def __len__(self):
        return len(self.host_offsets) - 1

    @property
    def n_points(self) -> int:
        return self.host_offsets[-1]

    def sizes(self) -> np.ndarray:
        return np.diff(np.asarray(self.host_offsets, dtype=np.int64))

    def _dev(self):
        if self.device is None:
            self.device = _lib.require_gpu()
        return self.device

    def _grow(self, rows: int):
        """room for `rows` more points; the buffer grows by half its size at least, so a scan is copied O(1) times"""
        need = self.n_points + rows
        have = 0 if self.points is None else self.points.shape[0]
        if need <= have:
            return
        cap = max(need, have + have // 2)
        try:
            new = torch.empty((cap, 3), dtype=torch.float64, device=self._dev())
        except torch.cuda.OutOfMemoryError as e:
            raise MemoryError(f"CloudBank: a bank of {cap} points needs {cap * 24} bytes of device memory next to the "
                              f"{have * 24} it holds; split the scans by sequence") from e
        if self.points is not None and self.n_points:
            new[: self.n_points] = self.points[: self.n_points]
        self.points = new

    def _add_chunk(self, raws: List[np.ndarray]):
        lib = _lib.load()
        dev = self._dev()
        stride = raws[0].shape[1]
        off = np.zeros(len(raws) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(r) for r in raws])
        n, B = int(off[-1]), len(raws)
        raw = torch.from_numpy(np.concatenate(raws) if n else np.zeros((0, stride), np.float32)).to(dev)
        raw_off = torch.from_numpy(off).to(dev)
        pts = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
        pts_off = torch.empty(B + 1, dtype=torch.int64, device=dev)
        scratch = torch.empty(lib.egonn_filter_points_scratch_ints(n), dtype=torch.int32, device=dev)
        # zero-point removal only: the ground cut of load_pc is the crop's min_z, applied by the downsample
        _lib.call(dev, lib.egonn_filter_points, raw.data_ptr() if n else None, n, stride, raw_off.data_ptr(), B, 1, 0, 0.0,
                  pts.data_ptr(), pts_off.data_ptr(), scratch.data_ptr(), scratch.numel())
        ds = _reg.voxel_downsample(pts[:n] if n else pts[:0], pts_off, self.voxel_size, self.crop)
        host = torch.cat([ds["offsets"], ds["status"].to(torch.int64)]).tolist()       # [SYNC] one copy per chunk
        ds_off, st = host[: B + 1], host[B + 1:]
        self._grow(ds_off[-1])
        base = self.n_points
        if ds_off[-1]:
            self.points[base: base + ds_off[-1]] = ds["points"][: ds_off[-1]]
        self.host_offsets += [base + o for o in ds_off[1:]]
        self.status += [int(s) for s in st]
        self._offsets_dev = None

    def add(self, scans: Sequence[np.ndarray]) -> "CloudBank":
        """raw scans (n, 3 | 4) float32 in order; one [SYNC] per chunk of about `chunk_points` raw points (the downsampled
        sizes come back to place the chunk in the bank)."""
        raws = []
        for s in scans:
            a = np.ascontiguousarray(s.cpu().numpy() if torch.is_tensor(s) else s, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] not in (3, 4):
                raise ValueError(f"CloudBank.add: a scan is (n, 3 | 4) float32, got shape {a.shape}")
            raws.append(a)
        if raws and any(r.shape[1] != raws[0].shape[1] for r in raws):
            raise ValueError("CloudBank.add: scans of one call have the same number of columns")
        chunk, rows = [], 0
        for r in raws:
            if chunk and (rows + len(r) > self.chunk_points or len(chunk) >= MAX_BATCH):
                self._add_chunk(chunk)
                chunk, rows = [], 0
            chunk.append(r)
            rows += len(r)
        if chunk:
            self._add_chunk(chunk)
        return self

    def offsets(self) -> torch.Tensor:
        if self._offsets_dev is None:
            self._offsets_dev = torch.tensor(self.host_offsets, dtype=torch.int64).to(self._dev())
        return self._offsets_dev

    def cloud(self, i: int) -> torch.Tensor:
        return self.points[self.host_offsets[i]: self.host_offsets[i + 1]]

    def gather(self, pick, capacity: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """clouds pick[0..n) back to back: {'points': (capacity,3) f64, 'offsets': (n+1,) int64, 'status': int32 ()} on the
        device.  capacity=None sizes the output exactly from the host copy of the bank's offsets (host picks only); no host
        synchronisation either way."""
        n_pick = len(pick)
        if not 1 <= n_pick <= MAX_PICK:
            raise ValueError(f"CloudBank.gather: 1 to {MAX_PICK} picks per call, got {n_pick}")
        if capacity is None:
            if torch.is_tensor(pick) and pick.is_cuda:
                raise ValueError("CloudBank.gather: device picks need an explicit capacity")
            p = np.asarray(pick, dtype=np.int64)
            if p.size and (p.min() < 0 or p.max() >= len(self)):
                raise ValueError(f"CloudBank.gather: pick outside [0, {len(self)})")
            capacity = int(self.sizes()[p].sum())
        if int(capacity) < 0:
            raise ValueError("CloudBank.gather: negative capacity")
        lib = _lib.load()
        dev = self._dev()
        pk = _lib.as_dev(pick, dev, torch.int32)
        out = torch.empty((max(int(capacity), 1), 3), dtype=torch.float64, device=dev)
        off = torch.empty((n_pick + 1,), dtype=torch.int64, device=dev)
        status = torch.empty((), dtype=torch.int32, device=dev)
        _lib.call(dev, lib.egonn_gather_clouds, _lib._ptr(self.points) if self.n_points else None, self.n_points,
                  self.offsets().data_ptr(), len(self), pk.data_ptr(), n_pick, out.data_ptr(), int(capacity), off.data_ptr(),
                  status.data_ptr())
        return {"points": out[: int(capacity)], "offsets": off, "status": status, "_keep": (pk, out)}


# ------------------------------------------------------------------ the generator
def _csr_to_host(nb) -> Tuple[np.ndarray, np.ndarray]:
    return nb["offsets"].cpu().numpy(), nb["indices"].cpu().numpy()


def generate_training_tuples(poses, scans, pos_threshold: float = 2., neg_threshold: float = 10., refine: bool = True,
                             pairs_per_call: int = 16, negate_translation: bool = True, inlier_dist_threshold: float = 1.2,
                             max_iteration: int = 200, timestamps=None, rel_scan_filepaths=None, point2plane: bool = False,
                             knn: int = 20):
    """datasets/mulran/generate_training_tuples.py:41-100 for poses (n,4,4) float64 and scans = a `CloudBank` that holds the n
    scans, or a callable i -> (n_i, 3 | 4) float32 raw scan (a bank is then filled from it).  positives: other scans within
    pos_threshold of the anchor's (x, y) = poses[:, :2, 3]; non_negatives: scans within neg_threshold, the anchor included;
    both sorted int32.  refine=True: for every (anchor i, positive j) in tuple order, in chunks of pairs_per_call,
    positives_poses[j] = ICP(cloud i -> cloud j) started at relative_poses(i, j); refine=False: that start itself (the
    reference's DEBUG branch).  Returns ({ndx: TrainingTuple}, stats): stats has 'pairs', 'fitness' / 'inlier_rmse' as
    {'min', 'mean', 'max'} (1. without refinement, as the reference reports), 'status_counts' {ICP status: pairs} and
    'pose_status_counts'.  T, fitness, rmse and status of all pairs come back in ONE device-to-host copy at the end.
    point2plane: the point-to-plane estimator, on normals of each chunk's gathered target clouds (`estimate_normals`, knn
    neighbours); the normals of a cloud do not depend on the chunk it is gathered into."""
    _check_poses("generate_training_tuples", poses)
    n = int(poses.shape[0])
    if not 1 <= int(pairs_per_call) <= MAX_BATCH:
        raise ValueError(f"generate_training_tuples: pairs_per_call in [1, {MAX_BATCH}]")
    radii = _check_radii([pos_threshold, neg_threshold])
    for name, v in (("timestamps", timestamps), ("rel_scan_filepaths", rel_scan_filepaths)):
        if v is not None and len(v) != n:
            raise ValueError(f"generate_training_tuples: {name} must have one entry per pose")
    if refine and not isinstance(scans, CloudBank) and not callable(scans):
        raise ValueError("generate_training_tuples: scans is a CloudBank or a callable i -> raw scan")
    if refine and isinstance(scans, CloudBank) and len(scans) != n:
        raise ValueError(f"generate_training_tuples: the bank holds {len(scans)} scans for {n} poses")
    dev = _lib.require_gpu()
    poses_np = np.ascontiguousarray(poses.cpu().numpy() if torch.is_tensor(poses) else poses, dtype=np.float64)
    poses_dev = torch.from_numpy(poses_np).to(dev)
    xy = poses_dev[:, :2, 3].contiguous()
    nb_pos, nb_non = radius_neighbors(xy, None, radii, exclude_self=[True, False])
    pos_off, pos_idx = _csr_to_host(nb_pos)
    non_off, non_idx = _csr_to_host(nb_non)
    n_pairs = int(pos_off[-1])
    idx_a = np.repeat(np.arange(n, dtype=np.int32), np.diff(pos_off))      # anchors, tuple order
    idx_b = pos_idx                                                         # their positives, ascending
    result = torch.zeros((max(n_pairs, 1), 19), dtype=torch.float64, device=dev)     # T (16), fitness, rmse, status
    pose_status = None
    if n_pairs:
        T_init, pose_status = relative_poses(poses_dev, idx_a, idx_b, negate_translation, return_status=True)
        result[:, :16] = T_init.reshape(n_pairs, 16)
        result[:, 16:18] = 1.0
    if refine and n_pairs:
        bank = scans
        if not isinstance(bank, CloudBank):
            bank = CloudBank().add([scans(i) for i in range(n)])
        for lo in range(0, n_pairs, int(pairs_per_call)):
            hi = min(lo + int(pairs_per_call), n_pairs)
            src, tgt = bank.gather(idx_a[lo:hi]), bank.gather(idx_b[lo:hi])
            nrm = _reg.estimate_normals(tgt["points"], tgt["offsets"], knn)["normals"] if point2plane else None
            r = _reg.icp_pairs(src["points"], src["offsets"], tgt["points"], tgt["offsets"], T_init[lo:hi],
                               inlier_dist_threshold, max_iteration, tgt_normals=nrm)
            result[lo:hi, :16] = r["T"].reshape(hi - lo, 16)
            result[lo:hi, 16] = r["fitness"]
            result[lo:hi, 17] = r["inlier_rmse"]
            result[lo:hi, 18] = r["status"].to(torch.float64)
    host = result.cpu().numpy()                          # the one copy back
    T = host[:n_pairs, :16].reshape(n_pairs, 4, 4)
    fitness, rmse, status = host[:n_pairs, 16], host[:n_pairs, 17], host[:n_pairs, 18].astype(np.int64)
    tuples = {}
    for i in range(n):
        p = pos_idx[pos_off[i]: pos_off[i + 1]].copy()
        tuples[i] = TrainingTuple(id=i, timestamp=i if timestamps is None else timestamps[i],
                                  rel_scan_filepath="" if rel_scan_filepaths is None else rel_scan_filepaths[i], positives=p,
                                  non_negatives=non_idx[non_off[i]: non_off[i + 1]].copy(), pose=poses_np[i],
                                  positives_poses={int(j): T[pos_off[i] + k].copy() for k, j in enumerate(p)})
    mmm = lambda v: {"min": float(v.min()), "mean": float(v.mean()), "max": float(v.max())} if len(v) else None   # noqa: E731
    uniq = lambda v: {int(k): int(c) for k, c in zip(*np.unique(v, return_counts=True))}                            # noqa: E731
    stats = {"pairs": n_pairs, "fitness": mmm(fitness), "inlier_rmse": mmm(rmse), "status_counts": uniq(status),
             "pose_status_counts": uniq(pose_status.cpu().numpy()) if pose_status is not None else {},
             "fitness_per_pair": fitness, "inlier_rmse_per_pair": rmse, "status_per_pair": status}
    return tuples, stats


# ------------------------------------------------------------------ evaluation sets
def filter_query_elements(query_set: List[EvaluationTuple], map_set: List[EvaluationTuple],
                          dist_threshold: float) -> List[EvaluationTuple]:
    """datasets/dataset_utils.py:210-232: the query elements with a map element within dist_threshold.  Map positions are
    rounded to float32 first, as the reference's `map_pos` array does; query positions stay float64."""
    radii = _check_radii(dist_threshold)
    if not query_set:
        return []
    map_pos = np.zeros((len(map_set), 2), dtype=np.float32)
    for ndx, e in enumerate(map_set):
        map_pos[ndx] = e.position
    query_pos = np.stack([np.asarray(e.position, dtype=np.float64).reshape(2) for e in query_set])
    counts = count_within(query_pos, map_pos.astype(np.float64), radii[0]).cpu().numpy()
    return [e for e, c in zip(query_set, counts) if c > 0]


def generate_evaluation_set(map_set: List[EvaluationTuple], query_set: List[EvaluationTuple],
                            dist_threshold: float = 20.) -> EvaluationSet:
    """datasets/mulran/generate_evaluation_sets.py:25-38 downstream of the sequence readers"""
    return EvaluationSet(filter_query_elements(query_set, map_set, dist_threshold), map_set)


# ------------------------------------------------------------------ masks of a batch
class TupleIndex:
    """the positives / non-negatives of {ndx: TrainingTuple} as two CSR tables resident on the device; `masks(labels)` is the
    double loop of make_collate_fn (datasets/dataset_utils.py:83-88) in one launch.  Tuple ids must be 0..n-1."""

    def __init__(self, tuples: Dict[int, TrainingTuple], device=None):
        n = len(tuples)
        if sorted(tuples) != list(range(n)):
            raise ValueError("TupleIndex: tuple ids must be the consecutive numbers 0..n-1")
        self.n_tuples = n
        self._host = {}
        for name in ("positives", "non_negatives"):
            rows = [np.asarray(getattr(tuples[i], name), dtype=np.int32).reshape(-1) for i in range(n)]
            for i, r in enumerate(rows):
                if r.size > 1 and not (np.diff(r) > 0).all():
                    raise ValueError(f"TupleIndex: {name} of tuple {i} are not sorted ascending")
            off = np.zeros(n + 1, dtype=np.int64)
            off[1:] = np.cumsum([r.size for r in rows])
            self._host[name] = (off, np.concatenate(rows) if rows else np.zeros(0, np.int32))
        self.device = device
        self._dev = None

    def _tables(self):
        if self._dev is None:
            dev = self.device if self.device is not None else _lib.require_gpu()
            self.device = dev
            self._dev = {k: (torch.from_numpy(o).to(dev), torch.from_numpy(np.ascontiguousarray(i, np.int32)).to(dev))
                         for k, (o, i) in self._host.items()}
        return self._dev

    def masks_u8(self, labels, out=None):
        """-> (positives_mask, negatives_mask, status): (B,B) uint8 0/1 and int32 () on the device.  With device labels and
        `out` = the three tensors of an earlier call, nothing is allocated: the call can be captured into a graph."""
        B = int(labels.shape[0]) if hasattr(labels, "shape") else len(labels)
        if not 1 <= B <= MAX_BATCH:
            raise ValueError(f"TupleIndex.masks: batch size in [1, {MAX_BATCH}], got {B}")
        t = self._tables()
        dev = self.device
        lab = _lib.as_dev(labels, dev, torch.int32)
        if lab.dim() != 1:
            raise ValueError("TupleIndex.masks: labels are 1-D")
        if out is None:
            out = (torch.empty((B, B), dtype=torch.uint8, device=dev), torch.empty((B, B), dtype=torch.uint8, device=dev),
                   torch.empty((), dtype=torch.int32, device=dev))
        pm, nm, status = out
        (po, pi), (no, ni) = t["positives"], t["non_negatives"]
        _lib.call(dev, _lib.load().egonn_pair_masks, lab.data_ptr(), B, po.data_ptr(), pi.data_ptr() if pi.numel() else None,
                  pi.numel(), no.data_ptr(), ni.data_ptr() if ni.numel() else None, ni.numel(), self.n_tuples, pm.data_ptr(),
                  nm.data_ptr(), status.data_ptr())
        return pm, nm, status

    def masks(self, labels):
        """(positives_mask, negatives_mask) as torch.bool (B,B) on the device, no host synchronisation.  A label outside the
        tuples gives an all-False row and column (the status word of `masks_u8` tells)."""
        pm, nm, _ = self.masks_u8(labels)
        return pm.view(torch.bool), nm.view(torch.bool)


# ------------------------------------------------------------------ sampler (host)
class BatchSampler:
    """datasets/samplers.py:47-137 on {ndx: TrainingTuple}: batches of groups of k = 2 similar elements
    [a1, p1, a2, p2, ...].  An element is drawn among the unused ones; its partner is an unused positive if one exists, else
    any positive; elements without positives are skipped; a batch is flushed at batch_size or when the elements run out,
    and only if it holds >= 4 elements.  Seeded by its own random.Random(seed) (epoch e draws from seed + e), regenerated
    per __iter__; the draw sequence is not the reference's (that one rides on the global `random` state)."""

    def __init__(self, tuples: Dict[int, TrainingTuple], batch_size: int, batch_size_limit: Optional[int] = None,
                 batch_expansion_rate: Optional[float] = None, max_batches: Optional[int] = None, seed: int = 0):
        if batch_expansion_rate is not None:
            if not batch_expansion_rate > 1.:
                raise ValueError("batch_expansion_rate must be greater than 1")
            if batch_size_limit is None or batch_size > batch_size_limit:
                raise ValueError("batch_size_limit must be greater or equal to batch_size")
        self.k = 2
        self.batch_size = max(int(batch_size), 2 * self.k)
        self.batch_size_limit, self.batch_expansion_rate, self.max_batches = batch_size_limit, batch_expansion_rate, max_batches
        self.tuples = tuples
        self.elems_ndx = list(tuples)
        self.seed, self.epoch = int(seed), 0
        self.batch_idx: List[List[int]] = []

    def __iter__(self):
        self.generate_batches()
        for batch in self.batch_idx:
            yield batch

    def __len__(self):
        return len(self.batch_idx)

    def expand_batch(self):
        if self.batch_expansion_rate is None or self.batch_size >= self.batch_size_limit:
            return
        self.batch_size = min(int(self.batch_size * self.batch_expansion_rate), self.batch_size_limit)

    def generate_batches(self):
        rng = random.Random(self.seed + self.epoch)
        self.epoch += 1
        self.batch_idx = []
        items = list(self.elems_ndx)                       # unused elements: O(1) removal by swapping with the last
        where = {e: i for i, e in enumerate(items)}

        def remove(e):
            i = where.pop(e)
            last = items.pop()
            if i != len(items):
                items[i] = last
                where[last] = i
        batch: List[int] = []
        while True:
            if len(batch) >= self.batch_size or not items:
                if len(batch) >= 2 * self.k:
                    self.batch_idx.append(batch)
                    batch = []
                    if self.max_batches is not None and len(self.batch_idx) >= self.max_batches:
                        break
                if not items:
                    break
            first = items[rng.randrange(len(items))]
            remove(first)
            positives = [int(e) for e in self.tuples[first].positives]
            if not positives:
                continue
            unused = [e for e in positives if e in where]
            if unused:
                second = unused[rng.randrange(len(unused))]
                remove(second)
            else:
                second = positives[rng.randrange(len(positives))]
            batch += [first, second]


# ------------------------------------------------------------------ the glue
class TrainingSet:
    """tuples + scans -> the arguments of TrainStep / EgoNNTrainStep, one sampled batch at a time.

    load_scan: i -> (n_i, 3) float32 points of scan i (a numpy array or a tensor; already filtered, e.g. by ScanIngest).
    Iterating yields (batch, positives_mask, negatives_mask, local_batch):
      batch         TrainBatcher.__call__ on the batch's scans (augmentation, quantiser), scan ids = the labels
      masks         TupleIndex.masks(labels): torch.bool (B,B) on the device
      local_batch   with local=True, TrainBatcher.local on the sampler's groups: anchor = element 2g, positive = element
                    2g+1 (a positive of the anchor by construction), T_gt from tuples[anchor].positives_poses[positive]
                    (the perturbation of the batcher's RigidPerturbation composed on top); None with local=False."""

    def __init__(self, tuples: Dict[int, TrainingTuple], load_scan: Callable[[int], np.ndarray], batcher, sampler,
                 local: bool = True):
        self.tuples, self.load_scan, self.batcher, self.sampler, self.local = tuples, load_scan, batcher, sampler, local
        self.index = TupleIndex(tuples)
        self.draw = 0

    def _points(self, ids, dev):
        clouds = [torch.as_tensor(self.load_scan(int(i))).to(device=dev, dtype=torch.float32)[:, :3] for i in ids]
        off = np.zeros(len(clouds) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(c) for c in clouds])
        return torch.cat(clouds).contiguous(), off

    def collate(self, labels: Sequence[int]):
        dev = _lib.require_gpu()
        labels = [int(e) for e in labels]
        pts, off = self._points(labels, dev)
        draw = self.draw
        self.draw += 1
        batch = self.batcher(pts, off, labels, draw=draw, set_id=draw)
        pos_mask, neg_mask = self.index.masks(labels)
        local_batch = None
        if self.local:
            anchors, positives = labels[0::2], labels[1::2]
            T = np.stack([np.asarray(self.tuples[a].positives_poses[p], dtype=np.float64) for a, p in zip(anchors, positives)])
            a_pts, a_off = self._points(anchors, dev)
            p_pts, p_off = self._points(positives, dev)
            local_batch = self.batcher.local(a_pts, a_off, p_pts, p_off, positives, torch.from_numpy(T).float(), draw=draw)
        return batch, pos_mask, neg_mask, local_batch

    def __iter__(self):
        for labels in self.sampler:
            yield self.collate(labels)
