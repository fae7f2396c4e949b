"""A resident global voxel map (csrc/voxel_map.hip): fuse the clouds of a `CloudBank` under a trajectory's
poses into one map, grow it batch by batch, crop submaps out of it, and refine a scan's pose against it.

A voxel record is (key, integer sums of the points' residuals, point count, observation count).  The sums are integers, so
`insert` in any number of batches and in any order gives, bit for bit, the records of one call.  The centroid of a voxel is
its output point; `observations` (how many scans put a point there) is the one filter against dynamic objects.  There is no
torch or numpy fallback for the device arithmetic.

`NDTMap` is the NDT layer over a map's keys (csrc/ndt.hip): exact integer second moments per voxel, one
Gaussian per voxel (mean, information matrix, eigenvalues, normal), and scan-to-map registration against them, which needs
no submap, no per-call grid and no sort.  `refine_against_map(method="ndt")` and `Relocalizer(ndt_map=...)` run on it.

A map can give observations back: `remove` integrates them again and subtracts, exactly; with `track=True`
the map keeps a host ledger of what it holds and `repose` re-fuses the scans a pose-graph correction moved.  With
`moments=True` the records carry the NDT moments, `NDTMap.from_map` / `NDTMap.update` snapshot them and `build_ndt_map(...,
moments=True)` reads every point once.

Not here: cutting the sort's 63 key bits by a known extent, a device-side ledger, a `finalize` of only the touched rows, the
full Newton step of the NDT score with a line search, and distribution-to-distribution NDT."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from . import registration as _reg

MAX_OBS = 4096
MAX_BOXES = 4096
STATUS_RANGE, STATUS_CAPACITY, STATUS_BAD_INDEX, STATUS_MISMATCH = 1, 2, 4, 8
_FIELDS = ("keys", "sums", "count", "obs")
_MOMENTS = ("s1", "s2")


def _check_poses(name, poses, n=None):
    shape = tuple(getattr(poses, "shape", ()))
    if len(shape) != 3 or shape[1:] != (4, 4) or (n is not None and shape[0] != n):
        want = "(n, 4, 4)" if n is None else f"({n}, 4, 4)"
        raise ValueError(f"{name}: expected {want} poses, got shape {shape}")


def _check_filters(name, min_count, min_observations):
    if int(min_count) < 1 or int(min_observations) < 1:
        raise ValueError(f"{name}: min_count and min_observations are at least 1")


def _check_boxes(name, centers, half_extent) -> np.ndarray:
    """-> half extents (3,) float64"""
    shape = tuple(getattr(centers, "shape", ()))
    if len(shape) != 2 or shape[1] != 3 or not 1 <= shape[0] <= MAX_BOXES:
        raise ValueError(f"{name}: centers must be (n, 3) with 1 <= n <= {MAX_BOXES}, got shape {shape}")
    try:
        half = np.broadcast_to(np.asarray(half_extent, dtype=np.float64), (3,))
    except ValueError:
        half = None
    if half is None or not (np.isfinite(half).all() and (half > 0).all()):
        raise ValueError(f"{name}: half_extent is one positive finite number or three")
    return np.array(half, dtype=np.float64)          # a writable copy: torch.from_numpy wants one


def _records(rows: int, dev, moments: bool = False) -> Dict[str, torch.Tensor]:
    rows = max(int(rows), 1)
    r = {"keys": torch.empty((rows,), dtype=torch.int64, device=dev), "sums": torch.empty((rows, 3), dtype=torch.int64, device=dev),
         "count": torch.empty((rows,), dtype=torch.int32, device=dev), "obs": torch.empty((rows,), dtype=torch.int32, device=dev),
         "n": torch.zeros((), dtype=torch.int64, device=dev)}
    if moments:
        r["s1"] = torch.empty((rows, 3), dtype=torch.int64, device=dev)
        r["s2"] = torch.empty((rows, 6), dtype=torch.int64, device=dev)
    return r


def _rec_ptrs(r):
    return r["keys"].data_ptr(), r["sums"].data_ptr(), r["count"].data_ptr(), r["obs"].data_ptr()


def _mrec_ptrs(r):
    """the six arrays of a record set for the `_moments` entry points and subtract; s1 / s2 null without moments"""
    return _rec_ptrs(r) + (_lib._ptr(r.get("s1")), _lib._ptr(r.get("s2")))


def _scratch256(nbytes: int, dev) -> torch.Tensor:
    """scratch for the voxel-map calls: they want 256-byte alignment, which a fresh allocation of the caching allocator has"""
    s = _lib.scratch(nbytes, dev)
    assert s.data_ptr() % 256 == 0
    return s


class VoxelMap:
    """The map: `voxel_size` (0.2 m by default: twice the bank's 0.1 m downsample, so a surface seen by one scan fills its
    voxels), `origin` (3 floats; None = the translation of the first pose inserted, read on the host) and up to 2^21 voxels per
    axis around it.  capacity=None: the record buffers grow as needed and `insert` takes one [SYNC] per chunk to size them, as
    `CloudBank.add` does.  capacity=rows reserves two record buffers of that size: `insert` then has no host synchronisation
    (device picks and poses, explicit points_capacity) and can be captured; a chunk that would overflow is dropped whole and
    sets STATUS_CAPACITY, the map keeps what it holds.
    moments=True: the records carry the NDT layer's integer moments (`records` gains 's1' (rows,3) and 's2' (rows,6) int64;
    `NDTMap.from_map` reads them).  track=True: the map keeps a host `ledger` of the (pick, pose) it holds, which `remove`
    checks and `repose` needs; it takes host picks and host poses."""

    def __init__(self, voxel_size: float = 0.2, origin=None, capacity: Optional[int] = None, device=None,
                 chunk_points: int = 4_000_000, moments: bool = False, track: bool = False):
        v = float(voxel_size)
        if not (v > 0.0 and np.isfinite(v)):
            raise ValueError("VoxelMap: voxel_size must be positive and finite")
        if origin is not None:
            origin = np.asarray(origin, dtype=np.float64)
            if origin.shape != (3,) or not np.isfinite(origin).all():
                raise ValueError("VoxelMap: origin is three finite numbers")
        if capacity is not None and not 1 <= int(capacity) < 2 ** 31:
            raise ValueError("VoxelMap: capacity in [1, 2^31)")
        if int(chunk_points) < 1:
            raise ValueError("VoxelMap: chunk_points must be positive")
        self.voxel_size, self.origin, self.capacity = v, origin, None if capacity is None else int(capacity)
        self.device, self.chunk_points = device, int(chunk_points)
        self.moments, self.track = bool(moments), bool(track)
        self._ledger_pick, self._ledger_pose = [], []        # what the map holds, in insertion order (track=True)
        self._buf = [None, None]          # ping-pong record buffers
        self._cur = 0
        self._status = None
        self._work = {}                   # (points_capacity, n_obs) -> chunk records and scratch, kept for replays

    # ------------------------------------------------------------------ state
    def _dev(self):
        if self.device is None:
            self.device = _lib.require_gpu()
        return self.device

    def _ensure(self):
        if self._status is None:
            dev = self._dev()
            self._status = torch.zeros((), dtype=torch.int32, device=dev)
            rows = self.capacity if self.capacity is not None else 1
            self._buf = [_records(rows, dev, self.moments), _records(rows, dev, self.moments)]

    def _origin_c(self):
        return (ctypes.c_double * 3)(*[float(v) for v in self.origin])

    @property
    def records(self) -> Dict[str, torch.Tensor]:
        """the live buffer: keys (rows) int64 (the 63-bit key), sums (rows,3) int64, count, obs (rows) int32, n () int64; with
        moments s1 (rows,3) and s2 (rows,6) int64"""
        self._ensure()
        return self._buf[self._cur]

    @property
    def n_voxels(self) -> int:
        """[SYNC]"""
        return 0 if self._status is None else int(self.records["n"].item())

    @property
    def status(self) -> int:
        """[SYNC] OR of the STATUS_* bits of every call so far"""
        return 0 if self._status is None else int(self._status.item())

    @property
    def ledger(self):
        """(pick (n,) int32, poses (n,4,4) float64) of the observations the map holds, in insertion order (track=True)"""
        n = len(self._ledger_pick)
        return (np.asarray(self._ledger_pick, dtype=np.int32).reshape(n),
                np.asarray(self._ledger_pose, dtype=np.float64).reshape(n, 4, 4))

    def clear(self) -> "VoxelMap":
        """empty map, status 0, empty ledger, buffers kept"""
        self._ledger_pick, self._ledger_pose = [], []
        if self._status is not None:
            self._cur = 0
            self._buf[0]["n"].zero_()
            self._status.zero_()
        return self

    # ------------------------------------------------------------------ insert
    def _chunk(self, bank, pk, ps, n_obs: int, points_capacity: int, subtract: bool = False):
        lib = _lib.load()
        dev = self._dev()
        key = (int(points_capacity), int(n_obs))
        work = self._work.get(key)
        if work is None:
            work = {"rec": _records(points_capacity, dev, self.moments),
                    "s_int": _scratch256(lib.egonn_voxel_map_integrate_scratch_bytes(points_capacity, n_obs), dev)}
            if self.capacity is not None:
                self._work[key] = work
        chunk = work["rec"]
        rows_c = max(int(points_capacity), 1)
        n_bank = bank.n_points
        if self.moments:                 # the scratch is integrate's (egonn_voxel_map_integrate_moments_scratch_bytes)
            _lib.call(dev, lib.egonn_voxel_map_integrate_moments, _lib._ptr(bank.points) if n_bank else None, n_bank,
                      bank.offsets().data_ptr(), len(bank), pk.data_ptr(), ps.data_ptr(), n_obs, self._origin_c(), self.voxel_size,
                      int(points_capacity), *_mrec_ptrs(chunk), rows_c, chunk["n"].data_ptr(), self._status.data_ptr(),
                      work["s_int"].data_ptr(), work["s_int"].numel() * 8)
        else:
            _lib.call(dev, lib.egonn_voxel_map_integrate, _lib._ptr(bank.points) if n_bank else None, n_bank, bank.offsets().data_ptr(),
                      len(bank), pk.data_ptr(), ps.data_ptr(), n_obs, self._origin_c(), self.voxel_size, int(points_capacity),
                      *_rec_ptrs(chunk), rows_c, chunk["n"].data_ptr(), self._status.data_ptr(), work["s_int"].data_ptr(),
                      work["s_int"].numel() * 8)
        A = self._buf[self._cur]
        rows_a = A["keys"].shape[0]
        if subtract:                     # out = A - chunk: never more rows than A has
            out = self._buf[1 - self._cur]
            if out["keys"].shape[0] < rows_a:
                out = self._buf[1 - self._cur] = _records(rows_a, dev, self.moments)
            rows_o = out["keys"].shape[0]
            skey = ("subtract", rows_a, rows_c, rows_o)
            s_sub = self._work.get(skey)
            if s_sub is None:
                s_sub = _scratch256(lib.egonn_voxel_map_subtract_scratch_bytes(rows_a, rows_c, rows_o), dev)
                if self.capacity is not None:
                    self._work[skey] = s_sub
            _lib.call(dev, lib.egonn_voxel_map_subtract, *_mrec_ptrs(A), A["n"].data_ptr(), rows_a, *_mrec_ptrs(chunk),
                      chunk["n"].data_ptr(), rows_c, *_mrec_ptrs(out), rows_o, out["n"].data_ptr(), self._status.data_ptr(),
                      s_sub.data_ptr(), s_sub.numel() * 8)
            out["_keep"] = (chunk, work, s_sub, pk, ps)
            self._cur = 1 - self._cur
            return
        if self.capacity is None:
            n_a, n_c = torch.stack([A["n"], chunk["n"]]).tolist()            # [SYNC] one copy per chunk: sizes the next buffer
            need = n_a + n_c
            out = self._buf[1 - self._cur]
            if out["keys"].shape[0] < max(need, rows_a):
                out = self._buf[1 - self._cur] = _records(max(need + need // 2, rows_a), dev, self.moments)
        else:
            out = self._buf[1 - self._cur]
        rows_o = out["keys"].shape[0]
        mkey = ("merge", rows_a, rows_c, rows_o)
        s_mrg = self._work.get(mkey)
        if s_mrg is None:
            s_mrg = _scratch256(lib.egonn_voxel_map_merge_scratch_bytes(rows_a, rows_c, rows_o), dev)
            if self.capacity is not None:
                self._work[mkey] = s_mrg
        if self.moments:                 # the scratch is merge's (egonn_voxel_map_merge_moments_scratch_bytes)
            _lib.call(dev, lib.egonn_voxel_map_merge_moments, *_mrec_ptrs(A), A["n"].data_ptr(), rows_a, *_mrec_ptrs(chunk),
                      chunk["n"].data_ptr(), rows_c, *_mrec_ptrs(out), rows_o, out["n"].data_ptr(), self._status.data_ptr(),
                      s_mrg.data_ptr(), s_mrg.numel() * 8)
        else:
            _lib.call(dev, lib.egonn_voxel_map_merge, *_rec_ptrs(A), A["n"].data_ptr(), rows_a, *_rec_ptrs(chunk), chunk["n"].data_ptr(),
                      rows_c, *_rec_ptrs(out), rows_o, out["n"].data_ptr(), self._status.data_ptr(), s_mrg.data_ptr(),
                      s_mrg.numel() * 8)
        out["_keep"] = (chunk, work, s_mrg, pk, ps)
        self._cur = 1 - self._cur

    def _observations(self, name, bank, poses, pick, points_capacity):
        """the argument checks `insert` and `remove` share, before a device is asked for -> (n, on_dev, p, sizes)"""
        n_bank = len(bank)
        on_dev = torch.is_tensor(pick) and pick.is_cuda
        n = n_bank if pick is None else len(pick)
        _check_poses(name, poses, n)
        if n < 1:
            raise ValueError(f"{name}: at least one observation")
        p = sizes = None
        if on_dev:
            if self.track:
                raise ValueError(f"{name}: a tracked map (track=True) takes host picks and host poses")
            if points_capacity is None or not 0 <= int(points_capacity) < 2 ** 31:
                raise ValueError(f"{name}: device picks need points_capacity in [0, 2^31)")
            if n > MAX_OBS:
                raise ValueError(f"{name}: at most {MAX_OBS} device picks per call, got {n}")
        else:
            p = np.arange(n_bank, dtype=np.int64) if pick is None else np.asarray(pick, dtype=np.int64).reshape(-1)
            if p.size and (p.min() < 0 or p.max() >= n_bank):
                raise ValueError(f"{name}: pick outside [0, {n_bank})")
            sizes = bank.sizes()[p]
        if self.track and torch.is_tensor(poses) and poses.is_cuda:
            raise ValueError(f"{name}: a tracked map (track=True) takes host picks and host poses")
        return n, on_dev, p, sizes

    def _chunks(self, bank, ps, n, on_dev, pick, p, sizes, points_capacity, subtract, held=None):
        """held (n,) bool, host picks: set for the observations of every chunk the map took.  Only a reserved map can drop a
        chunk (STATUS_CAPACITY); there each chunk runs on a cleared status word that is read back ([SYNC]) and OR-ed in again"""
        dev = self._dev()
        if on_dev:
            self._chunk(bank, _lib.as_dev(pick, dev, torch.int32), ps, n, int(points_capacity), subtract)
            return
        lo = 0
        while lo < n:
            hi, rows = lo + 1, int(sizes[lo])
            while hi < n and hi - lo < MAX_OBS and rows + int(sizes[hi]) <= self.chunk_points:
                rows += int(sizes[hi])
                hi += 1
            pk = torch.from_numpy(p[lo:hi].astype(np.int32)).to(dev)
            if held is None or self.capacity is None:
                self._chunk(bank, pk, ps[lo:hi].contiguous(), hi - lo, rows, subtract)
                took = True
            else:
                before = self._status.clone()
                self._status.zero_()
                self._chunk(bank, pk, ps[lo:hi].contiguous(), hi - lo, rows, subtract)
                took = not int(self._status.item()) & STATUS_CAPACITY              # [SYNC]
                self._status |= before
            if held is not None:
                held[lo:hi] = took
            lo = hi

    def insert(self, bank, poses, pick=None, points_capacity: Optional[int] = None) -> "VoxelMap":
        """Fuses clouds pick[k] of `bank` (a `CloudBank`; pick=None: all of them, in order) under poses[k] ((n,4,4) float64, scan
        frame -> map frame) into the map.  Host picks are chunked to <= 4096 observations and about `chunk_points` points; each
        chunk is integrated, then merged into the other record buffer.  Device picks (one chunk, <= 4096) need
        points_capacity, a bound on their clouds' total.  A tracked map appends (pick, pose) to its ledger; on a reserved map
        it reads the status after every chunk ([SYNC]) and a chunk dropped for STATUS_CAPACITY does not enter the ledger: the
        ledger is what the map holds.  Returns self."""
        n, on_dev, p, sizes = self._observations("VoxelMap.insert", bank, poses, pick, points_capacity)
        if self.origin is None:
            if torch.is_tensor(poses) and poses.is_cuda:
                raise ValueError("VoxelMap.insert: device poses need an explicit origin")
            o = np.asarray(poses[0], dtype=np.float64)[:3, 3].copy()
            if not np.isfinite(o).all():
                raise ValueError("VoxelMap.insert: the first pose's translation is not finite; give an origin")
            self.origin = o
        self._ensure()
        ps = _lib.as_dev(poses, self._dev(), torch.float64)
        held = np.zeros(n, dtype=bool) if self.track else None
        self._chunks(bank, ps, n, on_dev, pick, p, sizes, points_capacity, False, held)
        if self.track:
            host = np.asarray(poses, dtype=np.float64).reshape(n, 4, 4)
            self._ledger_pick += [int(p[k]) for k in range(n) if held[k]]
            self._ledger_pose += [host[k].copy() for k in range(n) if held[k]]
            self._held = held                                                    # `repose` reads it
        return self

    # ------------------------------------------------------------------ remove, repose
    def _ledger_match(self, name, p, host):
        """ledger positions of the (pick, pose) pairs, each entry used once; the pose is matched by its bytes"""
        free = {}
        for at, (lp, lx) in enumerate(zip(self._ledger_pick, self._ledger_pose)):
            free.setdefault((lp, lx.tobytes()), []).append(at)
        hit = []
        for k in range(len(p)):
            slots = free.get((int(p[k]), np.ascontiguousarray(host[k]).tobytes()))
            if not slots:
                raise ValueError(f"{name}: observation {k} (cloud {int(p[k])}) under this pose is not in the ledger")
            hit.append(slots.pop(0))
        return hit

    def remove(self, bank, poses, pick=None, points_capacity: Optional[int] = None) -> "VoxelMap":
        """Takes clouds pick[k] of `bank` under poses[k] out of the map again: the arguments, the chunking and the device-pick
        rule of `insert`; each chunk is integrated, then subtracted into the other record buffer (exactly: the sums are
        integers), and voxels left without points leave the map.  A tracked map checks every (pick, pose) against its ledger
        first (the pose by its bytes; each match uses one entry up, so a cloud inserted twice can be removed twice) and raises
        ValueError before any launch when one is missing.  Without tracking exactness is the caller's: the pose, the bank, the
        origin and the voxel size must be those of the insert, to the bit.  A chunk the map does not hold (a voxel absent, or
        fewer points or observations than the chunk has) sets STATUS_MISMATCH and leaves the map as it was before that chunk;
        earlier chunks of the call stay removed.  Returns self."""
        n, on_dev, p, sizes = self._observations("VoxelMap.remove", bank, poses, pick, points_capacity)
        hit = None
        if self.track:
            hit = self._ledger_match("VoxelMap.remove", p, np.asarray(poses, dtype=np.float64).reshape(n, 4, 4))
        if self._status is None:
            raise ValueError("VoxelMap.remove: the map is empty (nothing inserted)")
        ps = _lib.as_dev(poses, self._dev(), torch.float64)
        self._chunks(bank, ps, n, on_dev, pick, p, sizes, points_capacity, True)
        if hit is not None:
            gone = set(hit)
            self._ledger_pick = [v for at, v in enumerate(self._ledger_pick) if at not in gone]
            self._ledger_pose = [v for at, v in enumerate(self._ledger_pose) if at not in gone]
        return self

    def repose(self, bank, poses_new, rot_tol: float = 0.0, trans_tol: float = 0.0) -> int:
        """After a pose-graph correction: poses_new (len(ledger),4,4) host float64 in ledger order (track=True).  Entry k has
        moved iff max |R_new - R_old| > rot_tol or max |t_new - t_old| > trans_tol (elementwise, float64, on the host).
        The moved entries are removed at their ledger poses and inserted at the new ones; the ledger keeps its order and
        takes the new poses of the moved entries.  The tolerances trade map error for work; at their default 0 every pose
        that differs is fused again and the map is, bit for bit, the map built at poses_new.  On a reserved map a chunk of
        the re-insert that does not fit is dropped (STATUS_CAPACITY) and its entries leave the ledger with it.
        -> the number of entries moved."""
        if not self.track:
            raise ValueError("VoxelMap.repose: needs a tracked map (track=True)")
        if not (float(rot_tol) >= 0.0 and float(trans_tol) >= 0.0):
            raise ValueError("VoxelMap.repose: rot_tol and trans_tol are at least 0")
        picks, old = self.ledger
        _check_poses("VoxelMap.repose", poses_new, len(picks))
        if torch.is_tensor(poses_new) and poses_new.is_cuda:
            raise ValueError("VoxelMap.repose: poses_new on the host")
        new = np.array(poses_new, dtype=np.float64).reshape(len(picks), 4, 4)
        d = np.abs(new - old)
        d_rot = d[:, :3, :3].reshape(-1, 9).max(axis=1, initial=0.0)
        d_trans = d[:, :3, 3].max(axis=1, initial=0.0)
        at = np.flatnonzero((d_rot > float(rot_tol)) | (d_trans > float(trans_tol)))
        if at.size:
            self.remove(bank, old[at], picks[at])
            self.insert(bank, new[at], picks[at])
            old[at] = new[at]
            keep = np.ones(len(picks), dtype=bool)
            keep[at] = self._held                                                # a dropped chunk's entries are gone
            self._ledger_pick = [int(picks[k]) for k in range(len(picks)) if keep[k]]
            self._ledger_pose = [old[k].copy() for k in range(len(picks)) if keep[k]]
        return int(at.size)

    # ------------------------------------------------------------------ read
    def _select(self, boxes, n_boxes, relative, min_count, min_obs, capacity, with_counts):
        lib = _lib.load()
        dev = self._dev()
        R = self.records
        rows = R["keys"].shape[0]
        n_seg = max(n_boxes, 1)
        off = torch.empty((n_seg + 1,), dtype=torch.int64, device=dev)
        status = torch.zeros((), dtype=torch.int32, device=dev)
        scratch = _scratch256(lib.egonn_voxel_map_select_scratch_bytes(rows, n_boxes), dev)
        head = (*_rec_ptrs(R), R["n"].data_ptr(), rows, self._origin_c(), self.voxel_size, int(min_count), int(min_obs),
                _lib._ptr(boxes), n_boxes, int(bool(relative)))
        if capacity is None:                                                 # the sizing call, then [SYNC] its total
            _lib.call(dev, lib.egonn_voxel_map_select, *head, None, off.data_ptr(), None, None, 0, status.data_ptr(),
                      scratch.data_ptr(), scratch.numel() * 8)
            capacity = int(off[-1].item())
        capacity = int(capacity)
        pts = torch.empty((max(capacity, 1), 3), dtype=torch.float64, device=dev)
        cnt = torch.empty((max(capacity, 1),), dtype=torch.int32, device=dev) if with_counts else None
        obs = torch.empty((max(capacity, 1),), dtype=torch.int32, device=dev) if with_counts else None
        _lib.call(dev, lib.egonn_voxel_map_select, *head, pts.data_ptr(), off.data_ptr(), _lib._ptr(cnt), _lib._ptr(obs), capacity,
                  status.data_ptr(), scratch.data_ptr(), scratch.numel() * 8)
        return {"points": pts[:capacity], "offsets": off, "count": cnt, "observations": obs, "status": status,
                "_keep": (scratch, boxes, R)}

    def points(self, min_count: int = 1, min_observations: int = 1) -> Dict[str, torch.Tensor]:
        """The map as points: the centroids of the voxels with at least min_count points seen by at least min_observations
        scans, ascending key order -> {'points' (m,3) f64, 'count' (m,) int32, 'observations' (m,) int32} on the device.
        [SYNC] once, for m."""
        _check_filters("VoxelMap.points", min_count, min_observations)
        if self._status is None:
            raise ValueError("VoxelMap.points: the map is empty (nothing inserted)")
        r = self._select(None, 0, False, min_count, min_observations, None, True)
        m = r["points"].shape[0]
        return {"points": r["points"], "count": r["count"][:m], "observations": r["observations"][:m]}

    def submaps(self, centers, half_extent, min_count: int = 1, min_observations: int = 1, relative: bool = True,
                capacity: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """One submap per centre (n,3) in the map frame: the centroids c with centre - half <= c < centre + half per axis
        (half_extent: one number or three), ascending key order, as c - centre when `relative` (what `icp_pairs` wants as tgt:
        its search grid takes local coordinates) -> {'points' (capacity,3) f64, 'offsets' (n+1,) int64, 'status' () int32} on the
        device.  capacity=None sizes the output exactly ([SYNC] once); with a capacity there is no host synchronisation, and more
        points than it give STATUS_CAPACITY, all offsets zero."""
        half = _check_boxes("VoxelMap.submaps", centers, half_extent)
        _check_filters("VoxelMap.submaps", min_count, min_observations)
        if capacity is not None and not 0 <= int(capacity) < 2 ** 31:
            raise ValueError("VoxelMap.submaps: capacity in [0, 2^31)")
        if self._status is None:
            raise ValueError("VoxelMap.submaps: the map is empty (nothing inserted)")
        dev = self._dev()
        c = _lib.as_dev(centers, dev, torch.float64)
        boxes = torch.cat([c, torch.from_numpy(half).to(dev).expand(c.shape[0], 3)], dim=1).contiguous()
        r = self._select(boxes, c.shape[0], relative, min_count, min_observations, capacity, False)
        return {"points": r["points"], "offsets": r["offsets"], "status": r["status"], "_keep": r["_keep"]}

    # ------------------------------------------------------------------ files
    def save(self, path: str) -> None:
        """one .npz: the records, voxel_size, origin; the moments and the ledger when the map has them.  [SYNC]"""
        if self._status is None:
            raise ValueError("VoxelMap.save: the map is empty (nothing inserted)")
        R, n = self.records, self.n_voxels
        extra = {f: R[f][:n].cpu().numpy() for f in _MOMENTS} if self.moments else {}
        if self.track:
            extra["ledger_pick"], extra["ledger_poses"] = self.ledger
        np.savez(path, voxel_size=np.float64(self.voxel_size), origin=np.asarray(self.origin, dtype=np.float64),
                 status=np.int32(self.status), **{f: R[f][:n].cpu().numpy() for f in _FIELDS}, **extra)

    @classmethod
    def load(cls, path: str, capacity: Optional[int] = None, device=None, moments: Optional[bool] = None,
             track: Optional[bool] = None) -> "VoxelMap":
        """moments / track = None: as the file has them.  A file with moments loads only into a moments map and a file
        without them only into a plain one; track=True needs a file with a ledger."""
        with np.load(path) as z:
            missing = [k for k in _FIELDS + ("voxel_size", "origin") if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a voxel map (missing {missing})")
            data = {k: z[k] for k in z.files}
        has_m, has_l = all(f in data for f in _MOMENTS), "ledger_pick" in data and "ledger_poses" in data
        if moments is not None and bool(moments) != has_m:
            raise ValueError(f"{path}: a voxel map {'with' if has_m else 'without'} moments does not load into a map "
                             f"{'with' if moments else 'without'} them")
        if track and not has_l:
            raise ValueError(f"{path}: a voxel map without a ledger does not load into a tracked map")
        n = len(data["keys"])
        if capacity is not None and int(capacity) < n:
            raise ValueError(f"VoxelMap.load: capacity {capacity} below the file's {n} voxels")
        if not has_m and not has_l:
            m = cls(float(data["voxel_size"]), data["origin"], capacity, device)
        else:
            m = cls(float(data["voxel_size"]), data["origin"], capacity, device, moments=has_m,
                    track=has_l if track is None else bool(track))
        m._ensure()
        if capacity is None:
            m._buf[0] = _records(n, m._dev(), has_m)
        for f in _FIELDS + (_MOMENTS if has_m else ()):
            m._buf[0][f][:n] = torch.from_numpy(data[f]).to(m._dev())
        m._buf[0]["n"].fill_(n)
        m._status.fill_(int(data.get("status", 0)))
        if m.track:
            lp = np.asarray(data["ledger_pick"]).reshape(-1)
            lx = np.asarray(data["ledger_poses"], dtype=np.float64).reshape(-1, 4, 4)
            if len(lp) != len(lx):
                raise ValueError(f"{path}: the ledger's picks and poses differ in number")
            m._ledger_pick, m._ledger_pose = [int(v) for v in lp], [lx[k].copy() for k in range(len(lx))]
        return m


def build_map(bank, poses, voxel_size: float = 0.2, **kw) -> VoxelMap:
    """every cloud of `bank` under its pose: VoxelMap(voxel_size, **kw).insert(bank, poses)"""
    return VoxelMap(voxel_size, **kw).insert(bank, poses)


NDT_MIN_POINTS = 6            # a choice, not a tuned value: twice the three points a covariance needs at the least
NDT_MIN_EIG_RATIO = 0.01      # a choice: a flat voxel is given a thickness of a tenth of its largest extent (in sigma)
NDT_MAX_ITERATION, NDT_EPS_ROT, NDT_EPS_TRANS = 30, 1e-5, 1e-4      # choices: rounds, and a step of 1e-5 rad / 0.1 mm
_NDT_FIELDS = ("keys", "cnt", "s1", "s2")


class NDTMap:
    """The NDT layer over the keys of `vmap` (a `VoxelMap` that holds something): a snapshot (a clone of the keys and one
    [SYNC] for their number, `voxel_size`, `origin`); later inserts into `vmap` do not disturb it.  `accumulate` adds the exact
    integer moments of posed clouds (any batching and order: the bits of one call), `finalize` turns them into one Gaussian per
    voxel with at least `min_points` points, `register` runs the NDT against them."""

    def __init__(self, vmap: VoxelMap, min_points: int = NDT_MIN_POINTS, min_eig_ratio: float = NDT_MIN_EIG_RATIO,
                 chunk_points: int = 4_000_000):
        self._check_rule(min_points, min_eig_ratio)
        if int(chunk_points) < 1:
            raise ValueError("NDTMap: chunk_points must be positive")
        if not isinstance(vmap, VoxelMap) or vmap._status is None:
            raise ValueError("NDTMap: the voxel map is empty (nothing inserted)")
        n = vmap.n_voxels                                                     # [SYNC]
        self._init(vmap.records["keys"][:n].clone(), vmap.voxel_size, vmap.origin, min_points, min_eig_ratio, chunk_points, vmap._dev())

    @classmethod
    def from_map(cls, vmap: VoxelMap, min_points: int = NDT_MIN_POINTS, min_eig_ratio: float = NDT_MIN_EIG_RATIO,
                 chunk_points: int = 4_000_000) -> "NDTMap":
        """The layer of a map that carries its moments (`VoxelMap(moments=True)`): keys / cnt / s1 / s2 are copies of the map's
        live records, `missed` is 0, and no point is read again.  The synchronisation is `update`'s."""
        cls._check_rule(min_points, min_eig_ratio)
        if int(chunk_points) < 1:
            raise ValueError("NDTMap: chunk_points must be positive")
        m = cls.__new__(cls)
        m.min_points, m.min_eig_ratio, m.chunk_points = int(min_points), float(min_eig_ratio), int(chunk_points)
        m.keys = None
        return m.update(vmap)

    def update(self, vmap: VoxelMap) -> "NDTMap":
        """Snapshots `vmap` (with moments) again after it grew, shrank or was re-posed, and drops the Gaussians: `finalize`
        anew.  A map with a reserved `capacity` is copied at that size together with its device count: no host
        synchronisation.  `gaussians` then have `capacity` rows (zeros from the live count on); `keys`, `cnt`, `s1` and `s2`
        hold whatever the map's buffer held behind the live count (no kernel reads those rows), and the first read of
        `n_voxels`, which `save` takes, is a [SYNC].  Otherwise one [SYNC] for the count, as the constructor takes."""
        if not isinstance(vmap, VoxelMap) or vmap._status is None:
            raise ValueError("NDTMap: the voxel map is empty (nothing inserted)")
        if not vmap.moments:
            raise ValueError("NDTMap: the voxel map carries no moments (VoxelMap(moments=True))")
        if self.keys is not None and (float(vmap.voxel_size) != self.voxel_size or
                                      not np.array_equal(np.asarray(vmap.origin, np.float64), self.origin)):
            raise ValueError("NDTMap.update: another voxel size or origin than the layer's")
        R, dev = vmap.records, vmap._dev()
        n = R["keys"].shape[0] if vmap.capacity is not None else vmap.n_voxels            # [SYNC] without a capacity
        self._init(R["keys"][:n], vmap.voxel_size, vmap.origin, self.min_points, self.min_eig_ratio, self.chunk_points, dev)
        self.cnt[:n], self.s1[:n], self.s2[:n] = R["count"][:n], R["s1"][:n], R["s2"][:n]
        self._status.copy_(vmap._status)
        if vmap.capacity is not None:
            self._n.copy_(R["n"])
            self._n_host = None
        return self

    @staticmethod
    def _check_rule(min_points, min_eig_ratio):
        if int(min_points) < 3:
            raise ValueError("NDTMap: min_points is at least 3")
        if not (float(min_eig_ratio) > 0.0 and np.isfinite(float(min_eig_ratio))):
            raise ValueError("NDTMap: min_eig_ratio must be positive and finite")

    def _init(self, keys, voxel_size, origin, min_points, min_eig_ratio, chunk_points, dev):
        n = int(keys.shape[0])
        rows = max(n, 1)
        self.device, self.voxel_size, self.origin = dev, float(voxel_size), np.asarray(origin, dtype=np.float64).copy()
        self.min_points, self.min_eig_ratio, self.chunk_points = int(min_points), float(min_eig_ratio), int(chunk_points)
        self._n_host = n                                                      # None: only the device knows (`update`)
        self.keys = torch.zeros((rows,), dtype=torch.int64, device=dev)
        self.keys[:n] = keys
        self._n = torch.full((), n, dtype=torch.int64, device=dev)
        self.cnt = torch.zeros((rows,), dtype=torch.int32, device=dev)
        self.s1 = torch.zeros((rows, 3), dtype=torch.int64, device=dev)
        self.s2 = torch.zeros((rows, 6), dtype=torch.int64, device=dev)
        self._missed = torch.zeros((), dtype=torch.int64, device=dev)
        self._status = torch.zeros((), dtype=torch.int32, device=dev)
        self._origin_dev = torch.from_numpy(self.origin).to(dev)
        self.gaussians = None

    def _origin_c(self):
        return (ctypes.c_double * 3)(*[float(v) for v in self.origin])

    @property
    def n_voxels(self) -> int:
        """the rows of the layer; [SYNC] once after an `update` from a map with a reserved capacity"""
        if self._n_host is None:
            self._n_host = int(self._n.item())
        return self._n_host

    @property
    def missed(self) -> int:
        """[SYNC] valid points whose voxel is not among the keys"""
        return int(self._missed.item())

    @property
    def status(self) -> int:
        """[SYNC] OR of the STATUS_* bits of every `accumulate` so far"""
        return int(self._status.item())

    def accumulate(self, bank, poses, pick=None) -> "NDTMap":
        """Adds the moments of clouds pick[k] of `bank` (host picks; None: all, in order) under poses[k] ((n,4,4) f64, scan frame ->
        map frame), chunked as `VoxelMap.insert` chunks.  The Gaussians of an earlier `finalize` are dropped.  Returns self."""
        n_bank = len(bank)
        n = n_bank if pick is None else len(pick)
        _check_poses("NDTMap.accumulate", poses, n)
        if n < 1:
            raise ValueError("NDTMap.accumulate: at least one observation")
        p = np.arange(n_bank, dtype=np.int64) if pick is None else np.asarray(pick, dtype=np.int64).reshape(-1)
        if p.size and (p.min() < 0 or p.max() >= n_bank):
            raise ValueError(f"NDTMap.accumulate: pick outside [0, {n_bank})")
        sizes = bank.sizes()[p]
        lib, dev = _lib.load(), self.device
        ps = _lib.as_dev(poses, dev, torch.float64)
        rows_m, n_pts, keep = self.keys.shape[0], bank.n_points, []
        lo = 0
        while lo < n:
            hi, rows = lo + 1, int(sizes[lo])
            while hi < n and hi - lo < MAX_OBS and rows + int(sizes[hi]) <= self.chunk_points:
                rows += int(sizes[hi])
                hi += 1
            pk = torch.from_numpy(p[lo:hi].astype(np.int32)).to(dev)
            pc = ps[lo:hi].contiguous()
            s = _scratch256(lib.egonn_ndt_accumulate_scratch_bytes(rows, hi - lo), dev)
            _lib.call(dev, lib.egonn_ndt_accumulate, _lib._ptr(bank.points) if n_pts else None, n_pts, bank.offsets().data_ptr(), n_bank,
                      pk.data_ptr(), pc.data_ptr(), hi - lo, self._origin_c(), self.voxel_size, rows, self.keys.data_ptr(),
                      self._n.data_ptr(), rows_m, self.cnt.data_ptr(), self.s1.data_ptr(), self.s2.data_ptr(), self._missed.data_ptr(),
                      self._status.data_ptr(), s.data_ptr(), s.numel() * 8)
            keep.append((pk, pc, s))
            lo = hi
        self._keep, self.gaussians = keep, None
        return self

    def finalize(self, debug: bool = False) -> Dict[str, torch.Tensor]:
        """One Gaussian per voxel -> `gaussians` = {'mean' (n,3) f64 relative to `origin` (add it for a world point), 'info' (n,6)
        f64 (xx, xy, xz, yy, yz, zz), 'eigenvalues' (n,3) ascending, 'normal' (n,3), 'valid' (n,) uint8, 'n_valid' () int64} on
        the device; debug adds 'cov' (n,6).  An invalid voxel (fewer than min_points points, no extent) is all zeros."""
        lib, dev, rows = _lib.load(), self.device, self.keys.shape[0]
        f64 = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=dev)        # noqa: E731
        g = {"mean": f64(rows, 3), "info": f64(rows, 6), "eigenvalues": f64(rows, 3), "normal": f64(rows, 3),
             "valid": torch.zeros((rows,), dtype=torch.uint8, device=dev), "n_valid": torch.zeros((), dtype=torch.int64, device=dev)}
        if debug:
            g["cov"] = f64(rows, 6)
        _lib.call(dev, lib.egonn_ndt_finalize, self.keys.data_ptr(), self._n.data_ptr(), rows, self.cnt.data_ptr(), self.s1.data_ptr(),
                  self.s2.data_ptr(), self.voxel_size, self.min_points, self.min_eig_ratio, g["mean"].data_ptr(), g["info"].data_ptr(),
                  g["eigenvalues"].data_ptr(), g["normal"].data_ptr(), g["valid"].data_ptr(), g["n_valid"].data_ptr(),
                  _lib._ptr(g.get("cov")))
        n = rows if self._n_host is None else self._n_host
        self._layer = g
        self.gaussians = {k: (v if v.dim() == 0 else v[:n]) for k, v in g.items()}
        return self.gaussians

    def register(self, points, offsets, poses_init, neighbors: int = 1, max_iteration: int = NDT_MAX_ITERATION,
                 eps_rot: float = NDT_EPS_ROT, eps_trans: float = NDT_EPS_TRANS, debug: bool = False) -> Dict[str, torch.Tensor]:
        """NDT of P scans against the map: points (n,3) concatenated clouds with (P+1,) offsets (what `voxel_downsample` and
        `CloudBank.gather` return), poses_init (P,4,4) scan frame -> world frame.  `origin` is subtracted before and added after
        the library call, which works in the origin-relative frame.  neighbors: 1 (the voxel a point falls into) or 7 (and its
        face neighbours).  -> {'poses' (P,4,4) f64, 'fitness' (points with a Gaussian / points), 'score' (mean of exp(-d^2/2)
        over the points) (P,) f64, 'iterations', 'status' (P,) int32 (ICP_* bits)} on the device; debug adds T_trace
        (P, max_iteration+1, 4, 4) in the origin-relative frame, eval_trace (P, max_iteration+1, 4) = n_term, n_pts, score, stop
        and sums_trace (P, max_iteration+1, 30) = n_term, n_pts, A (21), b (6), score of every evaluation.  No host synchronisation with device arguments; capturable."""
        _reg._check_cloud("NDTMap.register", points)
        P = _reg._check_offsets("NDTMap.register", offsets)
        _check_poses("NDTMap.register", poses_init, P)
        if not 1 <= P <= MAX_OBS:
            raise ValueError(f"NDTMap.register: 1 to {MAX_OBS} scans per call, got {P}")
        if int(neighbors) not in (1, 7):
            raise ValueError(f"NDTMap.register: neighbors is 1 or 7, got {neighbors}")
        if int(max_iteration) < 0 or not all(float(e) > 0.0 and np.isfinite(float(e)) for e in (eps_rot, eps_trans)):
            raise ValueError("NDTMap.register: max_iteration >= 0, eps_rot and eps_trans positive and finite")
        if self.gaussians is None:
            raise ValueError("NDTMap.register: call finalize() first")
        lib, dev, g, K = _lib.load(), self.device, self._layer, int(max_iteration)
        src, off = _lib.as_dev(points, dev, torch.float64), _lib.as_dev(offsets, dev, torch.int64)
        T0 = _lib.as_dev(poses_init, dev, torch.float64).clone()
        T0[:, :3, 3] -= self._origin_dev
        ns = src.shape[0]
        s = _scratch256(lib.egonn_ndt_register_scratch_bytes(ns, P), dev)
        f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)        # noqa: E731
        i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)          # noqa: E731
        out = {"T": f64(P, 4, 4), "fitness": f64(P), "score": f64(P), "iterations": i32(P), "status": i32(P)}
        if debug:
            out.update({"T_trace": f64(P, K + 1, 4, 4), "eval_trace": f64(P, K + 1, 4), "sums_trace": f64(P, K + 1, 30)})
        _lib.call(dev, lib.egonn_ndt_register, src.data_ptr() if ns else None, ns, off.data_ptr(), P, T0.data_ptr(), self.keys.data_ptr(),
                  self._n.data_ptr(), self.keys.shape[0], g["mean"].data_ptr(), g["info"].data_ptr(), g["valid"].data_ptr(),
                  self.voxel_size, int(neighbors), K, float(eps_rot), float(eps_trans), out["T"].data_ptr(), out["fitness"].data_ptr(),
                  out["score"].data_ptr(), out["iterations"].data_ptr(), out["status"].data_ptr(), _lib._ptr(out.get("T_trace")),
                  _lib._ptr(out.get("eval_trace")), _lib._ptr(out.get("sums_trace")), s.data_ptr(), s.numel() * 8)
        poses = out.pop("T").clone()
        poses[:, :3, 3] += self._origin_dev
        out["poses"] = poses
        out["_keep"] = (src, off, T0, s, g)
        return out

    # ------------------------------------------------------------------ files
    def save(self, path: str) -> None:
        """one .npz: the keys, the moments, the rule, voxel_size, origin; `load` finalizes again where this one was.  [SYNC]"""
        n = self.n_voxels
        np.savez(path, voxel_size=np.float64(self.voxel_size), origin=self.origin, min_points=np.int32(self.min_points),
                 min_eig_ratio=np.float64(self.min_eig_ratio), missed=np.int64(self.missed), status=np.int32(self.status),
                 finalized=np.int32(self.gaussians is not None), ndt=np.int32(1),
                 **{f: getattr(self, f)[:n].cpu().numpy() for f in _NDT_FIELDS})

    @classmethod
    def load(cls, path: str, device=None) -> "NDTMap":
        with np.load(path) as z:
            missing = [k for k in _NDT_FIELDS + ("ndt", "voxel_size", "origin", "min_points", "min_eig_ratio") if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not an NDT map (missing {missing})")
            data = {k: z[k] for k in z.files}
        cls._check_rule(int(data["min_points"]), float(data["min_eig_ratio"]))
        dev = device if device is not None else _lib.require_gpu()
        m = cls.__new__(cls)
        m._init(torch.from_numpy(data["keys"]).to(dev), float(data["voxel_size"]), data["origin"], int(data["min_points"]),
                float(data["min_eig_ratio"]), 4_000_000, dev)
        n = m.n_voxels
        for f in ("cnt", "s1", "s2"):
            getattr(m, f)[:n] = torch.from_numpy(data[f]).to(dev)
        m._missed.fill_(int(data.get("missed", 0)))
        m._status.fill_(int(data.get("status", 0)))
        if int(data.get("finalized", 0)):
            m.finalize()
        return m


def build_ndt_map(bank, poses, voxel_size: float = 1.0, min_points: int = NDT_MIN_POINTS, min_eig_ratio: float = NDT_MIN_EIG_RATIO,
                  moments: bool = False, **kw) -> NDTMap:
    """every cloud of `bank` under its pose as an NDT map: build_map, NDTMap(...).accumulate(bank, poses), finalize().  1.0 m by
    default, not the voxel map's 0.2 m: a Gaussian needs points (at 0.2 m a voxel of the 0.1 m downsample holds a handful).
    moments=True reads every point once: a map with moments, `NDTMap.from_map`, finalize(); the map is the result's `.vmap`
    (insert into it, remove from it or repose it, then `update` and `finalize` the layer).  The same bits either way."""
    NDTMap._check_rule(min_points, min_eig_ratio)
    if moments:
        vm = build_map(bank, poses, voxel_size, moments=True, **kw)
        m = NDTMap.from_map(vm, min_points, min_eig_ratio)
        m.finalize()
        m.vmap = vm
        return m
    m = NDTMap(build_map(bank, poses, voxel_size, **kw), min_points, min_eig_ratio)
    m.accumulate(bank, poses).finalize()
    return m


def refine_against_map(vmap: VoxelMap, bank, pick, poses_init, half_extent=30.0, min_count: int = 1, min_observations: int = 1,
                       method: str = "icp", ndt: Optional[NDTMap] = None, **icp_kw) -> Dict[str, torch.Tensor]:
    """Scan-to-map ICP by composition: for scan pick[k] of `bank` with the initial pose poses_init[k] (scan -> map frame), the
    source is its cloud (`bank.gather`), the target the submap of `vmap` around the pose's translation (`submaps`, relative),
    T_init = translate(-centre) @ pose_init, `icp_pairs` runs on that and pose = translate(+centre) @ T.  Host picks.
    -> {'poses' (n,4,4) f64, 'fitness', 'inlier_rmse' (n,) f64, 'status' (n,) int32 (ICP_* bits)} on the device.  [SYNC] once,
    to size the submaps.
    method="ndt" registers against `ndt` (an `NDTMap`, finalized) instead: the clouds are gathered and handed to `ndt.register`
    with the keywords of that call; there is no submap and no sizing synchronisation (vmap, half_extent and the two filters
    are not read) -> the dict of `NDTMap.register`."""
    if method not in ("icp", "ndt"):
        raise ValueError(f"refine_against_map: method is 'icp' or 'ndt', got {method!r}")
    n = len(pick)
    _check_poses("refine_against_map", poses_init, n)
    if not 1 <= n <= MAX_OBS:
        raise ValueError(f"refine_against_map: 1 to {MAX_OBS} scans per call, got {n}")
    if method == "ndt":
        if not isinstance(ndt, NDTMap):
            raise ValueError("refine_against_map: method='ndt' needs ndt=NDTMap")
        src = bank.gather(pick)
        r = ndt.register(src["points"], src["offsets"], poses_init, **icp_kw)
        r["_keep"] = (src, r["_keep"])
        return r
    dev = vmap._dev()
    X = _lib.as_dev(poses_init, dev, torch.float64)
    centre = X[:, :3, 3].contiguous()
    tgt = vmap.submaps(centre, half_extent, min_count, min_observations, relative=True)
    src = bank.gather(pick)
    T0 = X.clone()
    T0[:, :3, 3] = 0.0                                                       # t - centre with centre = t
    r = _reg.icp_pairs(src["points"], src["offsets"], tgt["points"], tgt["offsets"], T0, **icp_kw)
    poses = r["T"].clone()
    poses[:, :3, 3] += centre
    return {"poses": poses, "fitness": r["fitness"], "inlier_rmse": r["inlier_rmse"], "status": r["status"],
            "_keep": (src, tgt, r)}
