"""ScanContext, the hand-crafted baseline the reference compares EgoNN with, on the device.

Mirrors the reference's names (third_party/scan_context/scan_context.py): `ScanContext` (:23-55), `sc2rk` (:86-88),
`distance_sc` (:58-83), `ScanContextManager` (:91-156), and `evaluate` (third_party/scan_context/evaluate_scan_context.py:
24-84).  Descriptors, ring keys, distances and the rerank run in libegonn_hip (egonn_scan_context /
egonn_scan_context_ringkey / egonn_scan_context_distance / egonn_scan_context_rerank, csrc/scan_context.hip), the candidate
search is egonn_knn over the ring keys and the recall table egonn_recall_counts; there is no torch or numpy fallback for the
arithmetic.  Batches follow the (points, offsets) convention of registration.py and ingest.py: points (n, 3), scan b = rows
[offsets[b], offsets[b+1]).  Results are float32 device tensors (the reference's descriptors are float64 arrays that hold
float32 heights, so nothing is lost).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import as_dev as _dev, check_cloud as _check_cloud, check_offsets as _check_offsets, concat_clouds as _concat_clouds
from .retrieval import knn

MAX_RING, MAX_SECTOR, MAX_K = 40, 128, 128
_CHUNK = 64          # scans per launch when lists of clouds are fed


def _check_shape(num_ring, num_sector):
    if not (1 <= int(num_ring) <= MAX_RING) or not (2 <= int(num_sector) <= MAX_SECTOR):
        raise ValueError(f"scan context: num_ring must be in [1, {MAX_RING}] and num_sector in [2, {MAX_SECTOR}], got "
                         f"{num_ring} x {num_sector}")


def _check_k(k):
    if not (1 <= int(k) <= MAX_K):
        raise ValueError(f"scan context: k must be in [1, {MAX_K}], got {k}")


def _check_sc(name, sc, lead_dims=(2, 3)):
    shape = tuple(getattr(sc, "shape", ()))
    if len(shape) not in lead_dims:
        raise ValueError(f"{name}: expected a (num_ring, num_sector) descriptor or a stack of them, got shape {shape}")
    _check_shape(shape[-2], shape[-1])
    return shape


def _device_of(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return _lib.require_gpu()


class ScanContext:
    """scan_context.py:23-55.  `__call__(pc)` -> (num_ring, num_sector); `batch(points, offsets)` -> ((B, R, S), (B, R)):
    descriptors and ring keys of B resident scans in one call, free of host synchronisation when both are device tensors."""

    def __init__(self, num_sector=60, num_ring=20, max_length=80, lidar_height=2.0):
        _check_shape(num_ring, num_sector)
        if not float(max_length) > 0.0:
            raise ValueError("scan context: max_length must be positive")
        self.lidar_height = float(lidar_height)
        self.num_sector = int(num_sector)
        self.num_ring = int(num_ring)
        self.max_length = float(max_length)
        self.gap_ring = self.max_length / self.num_ring
        self.gap_sector = 2. * np.pi / self.num_sector

    def batch(self, points, offsets):
        _check_cloud("ScanContext.batch", points)
        B = _check_offsets("ScanContext.batch", offsets)
        if B > 65535:
            raise ValueError("ScanContext.batch: at most 65535 scans per call")
        dev = _device_of(points)
        lib = _lib.load()
        pts, off = _dev(points, dev, torch.float32), _dev(offsets, dev, torch.int64)
        n = pts.shape[0]
        sc = torch.empty((B, self.num_ring, self.num_sector), dtype=torch.float32, device=dev)
        rk = torch.empty((B, self.num_ring), dtype=torch.float32, device=dev)
        _lib.call(dev, lib.egonn_scan_context, pts.data_ptr() if n else None, n, off.data_ptr(), B, self.num_sector,
                  self.num_ring, self.max_length, self.lidar_height, sc.data_ptr(), rk.data_ptr())
        return sc, rk

    def __call__(self, pc):
        _check_cloud("ScanContext", pc)
        return self.batch(pc, np.array([0, pc.shape[0]], dtype=np.int64))[0][0]


def sc2rk(sc):
    """scan_context.py:86-88: the ring key, the mean over sectors.  (R, S) -> (R,), (B, R, S) -> (B, R)."""
    shape = _check_sc("sc2rk", sc)
    dev = _device_of(sc)
    lib = _lib.load()
    x = _dev(sc, dev, torch.float32).reshape(-1, shape[-2], shape[-1])
    rk = torch.empty((x.shape[0], shape[-2]), dtype=torch.float32, device=dev)
    _lib.call(dev, lib.egonn_scan_context_ringkey, x.data_ptr() if x.shape[0] else None, x.shape[0], shape[-2], shape[-1],
              rk.data_ptr() if x.shape[0] else None)
    return rk[0] if len(shape) == 2 else rk


def distance_pairs(query_sc, map_sc, candidates=None):
    """distance_sc(map_sc[c], query_sc[q]) for every listed pair: query_sc (Q, R, S), map_sc (M, R, S), candidates (Q, k)
    int32 or None = every map element.  -> (dist (Q, k) f32, yaw (Q, k) int32) on the device; a candidate of -1 gives
    (+inf, -1), a pair with an all-zero descriptor (NaN, 1).  No host synchronisation with device tensors."""
    qs, ms = _check_sc("distance_pairs: query_sc", query_sc, (3,)), _check_sc("distance_pairs: map_sc", map_sc, (3,))
    if qs[1:] != ms[1:]:
        raise ValueError(f"distance_pairs: descriptors of different shapes, {qs[1:]} and {ms[1:]}")
    Q, M = qs[0], ms[0]
    if candidates is not None:
        cs = tuple(candidates.shape)
        if len(cs) != 2 or cs[0] != Q:
            raise ValueError(f"distance_pairs: candidates must have shape ({Q}, k), got {cs}")
    k = M if candidates is None else cs[1]
    dev = _device_of(query_sc, map_sc)
    lib = _lib.load()
    q, m = _dev(query_sc, dev, torch.float32), _dev(map_sc, dev, torch.float32)
    c = None if candidates is None else _dev(candidates, dev, torch.int32)
    dist = torch.empty((Q, k), dtype=torch.float32, device=dev)
    yaw = torch.empty((Q, k), dtype=torch.int32, device=dev)
    _lib.call(dev, lib.egonn_scan_context_distance, q.data_ptr() if Q else None, Q, m.data_ptr() if M else None, M, qs[1],
              qs[2], _lib._ptr(c) if k else None, k, dist.data_ptr(), yaw.data_ptr())
    return dist, yaw


def rerank(dist, yaw, candidates):
    """scan_context.py:151-154 for every query: (Q, k) x 3 -> (nn_ndx, sc_dist, sc_yaw_diff) ascending by distance, NaN last,
    equal distances by lower candidate index."""
    ds = tuple(dist.shape)
    if len(ds) != 2 or tuple(yaw.shape) != ds or tuple(candidates.shape) != ds:
        raise ValueError("rerank: dist, yaw and candidates must share one (Q, k) shape")
    _check_k(ds[1])
    dev = _device_of(dist, yaw, candidates)
    lib = _lib.load()
    d, y, c = _dev(dist, dev, torch.float32), _dev(yaw, dev, torch.int32), _dev(candidates, dev, torch.int32)
    oi, od, oy = torch.empty_like(c), torch.empty_like(d), torch.empty_like(y)
    _lib.call(dev, lib.egonn_scan_context_rerank, d.data_ptr(), y.data_ptr(), c.data_ptr(), ds[0], ds[1], oi.data_ptr(),
              od.data_ptr(), oy.data_ptr())
    return oi, od, oy


def distance_sc(sc1, sc2):
    """scan_context.py:58-83 for one pair: sc1 is the descriptor that is shifted (the candidate), sc2 the query.
    -> (dist, yaw_diff).  [SYNC] copies the result back."""
    s1, s2 = _check_sc("distance_sc", sc1, (2,)), _check_sc("distance_sc", sc2, (2,))
    if s1 != s2:
        raise ValueError(f"distance_sc: descriptors of different shapes, {s1} and {s2}")
    dev = _device_of(sc1, sc2)
    d, y = distance_pairs(_dev(sc2, dev, torch.float32)[None], _dev(sc1, dev, torch.float32)[None])
    return float(d[0, 0]), int(y[0, 0])


class ScanContextManager:
    """scan_context.py:91-156 with the descriptors kept on the device.  `add_node(pc)` / `add_nodes(points, offsets)` (the
    batched form, which is what a streaming ingest feeds) store descriptors and ring keys; `query(query_pc, k, reranking)`
    -> (nn_ndx, sc_dist, sc_yaw_diff) as numpy arrays for one cloud, `query_batch(points, offsets, k, reranking)` the same
    as (Q, k) device tensors for a batch of query scans.  Candidates are the k nearest ring keys (egonn_knn); with
    reranking they are ordered by the full descriptor distance.

    The reference builds its KD-tree over `ringkeys[:curr_node_idx - 1]` (:127), so the node added last can never be
    returned.  That is kept as the default (`include_last_node=False`) so that recall figures stay comparable with the
    reference's; `include_last_node=True` searches every node.  As in the reference (:120) the number of nodes must stay
    below `max_capacity`; here that is a ValueError raised before anything is stored."""

    def __init__(self, num_sector=60, num_ring=20, max_length=80, lidar_height=2.0, max_capacity=100000,
                 include_last_node=False):
        self.num_sector, self.num_ring = int(num_sector), int(num_ring)
        self.max_length, self.lidar_height = max_length, lidar_height
        self.max_capacity = int(max_capacity)
        self.include_last_node = bool(include_last_node)
        self.sc = ScanContext(self.num_sector, self.num_ring, self.max_length, self.lidar_height)
        self._sc_parts, self._rk_parts = [], []
        self.curr_node_idx = 0

    def _reserve(self, count):
        if self.curr_node_idx + count >= self.max_capacity:
            raise ValueError(f"Maximum ScanContextManager capacity exceeded: {self.max_capacity}")

    def add_nodes(self, points, offsets):
        _check_cloud("ScanContextManager.add_nodes", points)
        B = _check_offsets("ScanContextManager.add_nodes", offsets)
        self._reserve(B)
        sc, rk = self.sc.batch(points, offsets)
        self._sc_parts.append(sc)
        self._rk_parts.append(rk)
        self.curr_node_idx += B

    def add_node(self, pc):
        _check_cloud("ScanContextManager.add_node", pc)
        self.add_nodes(pc, np.array([0, pc.shape[0]], dtype=np.int64))

    @property
    def scancontexts(self) -> torch.Tensor:
        """(nodes, R, S) device tensor"""
        if len(self._sc_parts) > 1:
            self._sc_parts, self._rk_parts = [torch.cat(self._sc_parts)], [torch.cat(self._rk_parts)]
        return self._sc_parts[0]

    @property
    def ringkeys(self) -> torch.Tensor:
        """(nodes, R) device tensor"""
        self.scancontexts
        return self._rk_parts[0]

    def _eligible(self, k):
        _check_k(k)
        if self.curr_node_idx <= 0:
            raise ValueError("Empty database")
        m = self.curr_node_idx if self.include_last_node else self.curr_node_idx - 1
        if k > m:
            raise ValueError(f"ScanContextManager: k = {k} exceeds the {m} searchable nodes")
        return m

    def query_descriptors(self, query_sc, query_rk, k=1, reranking=True):
        """the search from descriptors on: (Q, R, S), (Q, R) -> (nn_ndx, sc_dist, sc_yaw_diff), each (Q, k) on the device"""
        m = self._eligible(k)
        cand, _ = knn(query_rk, self.ringkeys[:m], int(k))
        if not reranking:
            return cand, None, None
        dist, yaw = distance_pairs(query_sc, self.scancontexts, cand)
        return rerank(dist, yaw, cand)

    def query_batch(self, points, offsets, k=1, reranking=True):
        _check_cloud("ScanContextManager.query_batch", points)
        _check_offsets("ScanContextManager.query_batch", offsets)
        self._eligible(k)
        qsc, qrk = self.sc.batch(points, offsets)
        return self.query_descriptors(qsc, qrk, k, reranking)

    def query(self, query_pc, k=1, reranking=True):
        """[SYNC] copies the result back"""
        _check_cloud("ScanContextManager.query", query_pc)
        nn, dist, yaw = self.query_batch(query_pc, np.array([0, query_pc.shape[0]], dtype=np.int64), k, reranking)
        if not reranking:
            return nn[0].cpu().numpy(), None, None
        return nn[0].cpu().numpy(), dist[0].cpu().numpy(), yaw[0].cpu().numpy()


def evaluate(map_clouds: Sequence, query_clouds: Sequence, map_positions, query_positions, radius: Sequence[float], k: int = 50,
             reranking: bool = True, query_indexes: Optional[Sequence[int]] = None, include_last_node: bool = False,
             **manager_args) -> Dict:
    """evaluate_scan_context.py:24-84 from the loaded clouds on: {'recall1': {r: [recall@1 .. recall@k]}}.  map_clouds /
    query_clouds: per-scan (n, 3) arrays; positions (n, 2 or 3) in float64 (a common origin is subtracted in float64 before
    the device sees them, as retrieval.recall_at_k does); query_indexes = the reference's random sample of queries, all
    queries when None."""
    _check_k(k)
    for c in list(map_clouds) + list(query_clouds):
        _check_cloud("evaluate", c)
    if len(map_clouds) != len(map_positions) or len(query_clouds) != len(query_positions):
        raise ValueError("evaluate: one position per cloud")
    dev = _lib.require_gpu()
    lib = _lib.load()
    man = ScanContextManager(include_last_node=include_last_node, max_capacity=max(100000, len(map_clouds) + 1), **manager_args)
    for lo in range(0, len(map_clouds), _CHUNK):
        man.add_nodes(*_concat_clouds(map_clouds[lo:lo + _CHUNK], dev))
    sel = list(range(len(query_clouds))) if query_indexes is None else [int(i) for i in query_indexes]
    parts = []
    for lo in range(0, len(sel), _CHUNK):
        pts, off = _concat_clouds([query_clouds[i] for i in sel[lo:lo + _CHUNK]], dev)
        parts.append(man.query_batch(pts, off, k, reranking)[0])
    idx = torch.cat(parts).contiguous() if parts else torch.zeros((0, k), dtype=torch.int32, device=dev)
    mp64 = torch.as_tensor(np.asarray(map_positions, dtype=np.float64))
    qp64 = torch.as_tensor(np.asarray(query_positions, dtype=np.float64)).reshape(len(query_clouds), -1)
    origin = mp64.mean(dim=0, keepdim=True)
    mp = (mp64 - origin).to(device=dev, dtype=torch.float32).contiguous()
    qp = (qp64 - origin)[sel].to(device=dev, dtype=torch.float32).contiguous()
    rad = torch.tensor([float(r) for r in radius], dtype=torch.float32, device=dev)
    tp = torch.empty((len(radius), k), dtype=torch.int32, device=dev)
    _lib.call(dev, lib.egonn_recall_counts, idx.data_ptr() if len(sel) else None, qp.data_ptr(), mp.data_ptr(), len(sel), k,
              mp.shape[1], rad.data_ptr(), len(radius), tp.data_ptr())
    n = max(len(sel), 1)
    tpl = tp.cpu().tolist()
    return {'recall1': {r: [c / n for c in tpl[i]] for i, r in enumerate(radius)}, 'nn_index': idx}
