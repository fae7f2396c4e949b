"""Streaming ingest -> extract pipeline: raw scans in HOST memory (or `.bin` files) to descriptors, with the GPU kept busy.

This is the loop of the reference's evaluator (eval/evaluate.py:312-323: `for each scan: pc_loader(path); compute_embedding`)
re-built for throughput (BASELINE configs[4]): the reference reads one file, filters it on the CPU
(misc/point_clouds.py:95-111, datasets/mulran/mulran_raw.py:19-25), quantises on the CPU and runs one forward per scan.  Here

    reader threads    raw scans (n,4|3) f32 / `.bin` files -> one of S pinned staging buffers (memcpy / readinto: the
                      GIL is released, no per-scan Python tensor code)
    copy + compute    per slot, on the slot's own HIP stream: ONE H2D copy of the batch's raw payload (+ the B+1 raw
                      offsets), then ONE hipGraphLaunch of the captured step
                          egonn_filter_points (zero / ground-plane filter, compaction; writes the survivors' offsets ON THE
                          DEVICE) -> egonn_voxelize_device (reads them there) -> forward -> top-n_k
                      then the D2H copy of the (B,256) descriptors (and, optionally, keypoints / local descriptors) into the
                      slot's pinned result buffers
    consumer          waits for the slot's event, checks the plan flags, yields host tensors in submission order.

No host synchronisation sits between the file read and the results: S batches are in flight, the host only fills buffers
and launches.  A batch that overflows the reserved capacities (flagged by the library, never out of bounds) is re-run through
the eager exact-size path, so the results always equal `DescriptorExtractor.extract` on the filtered scans (bitwise: same
kernels, tests/test_gpu_parity.py::test_streaming_pipeline_equals_extract)."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .evaluator import DescriptorExtractor, GraphExtractor
from .ingest import GROUND_PLANE_LEVEL

Source = Union[np.ndarray, str]


class _Slot(GraphExtractor):
    """One batch in flight: pinned staging + device raw buffer + the captured filter -> voxelise -> forward -> select step."""

    def __init__(self, owner: "StreamingExtractor", slot: int):
        ex = owner.extractor
        super().__init__(ex, owner.batch_size, owner.max_points, owner.level_capacity, slot=200 + slot)
        self.owner = owner
        dev = self.ctx.device
        B, fpp = owner.batch_size, owner.floats_per_point
        self.h_raw = torch.empty(owner.max_points * fpp, dtype=torch.float32).pin_memory()
        self.h_raw_np = self.h_raw.numpy()
        self.h_raw_bytes = memoryview(self.h_raw_np).cast("B")
        self.h_off = torch.zeros(B + 1, dtype=torch.int64).pin_memory()
        self.d_raw = torch.zeros((owner.max_points, fpp), dtype=torch.float32, device=dev)
        self.d_raw_off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        self.scratch = torch.empty(self.ctx.lib.egonn_filter_points_scratch_ints(owner.max_points), dtype=torch.int32, device=dev)
        n_k, m = ex.n_k, ex.model
        self.h_global = torch.empty((B, m.global_descriptor_size), dtype=torch.float32).pin_memory()
        self.h_count = torch.empty((B,), dtype=torch.int32).pin_memory()
        self.h_kp = torch.empty((B, n_k, 3), dtype=torch.float32).pin_memory() if owner.keep_local else None
        self.h_desc = torch.empty((B, n_k, m.local_descriptor_size), dtype=torch.float32).pin_memory() if owner.keep_local else None
        self.done = torch.cuda.Event()
        self.n_real = 0

    # the captured step starts with the device filter: raw rows -> self.points / self.offsets (the graph's static inputs)
    def _enqueue(self):
        o, ctx = self.owner, self.ctx
        _lib.call(ctx.device, ctx.lib.egonn_filter_points, self.d_raw.data_ptr(), o.max_points, o.floats_per_point,
                  self.d_raw_off.data_ptr(), self.B, int(o.remove_zero_points), int(o.remove_ground_plane), o.ground,
                  self.points.data_ptr(), self.offsets.data_ptr(), self.scratch.data_ptr(), self.scratch.numel())
        super()._enqueue()

    def submit(self, n_rows: int, n_real: int):
        """the staging buffers hold a batch (n_rows raw rows, offsets in h_off): copy, launch, copy back — all asynchronous"""
        self.n_real = n_real
        fpp = self.owner.floats_per_point
        with torch.cuda.stream(self.stream):
            self.d_raw.view(-1)[: n_rows * fpp].copy_(self.h_raw[: n_rows * fpp], non_blocking=True)
            self.d_raw_off.copy_(self.h_off, non_blocking=True)
            if self.graph is None:
                self._enqueue()                            # eager once: grows every arena to its final size
                self.stream.synchronize()
                try:
                    self.ctx.plan_status()
                except _lib.CapacityError:                 # the slot's first batch already overflows the reservation: the
                    pass                                   # capture below is still valid (fixed capacities), the replay is
                                                           # flagged again and collect() takes the eager path
                g = _lib._P()
                _lib.check(self.ctx.lib.egonn_graph_begin(self.stream.cuda_stream))
                try:
                    self._enqueue()
                finally:
                    rc = self.ctx.lib.egonn_graph_end(self.stream.cuda_stream, _lib.C.byref(g))
                _lib.check(rc)
                self.graph = g
            _lib.check(self.ctx.lib.egonn_graph_launch(self.graph, self.stream.cuda_stream))
            out = self.out
            self.h_global.copy_(out["global"], non_blocking=True)
            self.h_count.copy_(out["count"], non_blocking=True)
            if self.owner.keep_local:
                self.h_kp.copy_(out["keypoints"], non_blocking=True)
                self.h_desc.copy_(out["descriptors"], non_blocking=True)
            self.done.record(self.stream)

    def collect(self) -> Dict[str, torch.Tensor]:
        self.done.synchronize()
        try:
            self.status()
        except _lib.CapacityError:
            return self._fallback()
        n = self.n_real
        res = {"global": self.h_global[:n].clone(), "count": self.h_count[:n].clone()}
        if self.owner.keep_local:
            res.update(keypoints=self.h_kp[:n].clone(), descriptors=self.h_desc[:n].clone())
        return res

    def _fallback(self) -> Dict[str, torch.Tensor]:
        """the batch did not fit the reservation: exact-size eager path on the filtered points (they are intact: the filter
        runs in front of the plan)"""
        self.owner.fallbacks += 1
        with torch.cuda.stream(self.stream):
            offs = self.offsets.tolist()
            out = self.ex.extract_packed(self.points[: offs[-1]], offs, slot=199)
            res = {k: out[k][: self.n_real].cpu() for k in ("global", "count")}
            if self.owner.keep_local:
                res.update(keypoints=out["keypoints"][: self.n_real].cpu(), descriptors=out["descriptors"][: self.n_real].cpu())
        return res


class StreamingExtractor:
    """extractor: DescriptorExtractor.  Batches of `batch_size` raw scans (host arrays (n, floats_per_point) f32 or `.bin`
    paths) -> descriptors, `slots` batches in flight.  Call `calibrate(sample)` (or pass level_capacity) before `run`."""

    def __init__(self, extractor: DescriptorExtractor, batch_size: int = 16, max_points_per_scan: int = 65536,
                 floats_per_point: int = 4, dataset_type: str = "mulran", remove_zero_points: bool = True,
                 remove_ground_plane: bool = True, slots: int = 4, workers: int = 8, level_capacity: Optional[Sequence[int]] = None,
                 keep_local: bool = True):
        assert floats_per_point in (3, 4)
        self.extractor = extractor
        self.batch_size = int(batch_size)
        self.max_points = int(batch_size) * int(max_points_per_scan)
        self.floats_per_point = floats_per_point
        self.ground = float(GROUND_PLANE_LEVEL[dataset_type])
        self.remove_zero_points, self.remove_ground_plane = remove_zero_points, remove_ground_plane
        self.n_slots = int(slots)
        self.level_capacity = list(level_capacity) if level_capacity is not None else None
        self.keep_local = keep_local
        self.pool = ThreadPoolExecutor(max_workers=max(1, workers))
        self.slots: List[_Slot] = []
        self.fallbacks = 0

    # ------------------------------------------------------------------ capacities
    def calibrate(self, sample: Sequence[Source], margin: float = 1.3):
        """level capacities from one representative batch of raw scans (eager ingest + exact plan)."""
        from .ingest import ScanIngest, read_bin
        raws = [read_bin(s) if isinstance(s, str) else np.ascontiguousarray(s, dtype=np.float32) for s in sample]
        ex = self.extractor
        ing = ScanIngest.__new__(ScanIngest)
        ing.ground, ing.remove_zero_points, ing.remove_ground_plane = self.ground, self.remove_zero_points, self.remove_ground_plane
        ing.device, ing._pinned = ex.model.context(0).device, None
        pts, off = ing(raws)
        self.level_capacity = ex.calibrate(pts, off, margin)
        return self.level_capacity

    # ------------------------------------------------------------------ host staging
    def _fill_one(self, slot: _Slot, src: Source, row0: int) -> None:
        fpp = self.floats_per_point
        if isinstance(src, str):
            with open(src, "rb", buffering=0) as f:
                n = os.path.getsize(src) // (4 * fpp)
                got = f.readinto(slot.h_raw_bytes[row0 * fpp * 4: (row0 + n) * fpp * 4])
                assert got == n * fpp * 4, src
        else:
            np.copyto(slot.h_raw_np[row0 * fpp: (row0 + len(src)) * fpp].reshape(len(src), fpp), src, casting="no")

    def _stage(self, slot: _Slot, batch: Sequence[Source]) -> int:
        fpp = self.floats_per_point
        rows = [os.path.getsize(s) // (4 * fpp) if isinstance(s, str) else len(s) for s in batch]
        off = np.zeros(self.batch_size + 1, dtype=np.int64)
        off[1: len(rows) + 1] = np.cumsum(rows)
        off[len(rows) + 1:] = off[len(rows)]               # a short last batch is padded with empty scans
        if int(off[-1]) > self.max_points:
            raise ValueError(f"batch of {int(off[-1])} raw points exceeds the staging capacity {self.max_points}")
        slot.h_off.numpy()[:] = off
        list(self.pool.map(lambda a: self._fill_one(slot, a[0], a[1]), zip(batch, off[:-1].tolist())))
        return int(off[-1])

    # ------------------------------------------------------------------ the pipeline
    def run(self, batches: Iterable[Sequence[Source]]) -> Iterator[Dict[str, torch.Tensor]]:
        """batches: iterable of lists (<= batch_size) of raw scans.  Yields, in order, host tensors: global (b,256),
        count (b,), and with keep_local keypoints (b,n_k,3), descriptors (b,n_k,128)."""
        if self.level_capacity is None:
            raise RuntimeError("StreamingExtractor: call calibrate(sample) or pass level_capacity first")
        self.extractor.model._sync_weights()
        if not self.slots:
            self.slots = [_Slot(self, i) for i in range(self.n_slots)]
        inflight: List[_Slot] = []
        i = 0
        try:
            for batch in batches:
                assert 1 <= len(batch) <= self.batch_size
                if len(inflight) == self.n_slots:
                    yield inflight.pop(0).collect()
                slot = self.slots[i % self.n_slots]
                i += 1
                n_rows = self._stage(slot, batch)
                slot.submit(n_rows, len(batch))
                inflight.append(slot)
            while inflight:
                yield inflight.pop(0).collect()
        finally:
            # a consumer that abandons the generator early leaves batches in flight: wait for them, so that the next
            # run() (which restarts at slot 0) never overwrites a pinned staging buffer a copy or graph still reads
            for slot in inflight:
                slot.done.synchronize()

    def close(self):
        self.pool.shutdown(wait=False)
