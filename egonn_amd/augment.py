"""Training augmentation on the device, with the reference's names (datasets/augmentation.py).

`TrainTransform(aug_mode)` / `TrainSetTransform(aug_mode)` and the individual transform classes take the reference's
arguments with the reference's defaults.  Called on one (n,3) cloud they behave like the reference's call sites (a CPU
input is staged through the GPU and comes back on its own device); the batched form
`t(points (N,3), offsets, scan_ids, draw)` returns `(points, offsets)` for scans that are resident.  Every draw is a
pure function of (seed, draw, scan id, point index, slot): egonn_amd/csrc/augment.hip spells it out.  `TrainBatcher`
does what datasets/dataset_utils.py:make_collate_fn does for resident scans and hands `TrainStep` its batch.

What the reference never configures is refused: max_theta2, random axes, JitterPoints(p < 1), RandomScale, RandomShear.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

JITTER, REMOVE_POINTS, TRANSLATE, ROTATE, BLOCK, SET_ROTATE, FLIP, RIGID, JITTER_CLIP = 1, 2, 4, 8, 16, 32, 64, 128, 256
STATUS_BAD_ID = 1
TILE, SELECT_WG, BOX_CHUNKS, BOX_WG = 256, 1024, 16, 256      # launch geometry of augment.hip (AUG_TILE, AUG_SEL_WG, ...)
MAX_DRAW, MAX_ID, MAX_POINTS = 1 << 14, 1 << 22, 1 << 24      # the fields of the draw counter
REC_I, REC_D = 8, 32


class _CParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("draw", C.c_uint32), ("set_id", C.c_uint32), ("stages", C.c_uint32),
                ("reserved", C.c_uint32), ("sigma", C.c_double), ("clip", C.c_double), ("r_min", C.c_double),
                ("r_max", C.c_double), ("max_delta", C.c_double), ("max_theta", C.c_double), ("block_p", C.c_double),
                ("scale_lo", C.c_double), ("scale_hi", C.c_double), ("ratio_lo", C.c_double), ("ratio_hi", C.c_double),
                ("set_max_theta", C.c_double), ("flip_cum", C.c_double * 3), ("rot_max", C.c_double),
                ("trans_max", C.c_double)]


@dataclass
class AugmentParams:
    """every parameter of the three call sites; the defaults are the reference's (TrainTransform / TrainSetTransform)"""
    seed: int = 0
    stages: int = 0
    sigma: float = 0.1
    clip: Optional[float] = 0.2
    r_min: float = 0.0
    r_max: float = 0.1
    max_delta: float = 0.3
    max_theta: float = 180.0
    block_p: float = 0.4
    scale: Sequence[float] = (0.02, 0.33)
    ratio: Sequence[float] = (0.3, 3.3)
    set_max_theta: float = 5.0
    flip_p: Sequence[float] = (0.25, 0.25, 0.0)
    rot_max: float = 0.0
    trans_max: float = 0.0

    def c_struct(self, draw: int, set_id: int) -> _CParams:
        if not (0 <= int(draw) < MAX_DRAW):
            raise ValueError(f"augment: draw {draw} does not fit the 14 bits of the draw counter")
        if not (0 <= int(set_id) < MAX_ID):
            raise ValueError(f"augment: set_id {set_id} does not fit its 22 bits")
        stages = int(self.stages) & ~JITTER_CLIP
        if self.clip is not None and stages & JITTER:
            stages |= JITTER_CLIP
        cum = np.cumsum(np.asarray(self.flip_p, np.float64))
        return _CParams(int(self.seed) & (2 ** 64 - 1), int(draw), int(set_id), stages, 0, float(self.sigma),
                        float(self.clip if self.clip is not None else 0.0), float(self.r_min), float(self.r_max),
                        float(self.max_delta), float(self.max_theta), float(self.block_p), float(self.scale[0]),
                        float(self.scale[1]), float(self.ratio[0]), float(self.ratio[1]), float(self.set_max_theta),
                        (C.c_double * 3)(*[float(v) for v in cum]), float(self.rot_max), float(self.trans_max))


@dataclass
class AugmentResult:
    points: torch.Tensor
    T_out: Optional[torch.Tensor] = None
    rec_i: Optional[torch.Tensor] = None      # (B, 8) int32, see include/egonn_hip.h
    rec_d: Optional[torch.Tensor] = None      # (B, 32) float64
    flags: Optional[torch.Tensor] = None      # (N,) uint8: bit 0 removed, bit 1 erased


def check_scan_ids(scan_ids) -> None:
    """host-side ids (a list, an array, a CPU tensor) are checked before the launch; device ids are checked by the kernel,
    which marks the scan in the record (STATUS_BAD_ID) and fills its points with NaN"""
    if scan_ids is None or (isinstance(scan_ids, torch.Tensor) and scan_ids.is_cuda):
        return
    a = np.asarray(scan_ids, dtype=np.int64)
    if a.size and (a.min() < 0 or a.max() >= MAX_ID):
        raise ValueError(f"augment: scan ids must fit 22 bits, got [{a.min()}, {a.max()}]")


def scratch_bytes(n: int, batch_size: int) -> int:
    v = _lib.load().egonn_augment_scratch_bytes(int(n), int(batch_size))
    if v < 0:
        raise ValueError(f"augment: bad shape (n={n} must be below 2^24 = the draw's point field, batch_size={batch_size})")
    return v


def augment_points(points: torch.Tensor, offsets: torch.Tensor, scan_ids: Optional[torch.Tensor], params: AugmentParams,
                   draw: int = 0, set_id: int = 0, T_in: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                   record: bool = False, flags: bool = False, scratch: Optional[torch.Tensor] = None) -> AugmentResult:
    """egonn_augment_points on device tensors: points (N,3) f32 (N is a capacity), offsets (B+1,) int64, scan_ids (B,) int32 or
    None, all on the device.  No host synchronisation; capturable when `out` and `scratch` are given."""
    lib = _lib.load()
    assert points.is_cuda and points.dtype == torch.float32 and points.is_contiguous() and points.dim() == 2 and points.shape[1] == 3
    assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.numel() >= 2
    dev = points.device
    B, N = offsets.numel() - 1, points.shape[0]
    if scan_ids is not None:
        assert scan_ids.is_cuda and scan_ids.dtype == torch.int32 and scan_ids.numel() == B
    cp = params.c_struct(draw, set_id)
    need = scratch_bytes(N, B)
    if scratch is None:
        scratch = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    sp = (scratch.data_ptr() + 255) & ~255
    assert scratch.is_cuda and sp + need <= scratch.data_ptr() + scratch.numel(), "augment: scratch too small"
    if out is None:
        out = torch.empty_like(points)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == points.shape
    T_out = None
    if cp.stages & RIGID:
        T_out = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
        if T_in is not None:
            T_in = T_in.to(device=dev, dtype=torch.float32).contiguous()
            assert T_in.shape == (B, 4, 4)
    ri = torch.zeros((B, REC_I), dtype=torch.int32, device=dev) if record else None
    rd = torch.zeros((B, REC_D), dtype=torch.float64, device=dev) if record else None
    fl = torch.zeros((N,), dtype=torch.uint8, device=dev) if flags else None
    _lib.call(dev, lib.egonn_augment_points, points.data_ptr(), N, offsets.data_ptr(), B, _lib._ptr(scan_ids), C.byref(cp),
              _lib._ptr(T_in) if T_out is not None else None, out.data_ptr(), _lib._ptr(T_out), _lib._ptr(ri), _lib._ptr(rd),
              _lib._ptr(fl), sp, need)
    return AugmentResult(out, T_out, ri, rd, fl)


# ------------------------------------------------------------------ the reference's classes
class _Transform:
    """a set of stages and their parameters; `+`-free composition happens in Compose"""
    per_batch = False

    def __init__(self, seed: int = 0):
        self.seed = int(seed)
        self._calls = 0

    def fill(self, p: AugmentParams) -> None:           # pragma: no cover - overridden
        raise NotImplementedError

    def params(self) -> AugmentParams:
        p = AugmentParams(seed=self.seed)
        self.fill(p)
        return p

    def __call__(self, e, offsets=None, scan_ids=None, draw: int = 0, set_id: Optional[int] = None):
        """one (n,3) cloud -> the cloud (every call is a new draw: scan id = number of calls so far); or the batched form
        (points (N,3), offsets, scan_ids, draw) -> (points, offsets) on resident tensors"""
        if offsets is None:
            pc = e if isinstance(e, torch.Tensor) else torch.as_tensor(np.asarray(e))
            assert pc.dim() == 2 and pc.shape[1] == 3
            dev = _lib.require_gpu()
            x = pc.to(device=dev, dtype=torch.float32).contiguous()
            call = self._calls
            self._calls += 1
            sid, dr = call % MAX_ID, (call // MAX_ID) % MAX_DRAW
            off = torch.tensor([0, x.shape[0]], dtype=torch.int64, device=dev)
            ids = torch.tensor([sid], dtype=torch.int32, device=dev)
            res = augment_points(x, off, ids, self.params(), draw=dr, set_id=sid)
            return res.points.to(device=pc.device, dtype=pc.dtype if pc.dtype.is_floating_point else torch.float32)
        dev = e.device
        check_scan_ids(scan_ids)
        off = torch.as_tensor(offsets).to(device=dev, dtype=torch.int64)
        ids = None if scan_ids is None else torch.as_tensor(scan_ids).to(device=dev, dtype=torch.int32)
        res = augment_points(e, off, ids, self.params(), draw=draw, set_id=draw if set_id is None else set_id)
        return res.points, offsets


class Compose(_Transform):
    """the transforms of one call site, in the reference's order, as ONE launch sequence"""
    ORDER = (JITTER, REMOVE_POINTS, TRANSLATE, ROTATE, BLOCK, SET_ROTATE, FLIP)

    def __init__(self, transforms, seed: int = 0):
        super().__init__(seed)
        self.transforms = list(transforms)
        seen = [t.stage for t in self.transforms]
        if sorted(seen, key=self.ORDER.index) != seen or len(set(seen)) != len(seen):
            raise NotImplementedError("augment: the device applies the stages in the reference's order, each at most once: "
                                      "jitter, remove points, translation, rotation, remove block | set rotation, flip")

    def fill(self, p: AugmentParams) -> None:
        for t in self.transforms:
            t.fill(p)


class JitterPoints(_Transform):
    stage = JITTER

    def __init__(self, sigma=0.01, clip=None, p=1., seed: int = 0):
        super().__init__(seed)
        if not sigma > 0 or (clip is not None and clip < 0):
            raise ValueError(f"JitterPoints: sigma {sigma} must be positive and clip {clip} non-negative or None")
        if p != 1:
            if 0 < p < 1:
                raise NotImplementedError("JitterPoints(p < 1) is not used by the reference's configurations and is not built")
            raise ValueError(f"JitterPoints: p {p} is not a probability above zero")
        self.sigma, self.clip, self.p = float(sigma), clip, 1.0

    def fill(self, p):
        p.stages |= JITTER
        p.sigma, p.clip = self.sigma, self.clip


class RemoveRandomPoints(_Transform):
    stage = REMOVE_POINTS

    def __init__(self, r, seed: int = 0):
        super().__init__(seed)
        # a range (lo, hi) or one fixed ratio, which is the range (r, r): r_min + 0 * u
        lo, hi = (float(v) for v in (r if np.ndim(r) else (r, r)))
        if not 0.0 <= lo <= hi <= 1.0:
            raise ValueError(f"RemoveRandomPoints: the ratio range ({lo}, {hi}) must be ascending inside [0, 1]")
        self.r_min, self.r_max = lo, hi

    def fill(self, p):
        p.stages |= REMOVE_POINTS
        p.r_min, p.r_max = self.r_min, self.r_max


class RandomTranslation(_Transform):
    stage = TRANSLATE

    def __init__(self, max_delta=0.05, seed: int = 0):
        super().__init__(seed)
        self.max_delta = max_delta

    def fill(self, p):
        p.stages |= TRANSLATE
        p.max_delta = self.max_delta


class RandomRotation(_Transform):
    """about z only; per_batch=True is the TrainSetTransform use (one draw for the whole batch)"""

    def __init__(self, axis=None, max_theta=180, max_theta2=None, per_batch: bool = False, seed: int = 0):
        super().__init__(seed)
        if max_theta2 is not None:
            raise NotImplementedError("RandomRotation(max_theta2) is not used by the reference's configurations and is not built")
        if axis is None:
            raise NotImplementedError("RandomRotation about a random axis is not used by the reference's configurations")
        a = np.asarray(axis, np.float64).reshape(-1)
        if a.shape != (3,) or a[0] != 0 or a[1] != 0 or not a[2] > 0:
            raise NotImplementedError("RandomRotation: only the +z axis is built (the reference's configurations)")
        self.axis, self.max_theta, self.per_batch = axis, max_theta, per_batch
        self.stage = SET_ROTATE if per_batch else ROTATE

    def fill(self, p):
        p.stages |= self.stage
        if self.per_batch:
            p.set_max_theta = self.max_theta
        else:
            p.max_theta = self.max_theta


class RemoveRandomBlock(_Transform):
    stage = BLOCK

    def __init__(self, p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), seed: int = 0):
        super().__init__(seed)
        self.p, self.scale, self.ratio = p, scale, ratio

    def fill(self, p):
        p.stages |= BLOCK
        p.block_p, p.scale, p.ratio = self.p, tuple(self.scale), tuple(self.ratio)


class RandomFlip(_Transform):
    stage = FLIP
    per_batch = True

    def __init__(self, p, seed: int = 0):
        super().__init__(seed)
        probs = tuple(float(v) for v in p)
        total = float(np.sum(probs))
        if len(probs) != 3 or min(probs) < 0 or not 0 < total <= 1:
            raise ValueError(f"RandomFlip: one probability per axis, none negative, together in (0, 1]; got {probs}")
        self.p = probs

    def fill(self, p):
        p.stages |= FLIP
        p.flip_p = tuple(self.p)


class RandomScale:
    def __init__(self, *a, **k):
        raise NotImplementedError("RandomScale is not used by the reference's configurations and is not built")


class RandomShear:
    def __init__(self, *a, **k):
        raise NotImplementedError("RandomShear is not used by the reference's configurations and is not built")


_Z = (0.0, 0.0, 1.0)
# aug_mode -> the stages of the two call sites; mode 2 turns every scan fully and leaves the batch unturned
_SCAN_ROTATION = {1: None, 2: 180}
_SET_ROTATION = {1: 5, 2: None}


def _known_mode(aug_mode) -> None:
    if aug_mode not in _SCAN_ROTATION:
        raise NotImplementedError(f"aug_mode {aug_mode!r}: the modes are {sorted(_SCAN_ROTATION)}")


class TrainTransform(Compose):
    def __init__(self, aug_mode, seed: int = 0):
        _known_mode(aug_mode)
        self.aug_mode = aug_mode
        t = [JitterPoints(sigma=0.1, clip=0.2), RemoveRandomPoints(r=(0.0, 0.1)), RandomTranslation(max_delta=0.3)]
        if _SCAN_ROTATION[aug_mode] is not None:
            t.append(RandomRotation(axis=_Z, max_theta=_SCAN_ROTATION[aug_mode]))
        t.append(RemoveRandomBlock(p=0.4))
        super().__init__(t, seed)


class TrainSetTransform(Compose):
    per_batch = True

    def __init__(self, aug_mode, seed: int = 0):
        _known_mode(aug_mode)
        self.aug_mode = aug_mode
        t = [RandomFlip((0.25, 0.25, 0.0))]
        if _SET_ROTATION[aug_mode] is not None:
            t.insert(0, RandomRotation(axis=_Z, max_theta=_SET_ROTATION[aug_mode], per_batch=True))
        super().__init__(t, seed)


class RigidPerturbation(_Transform):
    """datasets/mulran/mulran_train.py:41-50: a z-rotation uniform in +-rot_max (radians) and an xy translation uniform in
    +-trans_max, applied like misc/poses.py:apply_transform; `perturb` also returns m @ transform per scan"""
    stage = RIGID

    def __init__(self, rot_max: float = 0., trans_max: float = 0., seed: int = 0):
        super().__init__(seed)
        self.rot_max, self.trans_max = rot_max, trans_max

    def fill(self, p):
        p.stages |= RIGID
        p.rot_max, p.trans_max = self.rot_max, self.trans_max

    def perturb(self, points, offsets, scan_ids, transforms, draw: int = 0):
        check_scan_ids(scan_ids)
        dev = points.device
        off = torch.as_tensor(offsets).to(device=dev, dtype=torch.int64)
        ids = None if scan_ids is None else torch.as_tensor(scan_ids).to(device=dev, dtype=torch.int32)
        res = augment_points(points, off, ids, self.params(), draw=draw, T_in=transforms)
        return res.points, res.T_out


# ------------------------------------------------------------------ collate for resident scans
class TrainBatcher:
    """make_collate_fn (datasets/dataset_utils.py:60-95) for scans that are on the device: per-scan transform -> set transform
    (one launch sequence) -> the quantiser path (Context.voxelize) -> {'coords', 'features', 'batch_size'} for TrainStep.
    `local` is make_collate_fn_6DOF (:98-149) with the positive cloud's rigid perturbation."""

    def __init__(self, quantizer, aug_mode: Optional[int] = 1, seed: int = 0, set_transform: bool = True,
                 rot_max: float = 0., trans_max: float = 0.):
        self.quantizer = quantizer
        self.transform = TrainTransform(aug_mode, seed) if aug_mode else None
        self.set_transform = TrainSetTransform(aug_mode, seed) if (aug_mode and set_transform) else None
        self.rigid = RigidPerturbation(rot_max, trans_max, seed)
        self.seed = int(seed)
        self.ctx = quantizer._context()
        self.last: Optional[AugmentResult] = None

    def params(self) -> AugmentParams:
        p = AugmentParams(seed=self.seed)
        for t in (self.transform, self.set_transform):
            if t is not None:
                t.fill(p)
        return p

    def _quantize(self, pts: torch.Tensor, offsets: Sequence[int]):
        self.ctx.voxelize(pts, offsets, self.quantizer.mode, self.quantizer.step)
        coords = self.ctx.level_coords(0)
        return {"coords": coords, "features": torch.ones((coords.shape[0], 1), dtype=torch.float32, device=coords.device),
                "batch_size": len(offsets) - 1}

    def augment(self, points: torch.Tensor, offsets: Sequence[int], scan_ids, draw: int = 0, set_id: int = 0,
                record: bool = False) -> AugmentResult:
        check_scan_ids(scan_ids)
        dev = points.device
        off = torch.as_tensor(np.asarray(offsets, np.int64)).to(dev)
        ids = torch.as_tensor(np.asarray(scan_ids, np.int32)).to(dev)
        p = self.params()
        if p.stages == 0:
            return AugmentResult(points)
        self.last = augment_points(points, off, ids, p, draw=draw, set_id=set_id, record=record, flags=record)
        return self.last

    def __call__(self, points: torch.Tensor, offsets: Sequence[int], scan_ids, draw: int = 0, set_id: int = 0):
        """points (N,3) f32 on the device, offsets a HOST sequence (the quantiser path takes host offsets)"""
        return self._quantize(self.augment(points, offsets, scan_ids, draw, set_id).points, [int(o) for o in offsets])

    def local(self, anc_points, anc_offsets, pos_points, pos_offsets, scan_ids, transforms, draw: int = 0):
        """the 6-DoF batch: the positive clouds are perturbed, T_gt = m @ transform; anchors pass unchanged"""
        pos, T_gt = self.rigid.perturb(pos_points, np.asarray(pos_offsets, np.int64), scan_ids, transforms, draw)
        anc_batch = dict(self._quantize(anc_points, [int(o) for o in anc_offsets]))
        pos_batch = dict(self._quantize(pos, [int(o) for o in pos_offsets]))
        lens = [[int(anc_offsets[b + 1] - anc_offsets[b]), int(pos_offsets[b + 1] - pos_offsets[b])]
                for b in range(len(anc_offsets) - 1)]
        return {"anc_pcd": anc_points, "pos_pcd": pos, "anc_batch": anc_batch, "pos_batch": pos_batch, "T_gt": T_gt,
                "len_batch": lens}
