"""Seeded synthetic inputs for benchmarks and parity tests (no datasets or pretrained weights
exist in this environment — SURVEY.md §0).

* `lidar_scan`  — the LiDAR-like generator SURVEY.md §8(d) specifies for configs C1/C2
  (64 beams x 2048 azimuth steps, elevation -24.8..+2.0 deg, sensor height 1.73 m, ground
  plane + 60 random axis-aligned boxes, range < 80 m, sigma = 0.02 m noise, subsampled to an
  exact point count).  It must NOT be replaced by the uniform-box generator of the
  reference's `datasets/quantization.py:107-111`: at 0.1 m that yields isolated voxels.
* `seeded_state_dict` — deterministic weights for a given key/shape table, independent of
  any reference code, so fixtures only need to store (seed, outputs).
"""
from __future__ import annotations

import zlib
from typing import Dict, Tuple

import numpy as np


def lidar_scan(seed: int, n_points: int = 50_000, n_beams: int = 64, n_azimuth: int = 2048,
               max_range: float = 80.0, sensor_height: float = 1.73, n_boxes: int = 60,
               noise_sigma: float = 0.02) -> np.ndarray:
    """(n_points, 3) float32 point cloud in the sensor frame (z up, ground at z = -sensor_height)."""
    rng = np.random.default_rng(seed)
    elev = np.deg2rad(np.linspace(-24.8, 2.0, n_beams))
    azim = np.linspace(-np.pi, np.pi, n_azimuth, endpoint=False)
    el, az = np.meshgrid(elev, azim, indexing="ij")
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=-1).reshape(-1, 3)

    t = np.full(d.shape[0], np.inf)
    # ground plane z = -sensor_height
    down = d[:, 2] < -1e-6
    t[down] = -sensor_height / d[down, 2]

    # random axis-aligned boxes standing on the ground
    centres = rng.uniform(-70.0, 70.0, size=(n_boxes, 2))
    sizes_xy = rng.uniform(2.0, 25.0, size=(n_boxes, 2))
    heights = rng.uniform(1.5, 15.0, size=n_boxes)
    for c, s, h in zip(centres, sizes_xy, heights):
        lo = np.array([c[0] - s[0] / 2, c[1] - s[1] / 2, -sensor_height])
        hi = np.array([c[0] + s[0] / 2, c[1] + s[1] / 2, -sensor_height + h])
        if lo[0] <= 0.0 <= hi[0] and lo[1] <= 0.0 <= hi[1]:
            continue                                   # box covers the sensor: skipped
        with np.errstate(divide="ignore", invalid="ignore"):
            t0 = lo / d
            t1 = hi / d
        tmin = np.nanmax(np.minimum(t0, t1), axis=1)
        tmax = np.nanmin(np.maximum(t0, t1), axis=1)
        hit = (tmax >= tmin) & (tmin > 0.0)
        t = np.where(hit & (tmin < t), tmin, t)

    keep = np.isfinite(t) & (t < max_range)
    pts = d[keep] * t[keep, None]
    pts = pts + rng.normal(0.0, noise_sigma, size=pts.shape)
    if pts.shape[0] >= n_points:
        sel = rng.choice(pts.shape[0], size=n_points, replace=False)
    else:                                              # rare (tiny configs): sample with replacement + jitter
        sel = rng.choice(pts.shape[0], size=n_points, replace=True)
        pts = pts + 0.0
    pts = pts[sel]
    return np.ascontiguousarray(pts, dtype=np.float32)


def _key_seed(seed: int, key: str) -> int:
    return (int(seed) * 1_000_003 + zlib.crc32(key.encode())) & 0x7FFFFFFF


def seeded_tensor(seed: int, key: str, shape: Tuple[int, ...]) -> np.ndarray:
    """Deterministic fp32 tensor for a state_dict entry.  Distribution by key suffix:
    conv kernels / linear weights ~ N(0, sqrt(2/fan)), BN weight ~ U(0.5,1.5), BN bias and
    running_mean ~ N(0,0.1), running_var ~ U(0.5,1.5), linear bias ~ N(0,0.05), GeM p = 3; NetVLAD cluster / hidden
    matrices ~ N(0,1)/sqrt(C), gate ~ N(0,1)/sqrt(D), its bn1 / bn2 weight ~ U(0.5,1.5) and bias ~ N(0,0.1); SELayer.fc
    weights ~ N(0, 3 sqrt(2/fan)) and biases ~ N(0,0.3)."""
    rng = np.random.default_rng(_key_seed(seed, key))
    shape = tuple(int(s) for s in shape)
    if key.endswith("num_batches_tracked"):
        return np.zeros(shape, dtype=np.int64)
    if key.endswith("pooling.p"):
        return np.full(shape, 3.0, dtype=np.float32)
    if key.endswith(".kernel"):
        if len(shape) == 3:
            fan = shape[0] * shape[1]                  # K * Cin
        else:
            fan = shape[0]
        return (rng.standard_normal(shape) * np.sqrt(2.0 / fan)).astype(np.float32)
    if key.endswith("eca.conv.weight"):
        return rng.uniform(-0.8, 0.8, size=shape).astype(np.float32)
    if key.endswith("running_var"):
        return rng.uniform(0.5, 1.5, size=shape).astype(np.float32)
    if key.endswith("running_mean"):
        return (rng.standard_normal(shape) * 0.1).astype(np.float32)
    if key.endswith("bn.weight"):
        return rng.uniform(0.5, 1.5, size=shape).astype(np.float32)
    if key.endswith("bn.bias"):
        return (rng.standard_normal(shape) * 0.1).astype(np.float32)
    # NetVLADLoupe / GatingContext (reference layers/netvlad.py:26-29,89-90 init scale): randn / sqrt(C), C = feature size
    if key.endswith("cluster_weights"):
        return (rng.standard_normal(shape) / np.sqrt(shape[0])).astype(np.float32)
    if key.endswith("cluster_weights2"):
        return (rng.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32)
    if key.endswith("hidden1_weights"):
        return (rng.standard_normal(shape) / np.sqrt(shape[0] // 64)).astype(np.float32)   # (C * 64 clusters, D)
    if key.endswith("gating_weights"):
        return (rng.standard_normal(shape) / np.sqrt(shape[0])).astype(np.float32)         # (D, D)
    if key.endswith(("bn1.weight", "bn2.weight")):
        return rng.uniform(0.5, 1.5, size=shape).astype(np.float32)
    if key.endswith(("bn1.bias", "bn2.bias")):
        return (rng.standard_normal(shape) * 0.1).astype(np.float32)
    # SELayer.fc (layers/senet_block.py:39-43): three times the linear rule and biases of 0.3, so that the sigmoid gates of a
    # seeded model spread over 0.3 .. 0.7 and beyond instead of sitting at 0.5 (tests/golden/make_golden_se.py checks it)
    if ".se.fc." in key and key.endswith("linear.weight"):
        return (rng.standard_normal(shape) * 3.0 * np.sqrt(2.0 / shape[1])).astype(np.float32)
    if ".se.fc." in key and key.endswith("linear.bias"):
        return (rng.standard_normal(shape) * 0.3).astype(np.float32)
    if key.endswith("linear.weight"):
        return (rng.standard_normal(shape) * np.sqrt(2.0 / shape[1])).astype(np.float32)
    if key.endswith("linear.bias"):
        return (rng.standard_normal(shape) * 0.05).astype(np.float32)
    raise KeyError(f"no seeded distribution for state_dict key {key!r}")


def seeded_state_dict(seed: int, shapes: Dict[str, Tuple[int, ...]]) -> Dict[str, np.ndarray]:
    return {k: seeded_tensor(seed, k, s) for k, s in shapes.items()}


# ------------------------------------------------------------------ keypoint sets with a planted pose (registration tests / timing)
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def rot_zyx(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def planted_keypoint_pair(n, seed, outliers, noise=0.05, D=128, n2=None, desc_noise=0.02):
    """source keypoints in a +-80 m box (z +-10), target = T_gt source + noise, a share `outliers` of the target replaced by
    unrelated points with unrelated descriptors, the target order shuffled.  -> f1, f2, k1, k2 (float32), T_gt (4,4) float64"""
    rng = np.random.default_rng(seed)
    src = rng.uniform([-80, -80, -10], [80, 80, 10], size=(n, 3))
    R = rot_zyx(rng.uniform(-np.pi, np.pi), np.deg2rad(rng.uniform(-3, 3)), np.deg2rad(rng.uniform(-3, 3)))
    t = _unit(rng.standard_normal(3)) * rng.uniform(0, 20)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    tgt = src @ R.T + t + noise * rng.standard_normal((n, 3))
    base = _unit(rng.standard_normal((n, D)))
    d1 = _unit(base + desc_noise * rng.standard_normal((n, D)))
    d2 = _unit(base + desc_noise * rng.standard_normal((n, D)))
    out = rng.choice(n, size=int(round(outliers * n)), replace=False)
    tgt[out] = rng.uniform([-80, -80, -10], [80, 80, 10], size=(len(out), 3))
    d2[out] = _unit(rng.standard_normal((len(out), D)))
    perm = rng.permutation(n)
    tgt, d2 = tgt[perm], d2[perm]
    if n2 is not None:
        tgt, d2 = tgt[:n2], d2[:n2]
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)      # noqa: E731
    return f32(d1), f32(d2), f32(src), f32(tgt), T


def pad_keypoint_pairs(pairs, n_max=None, D=None):
    """list of (f1, f2, k1, k2, ...) -> padded float32 arrays (P, n_max, .) and int32 counts"""
    n_max = n_max or max(max(len(p[0]), len(p[1])) for p in pairs)
    D = D or pairs[0][0].shape[1]
    P = len(pairs)
    F1, F2 = np.zeros((P, n_max, D), np.float32), np.zeros((P, n_max, D), np.float32)
    K1, K2 = np.zeros((P, n_max, 3), np.float32), np.zeros((P, n_max, 3), np.float32)
    n1, n2 = np.zeros(P, np.int32), np.zeros(P, np.int32)
    for i, p in enumerate(pairs):
        n1[i], n2[i] = len(p[0]), len(p[1])
        F1[i, :n1[i]], F2[i, :n2[i]], K1[i, :n1[i]], K2[i, :n2[i]] = p[0], p[1], p[2], p[3]
    return F1, F2, K1, K2, n1, n2


# ------------------------------------------------------------------ scan pairs with a planted pose (ICP tests / timing)
def planted_scan_pair(seed, n_points, translation=(1.0, 0.5, 0.1), yaw_pitch_roll=(0.05, 0.01, 0.01), noise=0.02,
                      init_translation=(0.3, -0.2, 0.1), init_yaw_pitch_roll=(0.01, 0.0, 0.0)):
    """Two different subsamples of one `lidar_scan` scene: src = subsample A + noise, tgt = T_planted (subsample B) + noise
    (independent N(0, noise) per coordinate).  n_points: int or (n_src, n_tgt).  translation (m) and yaw_pitch_roll (rad)
    make T_planted; T_init = D T_planted with D the rigid motion of init_translation (m) / init_yaw_pitch_roll (rad) — the
    stated perturbation (zeros: T_init = T_planted).  -> src, tgt (float32), T_planted, T_init (4,4) float64."""
    n_src, n_tgt = (n_points, n_points) if np.isscalar(n_points) else n_points
    scene = lidar_scan(seed, n_points=int(1.6 * max(n_src, n_tgt))).astype(np.float64)
    rng = np.random.default_rng([seed, 0x1C9])
    a = scene[rng.choice(len(scene), size=n_src, replace=False)]
    b = scene[rng.choice(len(scene), size=n_tgt, replace=False)]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot_zyx(*yaw_pitch_roll), np.asarray(translation, dtype=np.float64)
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = rot_zyx(*init_yaw_pitch_roll), np.asarray(init_translation, dtype=np.float64)
    src = a + noise * rng.standard_normal(a.shape)
    tgt = b @ T[:3, :3].T + T[:3, 3] + noise * rng.standard_normal(b.shape)
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)      # noqa: E731
    return f32(src), f32(tgt), T, D @ T
