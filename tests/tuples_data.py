"""Numpy restatements of the rules of csrc/tuples.hip, the builders of the fixture's inputs (tests/golden/tuples_ref.npz,
written by tests/golden/make_golden_tuples.py from the reference's own functions) and the synthetic sequence of the
end-to-end test.  tests/test_tuples_host.py pins every restatement to the fixture; the GPU tests read the fixture and numpy
only."""
from __future__ import annotations

import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tuples_ref.npz")
TRAJECTORY_ROWS = (1, 63, 65, 257, 1150)        # off the tile (256) and the wave (64); 1150 = 1000 positions + a second pass
TRAJECTORY_RADII = (2.0, 10.0, 50.0)
LATTICE_RADIUS = 5.0
STATIONARY_RADIUS = 1.0
FILTER_RADIUS = 20.0
MASK_BATCHES = (4, 33, 130)
MASK_RADII = (2.0, 10.0)


def load_fixture():
    return np.load(FIXTURE)


# ------------------------------------------------------------------ restatements of the kernel rules
def radius_rows(query, ref, radius, exclude_self=False):
    """the fp64 rule, one rounding per operation: dx = qx - mx, dy = qy - my, dx*dx + dy*dy <= r*r; rows ascending.
    -> (offsets int64 (Q+1), indices int32)"""
    q, m = np.asarray(query, dtype=np.float64).reshape(-1, 2), np.asarray(ref, dtype=np.float64).reshape(-1, 2)
    r2 = np.float64(radius) * np.float64(radius)
    off, rows = np.zeros(len(q) + 1, dtype=np.int64), []
    with np.errstate(invalid="ignore"):
        for i in range(len(q)):
            dx, dy = q[i, 0] - m[:, 0], q[i, 1] - m[:, 1]
            hit = (dx * dx + dy * dy) <= r2
            if exclude_self:
                hit[i] = False
            rows.append(np.flatnonzero(hit).astype(np.int32))
            off[i + 1] = off[i] + len(rows[-1])
    return off, (np.concatenate(rows) if rows else np.zeros(0, np.int32))


def delta_encode(idx):
    """sorted rows stored as the differences of the flat index array (mostly +1: they deflate to little)"""
    d = np.diff(np.asarray(idx, dtype=np.int64), prepend=0)
    assert np.abs(d).max(initial=0) < 32768
    return d.astype(np.int16)


def fixture_rows(fx, key):
    """-> (offsets int64, indices int32) of a radius case of the fixture"""
    return fx[key + "_off"], np.cumsum(fx[key + "_didx"].astype(np.int64)).astype(np.int32)


def rows_of(off, idx):
    return [idx[off[i]: off[i + 1]] for i in range(len(off) - 1)]


def pair_masks(labels, pos_off, pos_idx, non_off, non_idx):
    """positives_mask[i][j] = l[j] in positives[l[i]], negatives_mask[i][j] = l[j] not in non_negatives[l[i]], each by
    np.searchsorted + equality; a label outside the tuples: row and column False in both"""
    labels = np.asarray(labels, dtype=np.int64)
    B, n = len(labels), len(pos_off) - 1
    pos, neg = np.zeros((B, B), dtype=bool), np.zeros((B, B), dtype=bool)

    def member(e, row):
        k = np.searchsorted(row, e)
        return k < len(row) and row[k] == e
    for i, li in enumerate(labels):
        for j, lj in enumerate(labels):
            if 0 <= li < n and 0 <= lj < n:
                pos[i, j] = member(lj, pos_idx[pos_off[li]: pos_off[li + 1]])
                neg[i, j] = not member(lj, non_idx[non_off[li]: non_off[li + 1]])
    return pos, neg


def relative_poses(poses, idx_a, idx_b, negate_translation, dtype=np.float64):
    """the device formula in `dtype`: adjugate / determinant inverse of R_b, R_b^-1 R_a, R_b^-1 (t_a - t_b) with the difference
    first, dot products summed left to right; -> (out (P,4,4), status (P,)): 1 bad last row, 2 singular, 4 bad index"""
    poses = np.asarray(poses)
    P, n = len(idx_a), len(poses)
    out = np.tile(np.eye(4, dtype=dtype), (P, 1, 1))
    status = np.zeros(P, dtype=np.int32)
    last = np.array([0.0, 0.0, 0.0, 1.0])
    with np.errstate(all="ignore"):
        for p in range(P):
            ia, ib = int(idx_a[p]), int(idx_b[p])
            if not (0 <= ia < n and 0 <= ib < n):
                status[p] = 4
                continue
            if not (np.array_equal(poses[ia][3], last) and np.array_equal(poses[ib][3], last)):
                status[p] = 1
                continue
            a, b = poses[ia].astype(dtype), poses[ib].astype(dtype)
            c = np.empty((3, 3), dtype=dtype)
            c[0, 0] = b[1, 1] * b[2, 2] - b[1, 2] * b[2, 1]
            c[0, 1] = b[0, 2] * b[2, 1] - b[0, 1] * b[2, 2]
            c[0, 2] = b[0, 1] * b[1, 2] - b[0, 2] * b[1, 1]
            c[1, 0] = b[1, 2] * b[2, 0] - b[1, 0] * b[2, 2]
            c[1, 1] = b[0, 0] * b[2, 2] - b[0, 2] * b[2, 0]
            c[1, 2] = b[0, 2] * b[1, 0] - b[0, 0] * b[1, 2]
            c[2, 0] = b[1, 0] * b[2, 1] - b[1, 1] * b[2, 0]
            c[2, 1] = b[0, 1] * b[2, 0] - b[0, 0] * b[2, 1]
            c[2, 2] = b[0, 0] * b[1, 1] - b[0, 1] * b[1, 0]
            det = (b[0, 0] * c[0, 0] + b[0, 1] * c[1, 0]) + b[0, 2] * c[2, 0]
            if not (abs(det) > 0 and np.isfinite(det)):
                status[p] = 2
                continue
            inv = c / det
            d = a[:3, 3] - b[:3, 3]
            for r in range(3):
                for k in range(3):
                    out[p, r, k] = (inv[r, 0] * a[0, k] + inv[r, 1] * a[1, k]) + inv[r, 2] * a[2, k]
                t = (inv[r, 0] * d[0] + inv[r, 1] * d[1]) + inv[r, 2] * d[2]
                out[p, r, 3] = -t if negate_translation else t
    return out, status


def gather(bank, bank_off, pick, capacity=None):
    """-> (points (sum,3), offsets (n_pick+1)); all-zero offsets when a pick is outside the bank or the sum beyond capacity"""
    n = len(bank_off) - 1
    zero = np.zeros((0, 3)), np.zeros(len(pick) + 1, dtype=np.int64)
    if any(not 0 <= int(p) < n for p in pick):
        return zero
    parts = [bank[bank_off[p]: bank_off[p + 1]] for p in pick]
    off = np.zeros(len(pick) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in parts])
    if capacity is not None and off[-1] > capacity:
        return zero
    return np.concatenate(parts), off


# ------------------------------------------------------------------ inputs of the fixture (make_golden_tuples.py stores them)
def trajectory(rows: int, seed: int):
    """a drive of ~1 m steps with a slowly turning heading, then a noisy second pass over its first part (a revisit):
    about rows / 1.15 positions + the rest as second pass; (rows, 2) float64 in a local metric frame"""
    rng = np.random.default_rng([seed, rows])
    n1 = max(1, int(round(rows / 1.15)))
    heading = np.cumsum(rng.normal(0.0, 0.05, size=n1)) + rng.uniform(-np.pi, np.pi)
    step = rng.uniform(0.6, 1.4, size=n1)
    xy = np.cumsum(np.stack([step * np.cos(heading), step * np.sin(heading)], axis=1), axis=0)
    second = xy[: rows - n1] + rng.normal(0.0, 0.5, size=(rows - n1, 2))
    return np.ascontiguousarray(np.concatenate([xy, second]), dtype=np.float64)


def lattice():
    """13 x 13 integer lattice: with r = 5 the pairs (3,4), (4,3), (5,0), (0,5) apart sit exactly on the boundary"""
    g = np.arange(13, dtype=np.float64)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2))


def stationary():
    return np.tile(np.array([[123.456, -78.9]], dtype=np.float64), (40, 1))


def filter_case():
    """500 map and 300 query positions: the map is a drive, two thirds of the queries follow it with metres of noise, a third
    runs away from it, so kept and dropped queries are both present at r = 20; UTM-like offsets make the float32 rounding of
    the map positions matter"""
    rng = np.random.default_rng(77)
    base = np.array([345090.0743, 4037591.323])
    m = trajectory(500, 5)[:500]
    q_near = m[rng.choice(500, size=200)] + rng.normal(0.0, 9.0, size=(200, 2))
    q_edge = m[rng.choice(500, size=50)] + rng.uniform(-1.0, 1.0, size=(50, 2)) * 0.2 + np.array([20.0, 0.0])
    q_far = m[rng.choice(500, size=50)] + rng.uniform(40.0, 90.0, size=(50, 2))
    return m + base, np.concatenate([q_near, q_edge, q_far]) + base


def _rot_zyx(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def pose_set(kind: str, n_poses: int = 120, n_pairs: int = 200):
    """'local': |t| <= 200 m around the origin; 'utm': a drive at UTM-sized coordinates (MulRan's global_pose.csv), pairs a few
    scans apart.  -> poses (n,4,4) f64, idx_a, idx_b (P,) int32"""
    rng = np.random.default_rng({"local": 31, "utm": 32}[kind])
    poses = np.tile(np.eye(4), (n_poses, 1, 1))
    for k in range(n_poses):
        poses[k, :3, :3] = _rot_zyx(rng.uniform(-np.pi, np.pi), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1))
    if kind == "local":
        poses[:, :3, 3] = rng.uniform(-1.0, 1.0, size=(n_poses, 3)) * np.array([200.0, 200.0, 5.0])
        ia, ib = rng.integers(0, n_poses, size=n_pairs), rng.integers(0, n_poses, size=n_pairs)
    else:
        xy = trajectory(n_poses, 9)[:n_poses] * 3.0
        poses[:, :2, 3] = xy + np.array([345090.0743, 4037591.323])
        poses[:, 2, 3] = 20.0 + rng.normal(0.0, 0.5, size=n_poses)
        ia = rng.integers(0, n_poses, size=n_pairs)
        ib = np.clip(ia + rng.integers(-3, 4, size=n_pairs), 0, n_poses - 1)
    return poses, ia.astype(np.int32), ib.astype(np.int32)


def mask_positions():
    """80 positions of a drive; tuples 10 and 79 (the last) are moved far away: their positive rows are empty"""
    xy = trajectory(80, 3)[:80].copy()
    xy[10] += 5000.0
    xy[79] -= 5000.0
    return xy


def mask_labels(B: int):
    """labels with repeats, neighbours, the isolated tuple 10 (B > 4), and 79 = the last tuple, whose positive row is empty too"""
    if B == 4:
        return np.array([79, 30, 31, 30], dtype=np.int32)
    rng = np.random.default_rng([41, B])
    labels = rng.integers(0, 80, size=B)
    labels[0], labels[1] = 79, 10
    labels[B - 1] = labels[B // 2]                   # a repeated label, whatever the draw
    labels[2:5] = (30, 31, 30)                       # neighbours and a repeat among them
    return labels.astype(np.int32)


# ------------------------------------------------------------------ the synthetic sequence of the end-to-end test
def planted_sequence(n_scans: int = 6, n_points: int = 6000, seed: int = 11, noise: float = 0.02, n_zero: int = 17):
    """n_scans views of ONE `synth.lidar_scan` scene, as `synth.planted_scan_pair` makes two: scan k = a subsample of the scene
    seen from the planted pose W_k (scan frame -> world), plus N(0, noise) per coordinate, plus n_zero all-zero returns that
    the bank has to drop.  Planted poses: 1 m apart along a gentle curve.  "GPS" poses: the planted ones perturbed by <= 0.3 m
    and <= 0.02 rad of yaw.  -> raws [(n_points + n_zero, 4) float32], planted (n,4,4), gps (n,4,4)"""
    from egonn_amd.synth import lidar_scan
    scene = lidar_scan(seed, n_points=int(1.6 * n_points)).astype(np.float64)
    rng = np.random.default_rng([seed, 0x7051])
    planted, gps, raws = np.tile(np.eye(4), (n_scans, 1, 1)), np.tile(np.eye(4), (n_scans, 1, 1)), []
    for k in range(n_scans):
        yaw = 0.03 * k                                                       # the curve: heading turns 0.03 rad per metre
        planted[k, :3, :3] = _rot_zyx(yaw, 0.002 * k, -0.001 * k)
        planted[k, :3, 3] = [np.sin(yaw) / 0.03 if k else 0.0, (1.0 - np.cos(yaw)) / 0.03 if k else 0.0, 0.01 * k]
        d = rng.uniform(-1.0, 1.0, size=3)
        d = 0.3 * rng.uniform(0.3, 1.0) * d / np.linalg.norm(d)
        gps[k, :3, :3] = _rot_zyx(yaw + rng.uniform(-0.02, 0.02), 0.002 * k, -0.001 * k)
        gps[k, :3, 3] = planted[k, :3, 3] + d
        world = scene[rng.choice(len(scene), size=n_points, replace=False)]
        local = (world - planted[k, :3, 3]) @ planted[k, :3, :3] + noise * rng.standard_normal(world.shape)   # R^T (p - t)
        raw = np.zeros((n_points + n_zero, 4), dtype=np.float32)
        keep = np.ones(len(raw), dtype=bool)
        keep[rng.choice(len(raw), size=n_zero, replace=False)] = False
        raw[keep, :3] = local
        raw[keep, 3] = rng.uniform(0.0, 1.0, size=n_points)
        raws.append(raw)
    return raws, planted, gps


def zero_filtered(raw):
    """load_pc's first step: drop the returns whose coordinates are all (close to) zero"""
    pc = raw[:, :3]
    return np.ascontiguousarray(pc[~np.all(np.isclose(pc, 0.0), axis=1)])
