"""Numpy restatement of csrc/voxel_map.hip (integrate, merge, select and the centroid formula), bit for bit as
include/egonn_hip.h states the arithmetic, with int64 sums; and a second, naive restatement (`NaiveMap`): a dict keyed by
Python ints with Python-int sums and Python-float arithmetic, one point at a time.  tests/test_voxel_map_host.py holds the two
against each other; the GPU tests compare the device with the first, bitwise."""
from __future__ import annotations

import math

import numpy as np

BITS = 21
BIAS = 1 << 20
ONE = 1 << 30
MASK = (1 << BITS) - 1
RANGE, CAPACITY, BAD_INDEX = 1, 2, 4
FIELDS = ("keys", "sums", "count", "obs")


def empty():
    return {"keys": np.zeros(0, np.uint64), "sums": np.zeros((0, 3), np.int64), "count": np.zeros(0, np.int32),
            "obs": np.zeros(0, np.int32), "status": 0}


def point_keys(points, pose, origin, voxel):
    """one observation: -> keys (n,) uint64, q (n,3) int64, valid (n,) bool; every operation rounded to fp64, in the order
    of the header: t' = t - origin first, ((R0 p0 + R1 p1) + R2 p2) + t', / voxel, floor, residual * 2^30, clamp"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    X = np.asarray(pose, np.float64)
    org = np.asarray(origin, np.float64)
    voxel = np.float64(voxel)
    n = len(p)
    idx, q, valid = np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int64), np.ones(n, bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            t = X[a, 3] - org[a]
            w = ((X[a, 0] * p[:, 0] + X[a, 1] * p[:, 1]) + X[a, 2] * p[:, 2]) + t
            s = w / voxel
            f = np.floor(s)
            ok = (f >= -float(BIAS)) & (f < float(BIAS))                 # False for NaN / inf
            valid &= ok
            idx[:, a] = np.where(ok, f, 0.0).astype(np.int64)
            r = np.floor((s - f) * float(ONE))
            q[:, a] = np.minimum(np.where(ok, r, 0.0).astype(np.int64), ONE - 1)
    keys = (((idx[:, 0] + BIAS).astype(np.uint64) << np.uint64(2 * BITS)) | ((idx[:, 1] + BIAS).astype(np.uint64) << np.uint64(BITS))
            | (idx[:, 2] + BIAS).astype(np.uint64))
    return keys, q, valid


def integrate(bank, bank_off, pick, poses, origin, voxel, points_capacity=None, capacity=None):
    """egonn_voxel_map_integrate -> records {'keys', 'sums', 'count', 'obs', 'status'}"""
    bank, bank_off = np.asarray(bank, np.float64).reshape(-1, 3), np.asarray(bank_off, np.int64)
    n_clouds, out = len(bank_off) - 1, empty()
    parts, total = [], 0
    for k, p in enumerate(pick):
        if not 0 <= int(p) < n_clouds:
            out["status"] |= BAD_INDEX
            continue
        pts = bank[bank_off[p]: bank_off[p + 1]]
        total += len(pts)
        parts.append((k, pts))
    if points_capacity is not None and total > points_capacity:
        out["status"] |= CAPACITY
        return out
    keys, qs, ks = [np.zeros(0, np.uint64)], [np.zeros((0, 3), np.int64)], [np.zeros(0, np.int64)]
    for k, pts in parts:
        key, q, valid = point_keys(pts, poses[k], origin, voxel)
        if not valid.all():
            out["status"] |= RANGE
        keys.append(key[valid])
        qs.append(q[valid])
        ks.append(np.full(int(valid.sum()), k, np.int64))
    keys, qs, ks = np.concatenate(keys), np.concatenate(qs), np.concatenate(ks)
    uniq, inv = np.unique(keys, return_inverse=True)
    if capacity is not None and len(uniq) > capacity:
        out["status"] |= CAPACITY
        return out
    sums = np.zeros((len(uniq), 3), np.int64)
    np.add.at(sums, inv, qs)
    seen = np.unique(np.stack([inv, ks], axis=1), axis=0) if len(inv) else np.zeros((0, 2), np.int64)
    out.update(keys=uniq, sums=sums, count=np.bincount(inv, minlength=len(uniq)).astype(np.int32),
               obs=np.bincount(seen[:, 0], minlength=len(uniq)).astype(np.int32))
    return out


def merge(A, B, capacity_out=None):
    """egonn_voxel_map_merge: the union by key, sums / count / obs added; beyond capacity_out: A unchanged, CAPACITY"""
    keys = np.union1d(A["keys"], B["keys"])
    status = A.get("status", 0) | B.get("status", 0)
    if capacity_out is not None and len(keys) > capacity_out:
        return {**{f: A[f].copy() for f in FIELDS}, "status": status | CAPACITY}
    out = {"keys": keys, "sums": np.zeros((len(keys), 3), np.int64), "count": np.zeros(len(keys), np.int32),
           "obs": np.zeros(len(keys), np.int32), "status": status}
    for R in (A, B):
        at = np.searchsorted(keys, R["keys"])
        out["sums"][at] += R["sums"]
        out["count"][at] += R["count"]
        out["obs"][at] += R["obs"]
    return out


def insert(rec, bank, bank_off, pick, poses, origin, voxel):
    """what VoxelMap.insert does with one chunk"""
    return merge(rec, integrate(bank, bank_off, pick, poses, origin, voxel))


def indices(keys):
    k = np.asarray(keys, np.uint64)
    return np.stack([((k >> np.uint64(s)) & np.uint64(MASK)).astype(np.int64) - BIAS for s in (2 * BITS, BITS, 0)], axis=1)


def centroids(rec, origin, voxel):
    """c_a = ((double) i_a + (double) sum_q_a / ((double) count * 2^30)) * voxel + origin_a"""
    i = indices(rec["keys"]).astype(np.float64)
    den = rec["count"].astype(np.float64) * float(ONE)
    return (i + rec["sums"].astype(np.float64) / den[:, None]) * np.float64(voxel) + np.asarray(origin, np.float64)[None, :]


def select(rec, origin, voxel, min_count=1, min_obs=1, boxes=None, relative=False, capacity=None):
    """egonn_voxel_map_select -> {'points', 'offsets', 'count', 'obs', 'status'}"""
    c = centroids(rec, origin, voxel) if len(rec["keys"]) else np.zeros((0, 3))
    keep = (rec["count"] >= min_count) & (rec["obs"] >= min_obs)
    segs = [None] if boxes is None else [np.asarray(b, np.float64) for b in boxes]
    pts, cnt, obs, off = [np.zeros((0, 3))], [np.zeros(0, np.int32)], [np.zeros(0, np.int32)], [0]
    for b in segs:
        m = keep.copy()
        if b is not None:
            with np.errstate(invalid="ignore"):
                m &= ((b[:3] - b[3:] <= c) & (c < b[:3] + b[3:])).all(axis=1)
        pts.append(c[m] - b[:3] if (relative and b is not None) else c[m])
        cnt.append(rec["count"][m])
        obs.append(rec["obs"][m])
        off.append(off[-1] + int(m.sum()))
    if capacity is not None and off[-1] > capacity:
        return {"points": np.zeros((0, 3)), "offsets": np.zeros(len(segs) + 1, np.int64), "count": cnt[0], "obs": obs[0],
                "status": CAPACITY}
    return {"points": np.concatenate(pts), "offsets": np.array(off, np.int64), "count": np.concatenate(cnt),
            "obs": np.concatenate(obs), "status": 0}


# ------------------------------------------------------------------ the naive restatement
class NaiveMap:
    """a dict {key (Python int): [sum_x, sum_y, sum_z, count, {observation ids}]}; Python floats are IEEE doubles, Python
    ints do not overflow"""

    def __init__(self, voxel, origin):
        self.voxel, self.origin = float(voxel), [float(v) for v in origin]
        self.vox, self.status, self.n_obs = {}, 0, 0

    def insert(self, bank, bank_off, pick, poses):
        for k, p in enumerate(pick):
            oid = self.n_obs
            self.n_obs += 1
            if not 0 <= int(p) < len(bank_off) - 1:
                self.status |= BAD_INDEX
                continue
            X = [[float(v) for v in row] for row in poses[k]]
            for pt in bank[bank_off[p]: bank_off[p + 1]]:
                p0, p1, p2 = (float(v) for v in pt)
                idx, q, ok = [], [], True
                for a in range(3):
                    t = X[a][3] - self.origin[a]
                    s = (((X[a][0] * p0 + X[a][1] * p1) + X[a][2] * p2) + t) / self.voxel
                    if not math.isfinite(s) or not -BIAS <= math.floor(s) < BIAS:
                        ok = False
                        break
                    i = math.floor(s)
                    idx.append(i)
                    q.append(min(math.floor((s - float(i)) * float(ONE)), ONE - 1))
                if not ok:
                    self.status |= RANGE
                    continue
                key = (idx[0] + BIAS) << (2 * BITS) | (idx[1] + BIAS) << BITS | (idx[2] + BIAS)
                v = self.vox.setdefault(key, [0, 0, 0, 0, set()])
                v[0] += q[0]
                v[1] += q[1]
                v[2] += q[2]
                v[3] += 1
                v[4].add(oid)
        return self

    def records(self):
        keys = sorted(self.vox)
        return {"keys": np.array(keys, np.uint64), "sums": np.array([self.vox[k][:3] for k in keys], np.int64).reshape(-1, 3),
                "count": np.array([self.vox[k][3] for k in keys], np.int32),
                "obs": np.array([len(self.vox[k][4]) for k in keys], np.int32), "status": self.status}

    def centroids(self):
        out = []
        for key in sorted(self.vox):
            v = self.vox[key]
            idx = [((key >> s) & MASK) - BIAS for s in (2 * BITS, BITS, 0)]
            out.append([(float(idx[a]) + float(v[a]) / (float(v[3]) * float(ONE))) * self.voxel + self.origin[a] for a in range(3)])
        return np.array(out, np.float64).reshape(-1, 3)


def same(a, b):
    """two sets of records, bit for bit"""
    return all(np.array_equal(np.asarray(a[f]), np.asarray(b[f])) and np.asarray(a[f]).shape == np.asarray(b[f]).shape for f in FIELDS)


# ------------------------------------------------------------------ inputs shared by the host and the GPU tests
def random_scene(seed=5, n_clouds=7, n_points=180, span=6.0, offset=(0.0, 0.0, 0.0)):
    """n_clouds clouds of about n_points points around 60 common anchors inside +-span (sizes differ, one cloud is empty) and as
    many poses that turn by up to 0.02 rad and sit `offset` (+- 0.05) away: the clouds share many voxels at 0.2 m to 0.5 m
    -> bank (n,3) f64, bank_off (n_clouds+1) int64, poses (n_clouds,4,4)"""
    rng = np.random.default_rng(seed)
    sizes = [0 if c == 3 else int(n_points + 17 * c - 40) for c in range(n_clouds)]
    base = rng.uniform(-span, span, size=(60, 3))
    clouds = [base[rng.integers(0, len(base), size=s)] + rng.normal(0.0, 0.15, size=(s, 3)) for s in sizes]
    off = np.zeros(n_clouds + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    poses = np.tile(np.eye(4), (n_clouds, 1, 1))
    for c in range(n_clouds):
        a = rng.uniform(-0.02, 0.02)
        poses[c, :3, :3] = [[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]
        poses[c, :3, 3] = np.asarray(offset) + rng.uniform(-0.05, 0.05, size=3)
    return np.ascontiguousarray(np.concatenate(clouds)), off, poses


def planted_bank():
    """the six scans of tuples_data.planted_sequence(), zero-filtered, no crop, as one bank -> bank, bank_off, planted, gps"""
    from tests import tuples_data as D
    raws, planted, gps = D.planted_sequence()
    clouds = [D.zero_filtered(r).astype(np.float64) for r in raws]
    off = np.zeros(len(clouds) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    return np.concatenate(clouds), off, planted, gps
