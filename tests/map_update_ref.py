"""Numpy restatement of the map update (include/egonn_hip.h, "map update"): records that carry the NDT
moments (`integrate_moments`, `merge_moments`), taking observations out again (`subtract` with its legality rule, `remove`)
and what `VoxelMap(track=True)` does with its ledger (`Map`: insert, remove, repose).  Built on tests/voxel_map_ref.py (the
point arithmetic, the four arrays) and tests/ndt_ref.py (the moment shift and order) by import.  `NaiveMap` is the second
restatement: a dict of Python ints that is simply built from the observations that survive.  tests/test_map_update_host.py
holds them against each other; the GPU tests compare the device with the first, bitwise."""
from __future__ import annotations

import numpy as np

from tests import ndt_ref as nref
from tests import voxel_map_ref as vref

RANGE, CAPACITY, BAD_INDEX, MISMATCH = vref.RANGE, vref.CAPACITY, vref.BAD_INDEX, 8
FIELDS = vref.FIELDS
MOMENTS = ("s1", "s2")
ALL = FIELDS + MOMENTS


def empty(moments=True):
    out = vref.empty()
    if moments:
        out.update(s1=np.zeros((0, 3), np.int64), s2=np.zeros((0, 6), np.int64))
    return out


def has_moments(rec):
    return "s1" in rec


def fields(rec):
    return ALL if has_moments(rec) else FIELDS


def same(a, b):
    """two sets of records, bit for bit, moments included when either has them"""
    if has_moments(a) != has_moments(b):
        return False
    return all(np.array_equal(np.asarray(a[f]), np.asarray(b[f])) and np.asarray(a[f]).shape == np.asarray(b[f]).shape and
               np.asarray(a[f]).dtype == np.asarray(b[f]).dtype for f in fields(a))


def copy(rec, status=None):
    out = {f: np.array(rec[f]) for f in fields(rec)}
    out["status"] = rec.get("status", 0) if status is None else status
    return out


def integrate_moments(bank, bank_off, pick, poses, origin, voxel, points_capacity=None, capacity=None):
    """egonn_voxel_map_integrate_moments: the four arrays of vref.integrate, and s1 = sum m, s2 = sum m_a m_b over the points of
    every voxel with m = q >> 10.  Written out once more, from the points: it does not call vref.integrate or nref.accumulate"""
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
        key, q, valid = vref.point_keys(pts, poses[k], origin, voxel)
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
    n = len(uniq)
    m = qs >> nref.SHIFT
    mm = np.stack([m[:, a] * m[:, b] for a, b in nref.PAIRS6], axis=1) if len(m) else np.zeros((0, 6), np.int64)
    sums, s1, s2 = np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int64), np.zeros((n, 6), np.int64)
    np.add.at(sums, inv, qs)
    np.add.at(s1, inv, m)
    np.add.at(s2, inv, mm)
    seen = np.unique(np.stack([inv, ks], axis=1), axis=0) if len(inv) else np.zeros((0, 2), np.int64)
    out.update(keys=uniq, sums=sums, count=np.bincount(inv, minlength=n).astype(np.int32),
               obs=np.bincount(seen[:, 0], minlength=n).astype(np.int32), s1=s1, s2=s2)
    return out


def integrate(bank, bank_off, pick, poses, origin, voxel, moments=True, **kw):
    """with or without moments"""
    return integrate_moments(bank, bank_off, pick, poses, origin, voxel, **kw) if moments \
        else vref.integrate(bank, bank_off, pick, poses, origin, voxel, **kw)


def merge_moments(A, B, capacity_out=None):
    """egonn_voxel_map_merge_moments: vref.merge on the four arrays (its positions and its capacity rule), the moments added on
    matched rows; beyond capacity_out: A with its moments, CAPACITY"""
    out = vref.merge(A, B, capacity_out)
    if not has_moments(A):
        return out
    if capacity_out is not None and len(np.union1d(A["keys"], B["keys"])) > capacity_out:
        out.update(s1=A["s1"].copy(), s2=A["s2"].copy())
        return out
    n = len(out["keys"])
    out.update(s1=np.zeros((n, 3), np.int64), s2=np.zeros((n, 6), np.int64))
    for R in (A, B):
        at = np.searchsorted(out["keys"], R["keys"])
        out["s1"][at] += R["s1"]
        out["s2"][at] += R["s2"]
    return out


def subtract(A, B):
    """egonn_voxel_map_subtract: out = A - B.  r = A[k] - B[k] over sums, count, obs (and s1, s2); a B row is legal iff k is in A
    and (r.count > 0 and r.obs > 0, or every field of r is zero).  All legal: A's rows with r in place of the matched ones,
    without those whose r.count is 0.  Otherwise A unchanged and MISMATCH"""
    assert has_moments(A) == has_moments(B)
    status = A.get("status", 0) | B.get("status", 0)
    na = len(A["keys"])
    at = np.searchsorted(A["keys"], B["keys"])
    present = (at < na) & (A["keys"][np.minimum(at, max(na - 1, 0))] == B["keys"]) if na else np.zeros(len(B["keys"]), bool)
    if not present.all():
        return copy(A, status | MISMATCH)
    value = [f for f in fields(A) if f != "keys"]
    r = {f: A[f].astype(np.int64) for f in value}                        # int64 - int64 wraps, as the device's does
    for f in value:
        r[f][at] -= B[f].astype(np.int64)
    zero = np.ones(len(at), bool)
    for f in value:
        zero &= (r[f][at] == 0).reshape(len(at), r[f][0:1].size).all(axis=1)
    legal = zero | ((r["count"][at] > 0) & (r["obs"][at] > 0))
    if not legal.all():
        return copy(A, status | MISMATCH)
    keep = r["count"] != 0
    out = {"keys": A["keys"][keep], "status": status}
    for f in value:
        out[f] = r[f][keep].astype(A[f].dtype)
    return out


def insert(rec, bank, bank_off, pick, poses, origin, voxel):
    """one chunk of VoxelMap.insert"""
    return merge_moments(rec, integrate(bank, bank_off, pick, poses, origin, voxel, has_moments(rec)))


def remove(rec, bank, bank_off, pick, poses, origin, voxel):
    """one chunk of VoxelMap.remove"""
    return subtract(rec, integrate(bank, bank_off, pick, poses, origin, voxel, has_moments(rec)))


class Map:
    """what VoxelMap does on the host side: the records, and with track=True the ledger and its rules"""

    def __init__(self, voxel, origin, moments=True, track=True):
        self.voxel, self.origin, self.moments, self.track = float(voxel), np.asarray(origin, np.float64), moments, track
        self.rec = empty(moments)
        self.pick, self.pose = [], []

    @property
    def ledger(self):
        n = len(self.pick)
        return np.asarray(self.pick, np.int32).reshape(n), np.asarray(self.pose, np.float64).reshape(n, 4, 4)

    def insert(self, bank, bank_off, pick, poses):
        self.rec = insert(self.rec, bank, bank_off, pick, poses, self.origin, self.voxel)
        if self.track:
            self.pick += [int(p) for p in pick]
            self.pose += [np.array(X, np.float64) for X in poses]
        return self

    def remove(self, bank, bank_off, pick, poses):
        if self.track:
            left = list(range(len(self.pick)))
            for p, X in zip(pick, poses):
                hit = [k for k in left if self.pick[k] == int(p) and self.pose[k].tobytes() == np.array(X, np.float64).tobytes()]
                if not hit:
                    raise ValueError("not in the ledger")                  # before anything changes
                left.remove(hit[0])
            self.pick, self.pose = [self.pick[k] for k in left], [self.pose[k] for k in left]
        self.rec = remove(self.rec, bank, bank_off, pick, poses, self.origin, self.voxel)
        return self

    def repose(self, bank, bank_off, poses_new, rot_tol=0.0, trans_tol=0.0):
        if not self.track:
            raise ValueError("repose needs the ledger")
        pick, old = self.ledger
        new = np.asarray(poses_new, np.float64)
        assert new.shape == old.shape
        d = np.abs(new - old)
        moved = np.array([d[k, :3, :3].max() > rot_tol or d[k, :3, 3].max() > trans_tol for k in range(len(pick))], bool)
        at = np.flatnonzero(moved)
        if len(at):
            self.remove(bank, bank_off, pick[at], old[at])
            self.insert(bank, bank_off, pick[at], new[at])
            old[at] = new[at]
            self.pick, self.pose = [int(p) for p in pick], [old[k].copy() for k in range(len(pick))]
        return int(moved.sum())


class NaiveMap:
    """{key (Python int): [sums (3), count, {observation ids}, s1 (3), s2 (6)]} with Python ints: a map that is only ever built,
    from whatever observations it is given (the survivors).  The key and q of a point are vref.point_keys' (held against
    vref.NaiveMap's Python-float arithmetic in tests/test_voxel_map_host.py)"""

    def __init__(self, voxel, origin):
        self.voxel, self.origin, self.vox, self.n_obs = voxel, origin, {}, 0

    def insert(self, bank, bank_off, pick, poses):
        for p, X in zip(pick, poses):
            oid = self.n_obs
            self.n_obs += 1
            key, q, valid = vref.point_keys(bank[bank_off[p]: bank_off[p + 1]], X, self.origin, self.voxel)
            for kk, qq in zip(key[valid].tolist(), q[valid].tolist()):
                v = self.vox.setdefault(kk, [[0, 0, 0], 0, set(), [0, 0, 0], [0] * 6])
                m = [c >> nref.SHIFT for c in qq]
                for a in range(3):
                    v[0][a] += qq[a]
                    v[3][a] += m[a]
                v[1] += 1
                v[2].add(oid)
                for e, (a, b) in enumerate(nref.PAIRS6):
                    v[4][e] += m[a] * m[b]
        return self

    def records(self, moments=True):
        keys = sorted(self.vox)
        col = lambda i, w: np.array([self.vox[k][i] for k in keys], np.int64).reshape(-1, w)      # noqa: E731
        out = {"keys": np.array(keys, np.uint64), "sums": col(0, 3), "count": np.array([self.vox[k][1] for k in keys], np.int32),
               "obs": np.array([len(self.vox[k][2]) for k in keys], np.int32), "status": 0}
        if moments:
            out.update(s1=col(3, 3), s2=col(4, 6))
        return out


def one_voxel(key, sums, count, obs, s1, s2):
    return {"keys": np.array([key], np.uint64), "sums": np.array([sums], np.int64), "count": np.array([count], np.int32),
            "obs": np.array([obs], np.int32), "s1": np.array([s1], np.int64), "s2": np.array([s2], np.int64), "status": 0}


# ------------------------------------------------------------------ inputs shared by the host and the GPU tests
def illegal_rows(A, row):
    """the five kinds of illegal B row against row `row` of A -> {name: a one-row B}"""
    k, f = A["keys"][row], {x: A[x][row] for x in ALL if x != "keys"}
    assert f["count"] >= 2 and f["obs"] >= 2
    held = set(A["keys"].tolist())
    absent = next(int(k) + d for d in range(1, len(held) + 2) if int(k) + d not in held)      # a z neighbour the map lacks
    half = lambda x: x // 2                                                    # noqa: E731
    return {"absent key": one_voxel(absent, half(f["sums"]), 1, 1, half(f["s1"]), half(f["s2"])),
            "excess count": one_voxel(k, f["sums"], f["count"] + 1, f["obs"], f["s1"], f["s2"]),
            "excess obs": one_voxel(k, half(f["sums"]), f["count"] - 1, f["obs"] + 1, half(f["s1"]), half(f["s2"])),
            "count 0 with a remainder": one_voxel(k, f["sums"] - np.array([1, 0, 0]), f["count"], f["obs"], f["s1"], f["s2"]),
            "count > 0 with obs 0": one_voxel(k, half(f["sums"]), f["count"] - 1, f["obs"], half(f["s1"]), half(f["s2"]))}


def with_row(B, extra):
    """the legal rows B and one more row, in key order (replacing B's row of that key)"""
    keep = B["keys"] != extra["keys"][0]
    keys = np.concatenate([B["keys"][keep], extra["keys"]])
    order = np.argsort(keys, kind="stable")
    out = {f: np.concatenate([B[f][keep], extra[f]])[order] for f in ALL}
    out["status"] = 0
    return out
