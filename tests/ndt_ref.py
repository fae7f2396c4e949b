"""Numpy restatement of csrc/ndt.hip (accumulate, finalize, register) as include/egonn_hip.h states the arithmetic ("NDT
layer"), and a second, naive one (`NaiveLayer`: a dict with Python ints and Python floats, one point at a time).  The moments,
the mean and the covariance are restated bit for bit; the eigen-decomposition exists twice (`eig="jacobi"`: the device's
schedule in Python floats; `eig="eigh"`: np.linalg.eigh, which shares no logic with the device), and the 6 x 6 solve is
np.linalg.solve (the device: LDL^T without pivoting).  tests/test_ndt_host.py holds the restatements against each other; the
GPU tests compare the device with them.  Inputs are the voxel-map tests' (`random_scene`, `planted_bank`)."""
from __future__ import annotations

import math

import numpy as np

from tests import voxel_map_ref as vref

SHIFT = 10                                   # m = q >> 10: 20 bits
RANGE, CAPACITY, BAD_INDEX = vref.RANGE, vref.CAPACITY, vref.BAD_INDEX
FEW_CORR, MAX_ITER, EMPTY, SINGULAR = 1, 2, 4, 16
OFFSETS = np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.int64)
PAIRS6 = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # xx, xy, xz, yy, yz, zz
SINGULAR_COND = 2.0 ** 40                    # the restatement's reading of "rank deficient", as tests/icp_plane_ref.py has it


def zeros(n):
    return {"cnt": np.zeros(n, np.int32), "s1": np.zeros((n, 3), np.int64), "s2": np.zeros((n, 6), np.int64), "missed": 0, "status": 0}


def moments(q):
    """q (n,3) int64 residuals -> m (n,3), mm (n,6)"""
    m = q >> SHIFT
    return m, np.stack([m[:, a] * m[:, b] for a, b in PAIRS6], axis=1)


def accumulate(keys, bank, bank_off, pick, poses, origin, voxel, points_capacity=None, out=None):
    """egonn_ndt_accumulate: adds into `out` (zeros(len(keys)) when None) and returns it"""
    keys = np.asarray(keys, np.uint64)
    bank, bank_off = np.asarray(bank, np.float64).reshape(-1, 3), np.asarray(bank_off, np.int64)
    out = zeros(len(keys)) if out is None else out
    n_clouds, parts, total = len(bank_off) - 1, [], 0
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
    for k, pts in parts:
        key, q, valid = vref.point_keys(pts, poses[k], origin, voxel)
        if not valid.all():
            out["status"] |= RANGE
        key, q = key[valid], q[valid]
        row = np.searchsorted(keys, key)
        hit = (row < len(keys)) & (keys[np.minimum(row, max(len(keys) - 1, 0))] == key) if len(keys) else np.zeros(len(key), bool)
        out["missed"] += int((~hit).sum())
        m, mm = moments(q[hit])
        np.add.at(out["cnt"], row[hit], 1)
        np.add.at(out["s1"], row[hit], m)
        np.add.at(out["s2"], row[hit], mm)
    return out


def same(a, b):
    return all(np.array_equal(a[f], b[f]) and a[f].dtype == b[f].dtype for f in ("cnt", "s1", "s2")) and a["missed"] == b["missed"]


def mean_cov(keys, cnt, s1, s2, voxel):
    """bit for bit as the header: -> mean (n,3) relative to the origin, cov (n,6); NaN / inf where cnt < 2"""
    voxel = np.float64(voxel)
    with np.errstate(all="ignore"):
        nf = np.asarray(cnt).astype(np.float64)
        a1 = np.asarray(s1).astype(np.float64)
        idx = vref.indices(keys).astype(np.float64)
        mean = (idx + (a1 / nf[:, None]) * 2.0 ** -20) * voxel
        u = voxel * 2.0 ** -20
        cov = np.stack([((((np.asarray(s2)[:, e].astype(np.float64) - (a1[:, a] * a1[:, b]) / nf) / (nf - 1.0)) * u) * u)
                        for e, (a, b) in enumerate(PAIRS6)], axis=1) if len(nf) else np.zeros((0, 6))
    return mean, cov


def full(c6):
    """(n,6) upper entries -> (n,3,3)"""
    c6 = np.asarray(c6, np.float64)
    M = np.zeros(c6.shape[:-1] + (3, 3))
    for e, (a, b) in enumerate(PAIRS6):
        M[..., a, b] = M[..., b, a] = c6[..., e]
    return M


def jacobi3(C):
    """the device's cyclic Jacobi (csrc/jacobi3.h) in Python floats -> (eigenvalues [3], V columns) unsorted"""
    A = [[float(C[i][j]) for j in range(3)] for i in range(3)]
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(30):
        if abs(A[0][1]) + abs(A[0][2]) + abs(A[1][2]) == 0.0:
            break
        for i in range(2):
            for j in range(i + 1, 3):
                apq = A[i][j]
                if apq != 0.0:
                    theta = (A[j][j] - A[i][i]) / (2.0 * apq)
                    tt = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                    c = 1.0 / math.sqrt(tt * tt + 1.0)
                    s = tt * c
                    for k in range(3):
                        aki, akj = A[k][i], A[k][j]
                        A[k][i], A[k][j] = c * aki - s * akj, s * aki + c * akj
                    for k in range(3):
                        aik, ajk = A[i][k], A[j][k]
                        A[i][k], A[j][k] = c * aik - s * ajk, s * aik + c * ajk
                    A[i][j] = A[j][i] = 0.0
                    for k in range(3):
                        vki, vkj = V[k][i], V[k][j]
                        V[k][i], V[k][j] = c * vki - s * vkj, s * vki + c * vkj
    return [A[0][0], A[1][1], A[2][2]], V


def finalize(keys, cnt, s1, s2, voxel, min_points=6, min_eig_ratio=0.01, eig="jacobi"):
    """egonn_ndt_finalize -> {'mean', 'cov', 'info', 'eigenvalues', 'normal', 'valid', 'n_valid'}; an invalid row is zeros"""
    n = len(keys)
    mean, cov = mean_cov(keys, cnt, s1, s2, voxel)
    C = full(cov)
    lam, vec = np.zeros((n, 3)), np.zeros((n, 3, 3))                  # vec[r, :, i] = eigenvector i
    fin = np.isfinite(C).all(axis=(1, 2)) if n else np.zeros(0, bool)
    for r in np.nonzero(fin)[0]:
        if eig == "jacobi":
            l, V = jacobi3(C[r])
            order = np.argsort(np.array(l), kind="stable")           # ascending, ties in column order
            lam[r], vec[r] = np.array(l)[order], np.array(V)[:, order]
        else:
            lam[r], vec[r] = np.linalg.eigh(C[r])
    with np.errstate(all="ignore"):
        lp = np.maximum(lam, np.float64(min_eig_ratio) * lam[:, 2:3])
        w = 1.0 / lp
        info = np.zeros((n, 6))
        for i in range(3):
            for e, (a, b) in enumerate(PAIRS6):
                info[:, e] = info[:, e] + (w[:, i] * vec[:, a, i]) * vec[:, b, i]
    normal = vec[:, :, 0].copy()
    lead = np.where(normal[:, 0] != 0, normal[:, 0], np.where(normal[:, 1] != 0, normal[:, 1], normal[:, 2]))
    normal[lead < 0] *= -1.0
    valid = fin & (np.asarray(cnt) >= min_points) & (lam[:, 2] > 0)
    for arr in (mean, cov, info, lam, normal):
        valid &= np.isfinite(arr).all(axis=1)
    for arr in (mean, cov, info, lam, normal):
        arr[~valid] = 0.0
    return {"mean": mean, "cov": cov, "info": info, "eigenvalues": lam, "normal": normal, "valid": valid.astype(np.uint8),
            "n_valid": int(valid.sum())}


# ------------------------------------------------------------------ the naive restatement
class NaiveLayer:
    """{key (Python int): [cnt, s1 (3 Python ints), s2 (6 Python ints)]} over a fixed key set; Python floats are IEEE doubles"""

    def __init__(self, keys, voxel, origin):
        self.keys = [int(k) for k in keys]
        self.vox = {k: [0, [0, 0, 0], [0] * 6] for k in self.keys}
        self.voxel, self.origin, self.missed, self.status = float(voxel), [float(v) for v in origin], 0, 0

    def accumulate(self, bank, bank_off, pick, poses):
        B, ONE = vref.BIAS, vref.ONE
        for k, p in enumerate(pick):
            if not 0 <= int(p) < len(bank_off) - 1:
                self.status |= BAD_INDEX
                continue
            X = [[float(v) for v in row] for row in poses[k]]
            for pt in bank[bank_off[p]: bank_off[p + 1]]:
                p0, p1, p2 = (float(v) for v in pt)
                idx, m, ok = [], [], True
                for a in range(3):
                    t = X[a][3] - self.origin[a]
                    s = (((X[a][0] * p0 + X[a][1] * p1) + X[a][2] * p2) + t) / self.voxel
                    if not math.isfinite(s) or not -B <= math.floor(s) < B:
                        ok = False
                        break
                    i = math.floor(s)
                    idx.append(i)
                    m.append(min(math.floor((s - float(i)) * float(ONE)), ONE - 1) >> SHIFT)
                if not ok:
                    self.status |= RANGE
                    continue
                key = (idx[0] + B) << (2 * vref.BITS) | (idx[1] + B) << vref.BITS | (idx[2] + B)
                v = self.vox.get(key)
                if v is None:
                    self.missed += 1
                    continue
                v[0] += 1
                for a in range(3):
                    v[1][a] += m[a]
                for e, (a, b) in enumerate(PAIRS6):
                    v[2][e] += m[a] * m[b]
        return self

    def arrays(self):
        return {"cnt": np.array([self.vox[k][0] for k in self.keys], np.int32),
                "s1": np.array([self.vox[k][1] for k in self.keys], np.int64).reshape(-1, 3),
                "s2": np.array([self.vox[k][2] for k in self.keys], np.int64).reshape(-1, 6), "missed": self.missed,
                "status": self.status}

    def mean_cov(self):
        """rows with cnt >= 2 only -> (rows, mean, cov)"""
        rows, mean, cov = [], [], []
        u = self.voxel * 2.0 ** -20
        for r, key in enumerate(self.keys):
            c, s1, s2 = self.vox[key]
            if c < 2:
                continue
            nf = float(c)
            idx = [((key >> s) & vref.MASK) - vref.BIAS for s in (2 * vref.BITS, vref.BITS, 0)]
            rows.append(r)
            mean.append([(float(idx[a]) + (float(s1[a]) / nf) * 2.0 ** -20) * self.voxel for a in range(3)])
            cov.append([(((float(s2[e]) - (float(s1[a]) * float(s1[b])) / nf) / (nf - 1.0)) * u) * u for e, (a, b) in enumerate(PAIRS6)])
        return np.array(rows, np.int64), np.array(mean, np.float64).reshape(-1, 3), np.array(cov, np.float64).reshape(-1, 6)


# ------------------------------------------------------------------ registration
def transform(T, p):
    """vs = ((R0 p0 + R1 p1) + R2 p2) + t"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], axis=1)


def evaluate(src, T, keys, G, voxel, neighbors=1):
    """the sums of one evaluation under T -> {'n_term', 'n_pts', 'score', 'A' (6,6), 'b' (6,)}; G = finalize(...)"""
    keys = np.asarray(keys, np.uint64)
    vs = transform(np.asarray(T, np.float64), src)
    n = len(vs)
    out = {"n_term": 0, "n_pts": 0, "score": 0.0, "A": np.zeros((6, 6)), "b": np.zeros(6)}
    if n == 0 or len(keys) == 0:
        return out
    with np.errstate(all="ignore"):
        f = np.floor(vs / np.float64(voxel))
    ok = np.isfinite(f).all(axis=1) & (np.abs(f) <= 2.0 ** 21).all(axis=1)
    i0 = np.where(ok[:, None], f, 0.0).astype(np.int64)
    I, mean, valid = full(G["info"]), G["mean"], G["valid"].astype(bool)
    any_term = np.zeros(n, bool)
    for off in OFFSETS[:neighbors]:
        idx = i0 + off
        inr = ok & ((idx >= -vref.BIAS) & (idx < vref.BIAS)).all(axis=1)
        b = np.where(inr[:, None], idx + vref.BIAS, 0).astype(np.uint64)
        key = (b[:, 0] << np.uint64(2 * vref.BITS)) | (b[:, 1] << np.uint64(vref.BITS)) | b[:, 2]
        row = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
        hit = inr & (keys[row] == key) & valid[row]
        r = vs[hit] - mean[row[hit]]
        Ih = I[row[hit]]
        g = np.einsum("nab,nb->na", Ih, r)
        with np.errstate(all="ignore"):
            m = (r * g).sum(1)
            fin = np.isfinite(m)
            w = np.exp(-0.5 * m[fin])
        rows = np.nonzero(hit)[0][fin]
        v, g, Ih = vs[rows], g[fin], Ih[fin]
        J = np.zeros((len(v), 3, 6))
        J[:, 0, 1], J[:, 0, 2], J[:, 1, 0], J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = v[:, 2], -v[:, 1], -v[:, 2], v[:, 0], v[:, 1], -v[:, 0]
        J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0                    # J = [-[vs]x | I]
        out["A"] += np.einsum("n,nai,nab,nbj->ij", w, J, Ih, J)
        out["b"] += np.einsum("n,nai,na->i", w, J, g)
        out["score"] += float(w.sum())
        out["n_term"] += len(rows)
        any_term[rows] = True
    out["n_pts"] = int(any_term.sum())
    return out


def step(ev):
    """-> (x (6,) or None when the system is rank deficient)"""
    A, b = ev["A"], ev["b"]
    if not np.isfinite(A).all() or not np.linalg.cond(A) < SINGULAR_COND:
        return None
    x = np.linalg.solve(A, -b)
    return x if np.isfinite(x).all() else None


def vec6_to_T(x):
    """(x0..x5) -> [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)]"""
    a, b, c = float(x[0]), float(x[1]), float(x[2])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    U = np.eye(4)
    U[:3, :3], U[:3, 3] = Rz @ Ry @ Rx, x[3:6]
    return U


def register(src, T_init, keys, G, voxel, neighbors=1, max_iteration=30, eps_rot=1e-5, eps_trans=1e-4):
    """the free-running loop of one pair -> {'T', 'fitness', 'score', 'iterations', 'status', 'trace', 'evals'}"""
    T = np.array(T_init, dtype=np.float64)
    src = np.asarray(src, np.float64).reshape(-1, 3)
    out = {"trace": [T], "evals": []}
    if len(src) == 0:
        return dict(out, T=T, fitness=0.0, score=0.0, iterations=0, status=EMPTY)
    conv = False
    for k in range(max_iteration + 1):
        ev = evaluate(src, T, keys, G, voxel, neighbors)
        out["evals"].append(ev)
        x, bit, stop = None, 0, False
        if conv:
            stop = True
        elif k >= max_iteration:
            stop, bit = True, MAX_ITER
        elif ev["n_term"] < 6:
            stop, bit = True, FEW_CORR
        else:
            x = step(ev)
            if x is None:
                stop, bit = True, SINGULAR
        if stop:
            return dict(out, T=T, fitness=ev["n_pts"] / len(src), score=ev["score"] / len(src), iterations=k, status=bit)
        T = vec6_to_T(x) @ T
        out["trace"].append(T)
        out.setdefault("steps", []).append(x)
        conv = bool(np.abs(x[:3]).max() < eps_rot and np.abs(x[3:]).max() < eps_trans)
    raise AssertionError("unreachable")


# ------------------------------------------------------------------ inputs shared by the host and the GPU tests
random_scene, planted_bank = vref.random_scene, vref.planted_bank
_CACHE = {}


def planted_case(voxel=1.0):
    """The six scans of tuples_data.planted_sequence(), cropped and downsampled as the bank does; for every scan k the layer of
    the OTHER five at their planted poses (keys of their voxel map at `voxel`, moments, Gaussians) and the start T0 = its "GPS"
    pose in the origin-relative frame (origin = the first planted pose's translation).  Computed once."""
    if voxel not in _CACHE:
        from tests import tuples_data as D
        from tests.test_icp_host import downsample_f64
        raws, planted, gps = D.planted_sequence()
        clouds = [downsample_f64(D.zero_filtered(r), 0.1, (-80., 80., -80., 80., -0.9, None))[0].astype(np.float64) for r in raws]
        off = np.zeros(7, np.int64)
        off[1:] = np.cumsum([len(c) for c in clouds])
        bank, org = np.concatenate(clouds), planted[0, :3, 3].copy()
        layers = []
        for k in range(6):
            others = [j for j in range(6) if j != k]
            keys = vref.integrate(bank, off, others, planted[others], org, voxel)["keys"]
            acc = accumulate(keys, bank, off, others, planted[others], org, voxel)
            layers.append({"keys": keys, "acc": acc, "G": finalize(keys, acc["cnt"], acc["s1"], acc["s2"], voxel), "others": others})
        rel = lambda X: np.concatenate([X[:, :3, :3], (X[:, :3, 3] - org)[:, :, None]], axis=2)       # noqa: E731
        T0, Tp = np.tile(np.eye(4), (6, 1, 1)), np.tile(np.eye(4), (6, 1, 1))
        T0[:, :3, :], Tp[:, :3, :] = rel(gps), rel(planted)
        _CACHE[voxel] = {"clouds": clouds, "bank": bank, "off": off, "planted": planted, "gps": gps, "origin": org, "layers": layers,
                         "T0": T0, "T_planted": Tp, "voxel": voxel, "free": {}}
    return _CACHE[voxel]


def finalize_case(voxel=0.5, origin=(0.5, -1.25, 0.125)):
    """The voxels of the finalize tests: random_scene() under its poses plus one cloud of special voxels far from it (a plane
    z = const, a tilted plane, a line, one point eight times, five points) -> bank, off, poses, keys, moments; computed once"""
    if "finalize" not in _CACHE:
        bank, off, poses = random_scene()
        g = np.arange(1, 8) / 8.0
        xy = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
        at = lambda i: np.asarray(origin) + voxel * np.array([40.0 + 2 * i, 0.0, 0.0])          # noqa: E731
        special = np.concatenate([at(0) + voxel * np.concatenate([xy, np.full((len(xy), 1), 0.5)], 1),
                                  at(1) + voxel * np.stack([xy[:, 0], xy[:, 0], xy[:, 1]], 1),
                                  at(2) + voxel * np.stack([g, g, g], 1), at(2) + voxel * np.stack([g, g, g], 1)[:3],
                                  at(3) + voxel * np.tile([[0.25, 0.5, 0.75]], (8, 1)),
                                  at(4) + voxel * np.random.default_rng(3).uniform(0.1, 0.9, (5, 3))])
        bank = np.concatenate([bank, special])
        off = np.concatenate([off, [len(bank)]])
        poses = np.concatenate([poses, np.eye(4)[None]])
        pick = np.arange(len(off) - 1)
        keys = vref.integrate(bank, off, pick, poses, origin, voxel)["keys"]
        _CACHE["finalize"] = {"bank": bank, "off": off, "poses": poses, "pick": pick, "keys": keys, "voxel": voxel,
                              "origin": np.asarray(origin, np.float64), "acc": accumulate(keys, bank, off, pick, poses, origin, voxel)}
    return _CACHE["finalize"]


def info_rel_diff(a, b):
    """largest |a - b| over a voxel's six entries relative to the voxel's largest |b| entry, over all voxels with one"""
    den = np.abs(b).max(axis=1)
    ok = den > 0
    return float((np.abs(a - b).max(axis=1)[ok] / den[ok]).max()) if ok.any() else 0.0


def planted_free(k, neighbors, voxel=1.0):
    """the restatement's free run of scan k of planted_case against the layer of the other five; computed once"""
    c = planted_case(voxel)
    if (k, neighbors) not in c["free"]:
        L = c["layers"][k]
        c["free"][(k, neighbors)] = register(c["clouds"][k], c["T0"][k], L["keys"], L["G"], voxel, neighbors)
    return c["free"][(k, neighbors)]
