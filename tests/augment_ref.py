"""Host restatement of the training augmentation (egonn_amd/csrc/augment.hip): the draws, every transform in float64
(the answer) and in the kernel's fp32 arithmetic, the counted error bound, and the checker the GPU tests use.

The draw, restated word for word from the top of augment.hip.  With 64-bit wrapping arithmetic
      ctr = (draw << 50) | (id << 28) | (point << 4) | slot      draw < 2^14, id < 2^22, point < 2^24, slot < 2^4
      z   = seed + 0x9E3779B97F4A7C15 * (ctr + 1)                (the state of splitmix64(seed) after ctr + 1 steps)
      z   = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
      z   = (z ^ (z >> 27)) * 0x94D049BB133111EB
      z   =  z ^ (z >> 31)
  uniform  u   = (z >> 11) * 2^-53                               fp64, in [0, 1)
  uniform  u24 = fp32(z >> 40) * 2^-24                           fp32, in [0, 1), exact
  normal   g   = sqrt(-2 * log(((z >> 32) + 1) * 2^-32)) * cos(6.283185307179586 * ((z & 0xFFFFFFFF) * 2^-32))
                 in fp64, every operation as written, rounded ONCE to fp32 where the reference's generator is fp32
  per point  (point = index inside the scan, < 2^24 - 2; id = the caller's scan id):
      slot 0, 1, 2: jitter normal of x, y, z;  slot 3: removal key = (z & ~0xFFFFFF) | point  (unique per scan)
  per scan   (point = 0xFFFFFF; id = the caller's scan id):
      slot 0: r;  1, 2, 3: translation normals;  4: rotation u;  5: block u;  6: area u;  7: aspect u;  8: x u;  9: y u;
      slot 10: rigid angle u;  11, 12: rigid tx, ty u24
  per batch  (point = 0xFFFFFE; id = set_id):  slot 0: set rotation u;  1: flip u

The error bound E of a position (max over the three coordinates, fp32 kernel against real arithmetic) is COUNTED, with
u = 2^-24 the unit roundoff of fp32:
  jitter       the normal is rounded to fp32 (u), may sit one fp32 step off where the device's log / cos and the host's differ
               in their last fp64 bits (2u), the product by sigma is rounded (u), the sum is rounded:  E += 4u|j| + u|p + j|
  removal      the point becomes exactly 0:  E = 0
  translation  t is rounded (u), may sit one step off (2u), the sum is rounded:  E += 3u|t| + u|p + t|
  rotation     c, s rounded (u each) and possibly one step off (2u), two products and a sum (<= 3u sum|terms|, the bound of
               a 3-term dot product in any order); the old error is turned with |c| + |s| <= sqrt 2:
               E = 1.4143 E + 6u (|x| + |y|)
  flip         exact
  rigid        as the rotation with the z and translation terms:  E = 1.4143 E + 6u (|x| + |y| + |z| + |t|)
Block edges carry the error of the box (the largest E of the scan, on both ends of a span) through get_params; block_band
counts it.  A row's block membership may differ from the float64 answer only within E + band of one of the four faces.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

JITTER, REMOVE_POINTS, TRANSLATE, ROTATE, BLOCK, SET_ROTATE, FLIP, RIGID, JITTER_CLIP = 1, 2, 4, 8, 16, 32, 64, 128, 256
MODE1 = JITTER | JITTER_CLIP | REMOVE_POINTS | TRANSLATE | BLOCK
MODE2 = MODE1 | ROTATE
SET1, SET2 = SET_ROTATE | FLIP, FLIP
PT_SCAN, PT_SET = 0xFFFFFF, 0xFFFFFE
U = 2.0 ** -24
REC_I, REC_D = 8, 32


@dataclass
class Params:
    seed: int = 0
    draw: int = 0
    set_id: int = 0
    stages: int = MODE1 | SET1
    sigma: float = 0.1
    clip: float = 0.2
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


# ------------------------------------------------------------------ draws
def hash64(seed: int, draw: int, sid: int, point, slot: int) -> np.ndarray:
    assert 0 <= draw < 1 << 14 and 0 <= sid < 1 << 22 and 0 <= slot < 16
    point = np.atleast_1d(np.asarray(point)).astype(np.uint64)
    assert point.size == 0 or int(point.max()) < 1 << 24
    with np.errstate(over="ignore"):
        ctr = (np.uint64(draw) << np.uint64(50)) | (np.uint64(sid) << np.uint64(28)) | (point << np.uint64(4)) | np.uint64(slot)
        z = np.uint64(seed & (2 ** 64 - 1)) + np.uint64(0x9E3779B97F4A7C15) * (ctr + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform(z) -> np.ndarray:
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def uniform24(z) -> np.ndarray:
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def normal(z) -> np.ndarray:
    u1 = ((z >> np.uint64(32)).astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = (z & np.uint64(0xFFFFFFFF)).astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def removal_keys(P: Params, sid: int, n: int) -> np.ndarray:
    i = np.arange(n, dtype=np.uint64)
    return (hash64(P.seed, P.draw, sid, i, 3) & ~np.uint64(0xFFFFFF)) | i


def theta_of(max_theta: float, u: float) -> float:
    return ((np.pi * max_theta) / 180.0) * 2.0 * (u - 0.5)


def scan_draws(P: Params, sid: int, n: int) -> dict:
    """everything drawn for one scan of n points, as float64 / ints (no arithmetic of the transforms yet)"""
    def su(slot):
        return float(uniform(hash64(P.seed, P.draw, sid, PT_SCAN, slot))[0])
    d = {"n": n, "sid": sid}
    d["r_u"] = su(0)
    d["r"] = P.r_min + (P.r_max - P.r_min) * d["r_u"] if P.stages & REMOVE_POINTS else 0.0
    d["k"] = int(n * d["r"])
    keys = removal_keys(P, sid, n)
    removed = np.zeros(n, bool)
    d["thresh"] = 0
    if d["k"] > 0:
        kth = np.partition(keys, d["k"] - 1)[d["k"] - 1]
        removed = keys <= kth
        d["thresh"] = int(kth)
    d["removed"] = removed
    i = np.arange(n, dtype=np.uint64)
    d["jitter_normal"] = np.stack([normal(hash64(P.seed, P.draw, sid, i, a)) for a in range(3)], axis=1) if n else np.zeros((0, 3))
    d["trans_normal"] = np.array([float(normal(hash64(P.seed, P.draw, sid, PT_SCAN, 1 + a))[0]) for a in range(3)])
    d["trans"] = P.max_delta * d["trans_normal"]
    d["rot_u"] = su(4)
    d["theta"] = theta_of(P.max_theta, d["rot_u"])
    d["block_u"] = su(5)
    d["area_u"], d["aspect_u"], d["x_u"], d["y_u"] = su(6), su(7), su(8), su(9)
    d["rigid_u"] = su(10)
    d["rigid_angle"] = -P.rot_max + (P.rot_max - (-P.rot_max)) * d["rigid_u"]
    d["rigid_u24"] = np.array([uniform24(hash64(P.seed, P.draw, sid, PT_SCAN, s))[0] for s in (11, 12)], np.float32)
    return d


def set_draws(P: Params) -> dict:
    d = {"rot_u": float(uniform(hash64(P.seed, P.draw, P.set_id, PT_SET, 0))[0]),
         "flip_u": float(uniform(hash64(P.seed, P.draw, P.set_id, PT_SET, 1))[0])}
    d["theta"] = theta_of(P.set_max_theta, d["rot_u"])
    cum = np.cumsum(np.asarray(P.flip_p, np.float64))
    d["flip"] = -1
    if P.stages & FLIP:
        d["flip"] = 0 if d["flip_u"] <= cum[0] else (1 if d["flip_u"] <= cum[1] else (2 if d["flip_u"] <= cum[2] else -1))
    return d


# ------------------------------------------------------------------ the transforms
def _rot(p, c, s, E):
    E = 1.4143 * E + 6 * U * (np.abs(p[:, 0]) + np.abs(p[:, 1])).astype(np.float64)
    x = p[:, 0] * c + p[:, 1] * s
    y = p[:, 0] * (-s) + p[:, 1] * c
    return np.stack([x, y, p[:, 2]], axis=1), E


def block_params(P: Params, d: dict, mn, mx, f):
    """RemoveRandomBlock.get_params on the box (mn, mx).  f = np.float32: the reference's mixed arithmetic (the box is an
    fp32 tensor, Python scalars are rounded to fp32 where they meet it, math.sqrt is fp64); f = np.float64: real arithmetic"""
    span0, span1 = f(mx[0] - mn[0]), f(mx[1] - mn[1])
    area = f(span0 * span1)
    ua = P.scale[0] + (P.scale[1] - P.scale[0]) * d["area_u"]
    ar = P.ratio[0] + (P.ratio[1] - P.ratio[0]) * d["aspect_u"]
    ea = f(f(ua) * area)
    h = float(np.sqrt(np.float64(f(ea * f(ar)))))
    w = float(np.sqrt(np.float64(f(ea / f(ar)))))
    ux = 0.0 + (1.0 - 0.0) * d["x_u"]
    uy = 0.0 + (1.0 - 0.0) * d["y_u"]
    x0 = f(f(mn[0]) + f(f(ux) * f(span0 - f(w))))
    y0 = f(f(mn[1]) + f(f(uy) * f(span1 - f(h))))
    return dict(x0=x0, y0=y0, w=w, h=h, x1=f(x0 + f(w)), y1=f(y0 + f(h)), ea=float(ea), ar=ar, span=(float(span0), float(span1)))


def block_band(bp: dict, mn, Emax: float):
    """counted error of the block's faces (x faces, y faces): the box ends carry Emax each, a span 2 Emax + u |span|; the area's
    relative error is the two spans' plus 4 roundings (product, scale product, ratio product / quotient, and sqrt's input),
    w and h inherit it (the square root halves it; not used); x0 = min + u (span - w) adds its own four roundings."""
    s0, s1 = bp["span"]
    rel = 8 * U + (2 * Emax / s0 if s0 > 0 else 0.0) + (2 * Emax / s1 if s1 > 0 else 0.0)
    out = []
    for a, (size, span) in enumerate(((bp["w"], s0), (bp["h"], s1))):
        e_size = size * rel + 2 * U * size
        e0 = 3 * Emax + e_size + 8 * U * (abs(float(mn[a])) + abs(span) + size)
        out.append(e0 + e_size + 2 * U * (abs(float(bp["x0" if a == 0 else "y0"])) + size))
    return out


def augment(points, offsets, ids, P: Params, dtype=np.float64, T_in=None):
    """-> dict(out (N,3) dtype, removed, erased (N,) bool, E (N,) float64 bound, scans: list of per-scan dicts, set: dict,
    T_out (B,4,4) float32 or None).  dtype float32 mirrors the kernel operation by operation; float64 is the answer."""
    f = np.float32 if dtype == np.float32 else np.float64
    points = np.asarray(points, np.float32)
    N = points.shape[0]
    out = np.array(points, dtype=f)
    removed, erased, E = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, np.float64)
    Q = set_draws(P)
    scans = []
    B = len(offsets) - 1
    T_out = None if not (P.stages & RIGID) else np.zeros((B, 4, 4), np.float32)
    for b in range(B):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        n = hi - lo
        d = scan_draws(P, int(ids[b]), n)
        p = out[lo:hi]
        e = np.zeros(n, np.float64)
        if P.stages & JITTER:
            j = f(P.sigma) * d["jitter_normal"].astype(f)
            if P.stages & JITTER_CLIP:
                j = np.minimum(np.maximum(j, f(-f(P.clip))), f(P.clip))
            p = p + j
            e = e + 4 * U * np.abs(j).max(axis=1, initial=0.0) + U * np.abs(p).max(axis=1, initial=0.0)
        p = np.where(d["removed"][:, None], f(0), p)
        e = np.where(d["removed"], 0.0, e)
        if P.stages & TRANSLATE:
            t = d["trans"].astype(f)
            p = p + t[None, :]
            e = e + 3 * U * np.abs(t).max() + U * np.abs(p).max(axis=1, initial=0.0)
        if P.stages & ROTATE:
            p, e = _rot(p, f(np.cos(d["theta"])), f(np.sin(d["theta"])), e)
        d["block_on"] = bool(P.stages & BLOCK) and d["block_u"] < P.block_p and n > 0
        d["block"] = None
        er = np.zeros(n, bool)
        if P.stages & BLOCK and n > 0:
            d["box"] = (p.min(axis=0), p.max(axis=0))
        if d["block_on"]:
            mn, mx = d["box"]
            bp = block_params(P, d, mn, mx, f)
            d["block"] = bp
            d["band"] = block_band(bp, mn, float(e.max(initial=0.0)))
            er = (bp["x0"] < p[:, 0]) & (p[:, 0] < bp["x1"]) & (bp["y0"] < p[:, 1]) & (p[:, 1] < bp["y1"])
            p = np.where(er[:, None], f(0), p)
        e = np.where(er, 0.0, e)
        if P.stages & SET_ROTATE:
            p, e = _rot(p, f(np.cos(Q["theta"])), f(np.sin(Q["theta"])), e)
        if Q["flip"] >= 0:
            p = p.copy()
            p[:, Q["flip"]] = -p[:, Q["flip"]]
        if P.stages & RIGID:
            cv, sv = np.float32(np.cos(d["rigid_angle"])), np.float32(np.sin(d["rigid_angle"]))
            tm = np.float32(P.trans_max)
            txy = d["rigid_u24"] * np.float32(2.0) * tm - tm
            m = np.eye(4, dtype=np.float32)
            m[0, 0], m[0, 1], m[1, 0], m[1, 1], m[0, 3], m[1, 3] = cv, sv, -sv, cv, txy[0], txy[1]
            d["m"] = m
            mf = m.astype(f) if f is np.float32 else np.eye(4)
            if f is np.float64:
                mf = np.eye(4)
                mf[0, 0] = mf[1, 1] = np.cos(d["rigid_angle"])
                mf[0, 1] = np.sin(d["rigid_angle"])
                mf[1, 0] = -mf[0, 1]
                mf[0, 3], mf[1, 3] = (d["rigid_u24"].astype(np.float64) * 2.0 * P.trans_max - P.trans_max)
            e = 1.4143 * e + 6 * U * (np.abs(p).sum(axis=1) + np.abs(mf[:3, 3]).max()).astype(np.float64)
            p = np.stack([p[:, 0] * mf[r, 0] + p[:, 1] * mf[r, 1] + p[:, 2] * mf[r, 2] + mf[r, 3] for r in range(3)], axis=1)
            Tin = np.eye(4, dtype=np.float32) if T_in is None else np.asarray(T_in[b], np.float32)
            To = np.zeros((4, 4), np.float32)
            for r in range(4):
                for q in range(4):
                    acc = np.float32(0)
                    for k in range(4):
                        acc = np.float32(acc + np.float32(m[r, k] * Tin[k, q]))
                    To[r, q] = acc
            T_out[b] = To
        out[lo:hi] = p
        removed[lo:hi], erased[lo:hi], E[lo:hi] = d["removed"], er, e
        scans.append(d)
    return dict(out=out, removed=removed, erased=erased, E=E + 1e-30, scans=scans, set=Q, T_out=T_out)


def stage1_xy(points, offsets, ids, P: Params, b: int, dtype=np.float64):
    """positions (n,2) of scan b as the block test sees them (after stage 1's rotation) and their bound"""
    Pb = Params(**{**P.__dict__, "stages": P.stages & (JITTER | JITTER_CLIP | REMOVE_POINTS | TRANSLATE | ROTATE)})
    lo, hi = int(offsets[b]), int(offsets[b + 1])
    r = augment(np.asarray(points)[lo:hi], [0, hi - lo], [ids[b]], Pb, dtype)
    return r["out"][:, :2].astype(np.float64), r["E"]


# ------------------------------------------------------------------ the checker
class Mismatch(AssertionError):
    pass


def check(points, offsets, ids, P: Params, got_out, got_removed, got_erased, ref=None, cap=0.001):
    """got_* against the float64 answer.  Removed set: exact.  Erased flags: equal outside E + band of the block's four faces;
    rows inside may differ (excused), at most `cap` of a scan's rows.  Jitter: |out - in| <= clip is implied by the position
    bound.  Positions of rows that are not excused: within E.  Returns the excused share per scan."""
    ref = augment(points, offsets, ids, P, np.float64) if ref is None else ref
    got_out = np.asarray(got_out, np.float64)
    got_removed, got_erased = np.asarray(got_removed, bool), np.asarray(got_erased, bool)
    if not np.array_equal(got_removed, ref["removed"]):
        raise Mismatch(f"removed set differs in {int((got_removed != ref['removed']).sum())} rows")
    shares = []
    for b, d in enumerate(ref["scans"]):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        diff = got_erased[lo:hi] != ref["erased"][lo:hi]
        excused = np.zeros(hi - lo, bool)
        if diff.any():
            if not d["block_on"]:
                raise Mismatch(f"scan {b}: erased rows without a block")
            xy, e = stage1_xy(points, offsets, ids, P, b)
            bp, band = d["block"], d["band"]
            near = np.zeros(hi - lo, bool)
            for a, (f0, f1) in enumerate(((bp["x0"], bp["x1"]), (bp["y0"], bp["y1"]))):
                w = e + band[a]
                near |= (np.abs(xy[:, a] - float(f0)) <= w) | (np.abs(xy[:, a] - float(f1)) <= w)
            if (diff & ~near).any():
                raise Mismatch(f"scan {b}: {int((diff & ~near).sum())} rows on the wrong side of a block face, outside the band")
            excused = diff
            if excused.sum() > cap * (hi - lo):
                raise Mismatch(f"scan {b}: {int(excused.sum())} excused rows of {hi - lo} exceed the cap {cap}")
        shares.append(float(excused.sum()) / max(hi - lo, 1))
        ok = ~excused
        err = np.abs(got_out[lo:hi] - ref["out"][lo:hi]).max(axis=1, initial=0.0)
        bad = ok & ~(err <= ref["E"][lo:hi])
        if bad.any():
            i = int(np.argmax(np.where(bad, err / ref["E"][lo:hi], 0)))
            raise Mismatch(f"scan {b}: {int(bad.sum())} positions outside the bound; row {i}: err {err[i]:.3e} > E {ref['E'][lo + i]:.3e}")
    return shares


def records(res: dict, P: Params):
    """(rec_i (B,8) int64, rec_d (B,32) float64) of an augment(..., float32) result, laid out like the C ABI's"""
    B = len(res["scans"])
    ri, rd = np.zeros((B, REC_I), np.int64), np.zeros((B, REC_D), np.float64)
    Q = res["set"]
    for b, d in enumerate(res["scans"]):
        ri[b, :6] = [d["n"], d["k"], int(d["block_on"]), Q["flip"], 0, d["sid"]]
        ri[b, 6], ri[b, 7] = d["thresh"] & 0xFFFFFFFF, d["thresh"] >> 32
        rd[b, 0] = d["r"]
        if P.stages & TRANSLATE:
            rd[b, 1:4] = d["trans"]
        if P.stages & ROTATE:
            rd[b, 4:7] = [d["theta"], np.cos(d["theta"]), np.sin(d["theta"])]
        if P.stages & BLOCK:
            rd[b, 7] = d["block_u"]
            if d["n"] > 0:
                rd[b, 8:11], rd[b, 11:14] = d["box"][0], d["box"][1]
            else:
                rd[b, 8:11], rd[b, 11:14] = np.inf, -np.inf
            if d["block_on"]:
                bp = d["block"]
                rd[b, 14:20] = [bp["x0"], bp["y0"], bp["w"], bp["h"], bp["x1"], bp["y1"]]
                rd[b, 29], rd[b, 30] = bp["ea"], bp["ar"]
        if P.stages & SET_ROTATE:
            rd[b, 20:23] = [Q["theta"], np.cos(Q["theta"]), np.sin(Q["theta"])]
        if P.stages & FLIP:
            rd[b, 23] = Q["flip_u"]
        if P.stages & RIGID:
            rd[b, 24:27] = [d["rigid_angle"], np.cos(d["rigid_angle"]), np.sin(d["rigid_angle"])]
            rd[b, 27:29] = d["m"][:2, 3]
    return ri, rd


def cloud(seed: int, n: int, spread: float = 40.0) -> np.ndarray:
    """a lidar-like fp32 cloud: wide in x and y, shallow in z"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3)) * np.array([spread, spread, 2.0])
    return p.astype(np.float32)


def batch(seed: int, sizes: Sequence[int]):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return cloud(seed, int(off[-1])), off
