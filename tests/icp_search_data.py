"""Edge geometries of the ICP target-grid search (icp_setup_kernel, icp_key_kernel, icp_cell_range, icp_stream_cells,
icp_search_kernel of egonn_amd/csrc/icp.hip) and an exact oracle for them, shared by tests/test_icp_search_host.py and
tests/test_gpu_icp_search.py.  No GPU here.

Oracle.  p = transform_f64(T, src) (tests/test_icp_host.py: the device's operation order), d2 = (dx*dx + dy*dy) + dz*dz for
every (source, target) pair by brute force, the winner is the minimum by (d2, index), a d2 that is not finite never wins, a row
is a correspondence iff d2 < max_dist * max_dist.  The device performs the same IEEE operations on the same numbers, so its
j(i) and n_corr are the oracle's whatever the coordinates are.  The coordinates, max_dist and every T_init are dyadic (multiples
of 2^-12 below 2^10, rotations by exact quarter and half turns; `cell_cap` goes down to 2^-30 beside its targets, `far_init`
up to 2^10): the winning d2 are exact and their sum is exact in any order, which tests/test_icp_search_host.py proves in
rational arithmetic, so sum_d2 is compared bit for bit as well.  No row is excused and there is no tolerance.

Grid restatement (`grid`, `cell_range`, `stream_shape`): org, ext, h, dim of icp_setup_kernel, the padded cell range of a box
as icp_cell_range has it, and what icp_stream_cells makes of that range: (x, y) columns, batches of 256 columns, target points
and tiles of 256 points per batch, empty columns.  Every geometry whose edge depends on the workgroup's box keeps ns <= 256:
the box is then the box of the whole transformed source and no Morton sort is needed to restate it."""
import math

import numpy as np

from tests.test_icp_host import transform_f64

WG = 256
CELL_MAX = 65535
I4 = np.eye(4)


# ------------------------------------------------------------------ the oracle
def oracle(src, tgt, T, max_dist):
    """-> dict: j (n,) winner or -1 where no correspondence, nn (n,) winner regardless of the threshold (-1: no finite d2),
    d2 (n,) of nn (inf where none), mult (n,) number of targets at exactly d2 (the tie's size), n_corr, sum_d2"""
    src, tgt = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    n, m = len(src), len(tgt)
    nn, best, mult = np.full(n, -1, np.int64), np.full(n, np.inf), np.zeros(n, np.int64)
    if n and m:
        p = transform_f64(np.asarray(T, np.float64), src)
        with np.errstate(invalid="ignore", over="ignore"):
            for a in range(0, n, 64):
                d = p[a:a + 64, None, :] - tgt[None]
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                d2 = np.where(np.isfinite(d2), d2, np.inf)                   # a non-finite d2 never wins
                j = d2.argmin(1)                                             # the first minimum: the lowest index
                b = d2[np.arange(len(j)), j]
                fin = np.isfinite(b)
                nn[a:a + 64], best[a:a + 64] = np.where(fin, j, -1), b
                mult[a:a + 64] = np.where(fin, (d2 == b[:, None]).sum(1), 0)
    ok = best < max_dist * max_dist
    return dict(j=np.where(ok, nn, -1), nn=nn, d2=best, mult=mult, n_corr=int(ok.sum()), sum_d2=float(best[ok].sum()))


def implied(o, ns):
    """(fitness, inlier_rmse) that an evaluation implies: the finish kernel's two divisions and its square root"""
    n = float(o["n_corr"])
    return (n / ns if ns else 0.0), (math.sqrt(o["sum_d2"] / n) if n > 0 else 0.0)


# ------------------------------------------------------------------ the grid, restated
def _cell(f, dim):
    return 0 if not f > 0.0 else (dim - 1 if f >= dim - 1 else int(f))


def grid(tgt, max_dist):
    """org, ext, h, hmin, dim of a finite, non-empty target"""
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    lo, hi = tgt.min(0), tgt.max(0)
    ext = float((hi - lo).max())
    h, hmin = float(max_dist), ext / (CELL_MAX - 1)
    if not h >= hmin:
        h = hmin
    if not h > 0.0:
        h = 1.0
    dim = [_cell(math.floor((hi[k] - lo[k]) / h), CELL_MAX + 1) + 1 for k in range(3)]
    return dict(org=lo, ext=ext, h=h, hmin=hmin, dim=dim)


def cell_range(g, box_lo, box_hi, reach):
    """the inclusive cell range (lo[3], hi[3]) of the box padded by reach; hi < lo on an axis = empty"""
    pad = reach * (1.0 + 2.0 ** -20) + 2.0 ** -20
    lo, hi = [], []
    for k in range(3):
        flo = math.floor((box_lo[k] - pad - g["org"][k]) / g["h"])
        fhi = math.floor((box_hi[k] + pad - g["org"][k]) / g["h"])
        lo.append(g["dim"][k] if flo > g["dim"][k] - 1 else _cell(flo, g["dim"][k]))
        hi.append(-1 if fhi < 0 else _cell(fhi, g["dim"][k]))
    return lo, hi


def source_box(src, T):
    p = transform_f64(np.asarray(T, np.float64), np.asarray(src, np.float64))
    p = p[np.isfinite(p).all(1)]
    return p.min(0), p.max(0)


def stream_shape(g, tgt, rg):
    """what icp_stream_cells walks for the range rg: columns, batches of 256 columns, points per batch, tiles, empty columns"""
    lo, hi = rg
    nx, ny = hi[0] - lo[0] + 1, hi[1] - lo[1] + 1
    ncol = nx * ny if nx > 0 and ny > 0 and hi[2] >= lo[2] else 0
    batches = -(-ncol // WG)
    per_batch = np.zeros(batches, np.int64)
    occupied = 0
    if ncol:
        f = np.floor((np.asarray(tgt, np.float64) - g["org"]) / g["h"])
        c = np.stack([np.clip(f[:, k], 0, g["dim"][k] - 1).astype(np.int64) for k in range(3)], 1)
        inside = ((c >= np.array(lo)) & (c <= np.array(hi))).all(1)
        col = (c[inside, 0] - lo[0]) * ny + (c[inside, 1] - lo[1])
        per_batch = np.bincount(col // WG, minlength=batches)
        occupied = len(np.unique(col))
    tiles = -(-per_batch // WG)
    return dict(ncol=ncol, batches=batches, per_batch=per_batch, tiles=tiles, empty_columns=ncol - occupied, points=int(per_batch.sum()))


def shape_of(src, tgt, T, max_dist):
    """grid and stream shape of one pair with ns <= 256 (one workgroup: its box is the source's)"""
    assert 0 < len(src) <= WG
    g = grid(tgt, max_dist)
    rg = cell_range(g, *source_box(src, T), max_dist)
    return g, rg, stream_shape(g, tgt, rg)


# ------------------------------------------------------------------ geometries
def _lattice(nx, ny, nz, spacing=1.0, origin=(0.0, 0.0, 0.0)):
    """x-major lattice, row k = (k // (ny nz), (k // nz) % ny, k % nz)"""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.float64) * spacing + np.asarray(origin, np.float64)


def _shuffle(a, mult):
    """rows in the order k * mult mod n (mult coprime to n): the index order is not the order of the cells"""
    n = len(a)
    assert math.gcd(mult, n) == 1
    return a[(np.arange(n) * mult) % n]


def _pose(R=None, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = t
    return T


def _pre_image(T, p):
    """s with T s = p, exact for a signed permutation rotation and dyadic numbers"""
    return (np.asarray(p, np.float64) - T[:3, 3]) @ T[:3, :3]


QUARTER_Z = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
HALF_X = np.diag([1.0, -1.0, -1.0])

SIZES = [(1, 600), (2, 257), (3, 256), (255, 255), (256, 1), (257, 600), (513, 257), (256, 256), (3, 1), (513, 255)]


def _sizes():
    full = _lattice(9, 9, 9)                                                   # 729 lattice points, z fastest
    srcs = [full[:ns] + np.array([0.125, 0.0, 0.0]) for ns, _ in SIZES]
    tgts = [_shuffle(full[:nt].copy(), 7) if nt % 7 else full[:nt].copy() for _, nt in SIZES]
    return dict(srcs=srcs, tgts=tgts, max_dist=1.25)


def _one_cell_tiles():
    site = lambda k: np.stack([k // 256, (k // 16) % 16, k % 16], -1).astype(np.float64)      # noqa: E731
    tgt = site((np.arange(700) * 7) % 4096) / 64.0
    tgt[650] = tgt[5]                                                          # the same point in the first and the third tile
    tgt[400] = tgt[10] + np.array([1.0 / 64, 0.0, 0.0])                        # neighbours along x: their midpoint is a tie
    src = site((np.arange(64) * 61) % 4096) / 64.0 + np.array([3.0, 5.0, 7.0]) / 512.0
    src[0] = tgt[5]
    src[1] = tgt[10] + np.array([1.0 / 128, 0.0, 0.0])
    return dict(srcs=[src], tgts=[tgt], max_dist=1.0, ties={0: (5, 650), 1: (10, 400)})


def _plane_sources(n, span):
    """n points spread over [0, span]^2 at z = 1/8 (every fourth at z = -1: out of reach), the first two in opposite corners"""
    k = np.arange(n)
    s = np.stack([(k * 37) % (span + 1) + 0.125, (k * 11) % (span + 1) - 0.1875, np.where(k % 4 == 3, -1.0, 0.125)], -1).astype(np.float64)
    s[0], s[1] = (0.125, 0.0625, 0.125), (span - 0.125, span - 0.0625, 0.125)
    return s


def _many_columns(side=95):
    xy = _lattice(side, side, 1)
    tgt = np.concatenate([xy + np.array([0.0, 0.0, z]) for z in (0.0, 0.25, 0.5)])
    mult = next(m for m in (7919, 7907, 7901) if math.gcd(m, len(tgt)) == 1)
    return dict(srcs=[_plane_sources(256, side - 1)], tgts=[_shuffle(tgt, mult)], max_dist=1.0)


def _sparse_columns():
    tgt = _shuffle(_lattice(48, 48, 1, 2.0), 1013)
    return dict(srcs=[_plane_sources(256, 94)], tgts=[tgt], max_dist=1.0)


def _cell_cap():
    k = np.arange(400)
    x = np.floor(k * 96.0 / 399.0 * 4096.0) / 4096.0
    x[-1] = 96.0
    tgt = np.stack([x, (k % 8) * 2.0 ** -15, (k % 5) * 2.0 ** -16], -1)
    src, partner = [], []
    for which, dx in enumerate((2.0 ** -11, 2.0 ** -10, 2.0 ** -10 - 2.0 ** -30)):
        for i in range(64):
            j = 0 if i == 0 else (399 if i == 63 else (i * 19 + which * 5) % 400)
            src.append(tgt[j] + np.array([dx if j < 399 else -dx, 0.0, 0.0]))
            partner.append(j)
    return dict(srcs=[np.array(src)], tgts=[_shuffle(tgt, 7)], max_dist=2.0 ** -10, partner_x=x[np.array(partner)])


def _outside():
    tgt = _shuffle(_lattice(5, 5, 5, 0.5), 7)                                  # the cube [0, 2]^3
    faces = []
    for ax in range(3):
        for side in (0.0, 2.0):
            out = -1.0 if side == 0.0 else 1.0
            for beyond in (0.25, 0.75, 3.0):                                   # within max_dist of a face point, beyond it, far
                for u, v in ((0.5, 1.5), (1.0625, 0.9375), (2.0, 0.0)):
                    p = np.zeros(3)
                    p[ax], p[(ax + 1) % 3], p[(ax + 2) % 3] = side + out * beyond, u, v
                    faces.append(p)
    faces = np.array(faces)
    inside = _lattice(3, 3, 3, 0.5, (0.5625, 0.4375, 0.5))
    far_pos = _lattice(2, 3, 3, 0.5, (4.0, 0.5, 0.5))                          # wholly outside, beyond the reach: lo = dim
    far_neg = _lattice(2, 3, 3, 0.5, (-4.0, 0.5, -3.0))                        # hi = -1 on x and z
    near = _lattice(1, 3, 3, 0.5, (2.25, 0.5, 0.5))                            # wholly outside, within the reach of the face
    srcs = [np.concatenate([faces, inside]), far_pos, far_neg, near]
    return dict(srcs=srcs, tgts=[tgt] * 4, max_dist=0.5)


def _degenerate_extent():
    c = np.array([1.0, 2.0, 3.0])
    ring = np.array([[0.0, 0, 0], [0.25, 0, 0], [0, -0.25, 0.25], [0.5, 0, 0], [0.25, 0.25, 0.25], [0, 0, -0.75], [-0.375, 0.25, 0]])
    cloud = _shuffle(_lattice(5, 5, 5, 0.25), 7)                               # 1 m
    wide = np.concatenate([_lattice(3, 3, 3, 0.375, (0.0625, 0.0625, 0.0625)), [[300.0, -200.0, 100.0], [600.0, 300.0, 0.0], [-20.0, 0.5, 0.5]]])
    tiny = np.array([[0.0, 0, 0], [2.0 ** -12, 0, 0], [0, -2.0 ** -12, 0], [2.0 ** -12, 2.0 ** -12, 0], [0, 0, 1.0]])
    return dict(srcs=[c + ring, c + ring, wide, c + tiny], tgts=[np.tile(c, (50, 1)), c[None], cloud, np.tile(c, (3, 1))],
                max_dist=[0.5, 0.5, 2.0 ** 9, 2.0 ** -12])


def _far_init():
    tgt = _shuffle(_lattice(6, 6, 6, 0.5), 7)
    # where the source lands: beside a target, every third row at exactly max_dist from it; 512 m are 2^17 cells of 2^-8 m
    want = _lattice(5, 5, 5, 0.5) + np.where(np.arange(125)[:, None] % 3 == 0, [[2.0 ** -8, 0.0, 0.0]], [[2.0 ** -9, 2.0 ** -10, -2.0 ** -9]])
    Ts =[_pose(QUARTER_Z, (3.25, -1.5, 0.75)), _pose(HALF_X, (-2.0, 4.125, 1.0)), _pose(None, (512.0, 0.0, 0.0)),
          _pose(QUARTER_Z, (0.0, -512.0, 256.0))]
    srcs = [_pre_image(Ts[0], want), _pre_image(Ts[1], want), want.copy(), want.copy()]
    return dict(srcs=srcs, tgts=[tgt] * 4, T=np.stack(Ts), max_dist=2.0 ** -8)


def _cross_cell_ties():
    # lattice points at the centres of the cells (one more target moves the grid's origin by half a cell), in an index order
    # that is not the order of the cells; sources at cell corners (8 targets), on cell edges (4) and faces (2)
    tgt = np.concatenate([_shuffle(_lattice(4, 4, 4), 23), [[-0.5, -0.5, -0.5]]])
    corners = _lattice(3, 3, 3, 1.0, (0.5, 0.5, 0.5))
    edges = np.concatenate([_lattice(3, 3, 4, 1.0, (0.5, 0.5, 0.0)), _lattice(4, 3, 3, 1.0, (0.0, 0.5, 0.5))])
    faces = np.concatenate([_lattice(3, 4, 4, 1.0, (0.5, 0.0, 0.0)), _lattice(4, 4, 3, 1.0, (0.0, 0.0, 0.5))])
    src = np.concatenate([corners, edges, faces])
    mult = np.array([8] * len(corners) + [4] * len(edges) + [2] * len(faces))
    return dict(srcs=[src], tgts=[tgt], max_dist=1.0, mult=mult)


def _non_finite():
    tgt = _shuffle(_lattice(5, 5, 5, 0.5), 7)
    src = _lattice(4, 4, 3, 0.5, (0.0625, 0.125, 0.1875))[:40]
    srcs, tgts, bad_src, bad_tgt = [], [], [], []
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        s = src.copy()
        s[7 + 11 * k, k] = v                                                   # one source row, another coordinate each time
        srcs.append(s)
        tgts.append(tgt.copy())
        bad_src.append(7 + 11 * k)
        bad_tgt.append(None)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        t = tgt.copy()
        row = int(oracle(src, tgt, I4, 0.5)["nn"][3 + k])                       # a target that a source row would have chosen
        t[row, (k + 1) % 3] = v
        srcs.append(src.copy())
        tgts.append(t)
        bad_src.append(None)
        bad_tgt.append(row)
    return dict(srcs=srcs, tgts=tgts, max_dist=0.5, bad_src=bad_src, bad_tgt=bad_tgt)


BATCH_NS, BATCH_NT = [256, 0, 257, 1, 512, 3], [5, 7, 0, 300, 257, 1]


def _batch():
    full = _lattice(9, 9, 9)
    srcs = [full[:ns] * np.array([1.0, 1.0, 0.5]) + np.array([0.125, -0.0625, 0.25]) for ns in BATCH_NS]
    tgts = [_shuffle(full[:nt].copy(), 7) if nt % 7 else full[:nt].copy() for nt in BATCH_NT]
    return dict(srcs=srcs, tgts=tgts, max_dist=1.0)


_MAKERS = dict(sizes=_sizes, one_cell_tiles=_one_cell_tiles, many_columns=_many_columns, sparse_columns=_sparse_columns,
               cell_cap=_cell_cap, outside=_outside, degenerate_extent=_degenerate_extent, far_init=_far_init,
               cross_cell_ties=_cross_cell_ties, non_finite=_non_finite, batch=_batch)
GEOMETRIES = list(_MAKERS)
FINITE = [n for n in GEOMETRIES if n != "non_finite"]
KNN_CLOUDS = ["many_columns", "sparse_columns", "cell_cap", "one_cell_tiles"]
_CACHE = {}


def geometry(name):
    """-> dict: srcs, tgts (lists of (n,3) float64, one entry per pair), T (P,4,4), max_dist (one float per pair),
    oracle (list of `oracle` results, computed once and shared), and what the geometry plants (ties, partners, bad rows)"""
    if name not in _CACHE:
        g = _MAKERS[name]()
        P = len(g["srcs"])
        g.setdefault("T", np.tile(np.eye(4), (P, 1, 1)))
        if np.isscalar(g["max_dist"]):
            g["max_dist"] = [float(g["max_dist"])] * P
        g["oracle"] = [oracle(g["srcs"][p], g["tgts"][p], g["T"][p], g["max_dist"][p]) for p in range(P)]
        for a in g["srcs"] + g["tgts"]:
            a.setflags(write=False)
        _CACHE[name] = g
    return _CACHE[name]


def calls(name):
    """the device calls of a geometry: one per distinct max_dist -> list of (pair indices, max_dist)"""
    g = geometry(name)
    out = {}
    for p, d in enumerate(g["max_dist"]):
        out.setdefault(d, []).append(p)
    return [(ps, d) for d, ps in out.items()]


# ------------------------------------------------------------------ exact k nearest neighbours of a cloud
def knn_exact(points, knn):
    """(n, knn) indices by (d2, index) ascending with d2 = (dx*dx + dy*dy) + dz*dz, for clouds too large for the all-pairs
    search of knn_f64 (tests/icp_plane_ref.py): the rows are taken in chunks of ascending x, a chunk is compared with every
    point whose x lies within r of the chunk's x range, and r doubles until the m-th smallest d2 of every row of the chunk is
    <= r * r: a point outside the slab is farther than r along x alone, so it is behind the m-th entry.  Inside the slab it is
    brute force; the candidates up to the m-th d2 are ordered by (d2, index).  No cells, no boxes of 256 points."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(p)
    m = min(knn, n)
    out = np.full((n, knn), -1, np.int64)
    if n == 0:
        return out
    by_x = np.argsort(p[:, 0], kind="stable")
    xs = p[by_x, 0]
    r0 = max((xs[-1] - xs[0]) / 64.0, 2.0 ** -20)
    for a in range(0, n, 128):
        rows = by_x[a:a + 128]
        r = r0
        while True:
            lo, hi = np.searchsorted(xs, xs[a] - r, "left"), np.searchsorted(xs, xs[min(a + 128, n) - 1] + r, "right")
            whole = lo == 0 and hi == n
            cand = np.sort(by_x[lo:hi])                                        # ascending index
            if len(cand) >= m:
                d = p[rows, None, :] - p[cand][None]
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                kth = np.partition(d2, m - 1, axis=1)[:, m - 1]
                if whole or (kth <= r * r).all():
                    break
            r = r + r
        rr, cc = np.nonzero(d2 <= kth[:, None])                                # row-major: ascending index inside a row
        order = np.lexsort((cc, d2[rr, cc], rr))
        rr, cc = rr[order], cc[order]
        first = np.searchsorted(rr, np.arange(len(rows)))
        out[rows, :m] = cand[cc[first[:, None] + np.arange(m)[None]]]
    return out
