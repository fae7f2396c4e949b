"""Shared helpers for parity tests: golden-fixture loading and coordinate-keyed joins.

Row order is implementation-defined on every side (ME: hash order; oracle: first-appearance;
HIP: Z-order), so every per-row comparison joins on the (b,x,y,z) coordinate first
(SURVEY.md §8c parity protocol)."""
from __future__ import annotations

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["egonn_cart01_b1", "egonn_cart01_b2", "egonn_cart03_b1", "egonn_polar_b1",
         "egonn_cart01_50k_b2"]      # the last one: BASELINE configs[1] cloud size (2 x 50 000 points, 0.1 m)


def load_case(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


MINKLOC_CASES = ["minkloc3d_cart03_b2", "minkloc_eca_cart03"]


def state_dict_shapes(name="egonn"):
    with open(os.path.join(GOLDEN, f"{name}_state_dict_shapes.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}        # dict order = reference state_dict order


def seeded_weights(seed, name="egonn"):
    from egonn_amd.synth import seeded_state_dict
    return seeded_state_dict(int(seed), state_dict_shapes(name))


def rowkey(c4):
    c = np.asarray(c4, dtype=np.int64)
    return ((c[:, 0] * 65536 + (c[:, 1] + 32768)) * 65536 + (c[:, 2] + 32768)) * 65536 + (c[:, 3] + 32768)


def sort_rows(c4):
    c = np.asarray(c4)
    return c[np.argsort(rowkey(c), kind="stable")]


def join_perm(c_from, c_to):
    """perm such that c_from[perm] == c_to row by row (asserts identical coordinate sets)."""
    kf, kt = rowkey(c_from), rowkey(c_to)
    assert len(kf) == len(kt), f"row count differs: {len(kf)} vs {len(kt)}"
    of = np.argsort(kf, kind="stable")
    ot = np.argsort(kt, kind="stable")
    assert np.array_equal(kf[of], kt[ot]), "coordinate sets differ"
    perm = np.empty(len(kt), dtype=np.int64)
    perm[ot] = of
    return perm


def cosine_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    num = (a * b).sum(axis=1)
    den = np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)
    return 1.0 - num / np.maximum(den, 1e-30)


def make_quantizer(case, mod):
    """Build the matching quantiser from module `mod` (oracle.egonn_ref or egonn_amd)."""
    step = case["quantization_step"]
    if str(case["coordinates"]) == "cartesian":
        return mod.CartesianQuantizer(float(step[0]))
    return mod.PolarQuantizer([float(s) for s in step])


def sparse_conv_f64(levels, kind, level_out, x, w):
    """float64 host evaluation of egonn_sparse_conv without epilogue: out[o] = sum_k sum_{(j,o) in map_k} x[j] @ w[k], rows in
    the order of `levels` (oracle.egonn_ref.SparseLevels).  kind 0: k=3 on level_out; 1: k=2/s=2 from level_out-1; 2: transposed
    from level_out+1 (the strided map with input and output swapped, ME's conv_transpose).  Non-finite inputs propagate."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    if kind == 0:
        maps = levels.kmap(level_out, level_out, 3)
    elif kind == 1:
        maps = levels.kmap(level_out - 1, level_out, 2)
    else:
        maps = [(o, j) for j, o in levels.kmap(level_out, level_out + 1, 2)]
    out = np.zeros((levels.n(level_out), w.shape[-1]), dtype=np.float64)
    for k, (j, o) in enumerate(maps):
        if len(j):
            out[o] += x[j] @ w[k]        # every output row appears at most once per offset
    return out


# --------------------------------------------------------------------------------------
# Edge geometries for the plan tests (tests/test_oracle.py pins the oracle on them, tests/test_gpu_maps.py the HIP plan).
# Plain seeded functions, no GPU.  A scan is an (n, 3) int64 array of distinct voxel coordinates.
# --------------------------------------------------------------------------------------
def _grid(n):
    a = np.arange(n, dtype=np.int64)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)


def corner_clusters(cb):
    """the eight 3x3x3 clusters in the corners of the coord_bits = cb range [-2^(cb-1), 2^(cb-1) - 1]^3: (216, 3)"""
    lo, hi = -(1 << (cb - 1)), (1 << (cb - 1)) - 1
    out = []
    for s in range(8):
        base = np.array([lo if (s >> a) & 1 == 0 else hi - 2 for a in range(3)], dtype=np.int64)
        out.append(base + _grid(3))
    return np.concatenate(out)


def face_pairs(cb):
    """(6, 3): per axis one voxel on the low face and one on the high face, the other two coordinates equal (0): were a key to
    wrap at the range's edge, the two would be neighbours.  Rows 2a, 2a+1 are the pair of axis a."""
    lo, hi = -(1 << (cb - 1)), (1 << (cb - 1)) - 1
    out = np.zeros((6, 3), dtype=np.int64)
    for a in range(3):
        out[2 * a, a], out[2 * a + 1, a] = lo, hi
    return out


def corners(cb):
    """corner_clusters(cb) followed by face_pairs(cb): (222, 3).  For cb >= 10 every face voxel is isolated from every other voxel
    at every level 0..7 (the nearest other cell is 2^(cb-1) >= 512 away on some axis, a level-7 step is 128)."""
    return np.concatenate([corner_clusters(cb), face_pairs(cb)])


def solid_cube(n, origin=(-3, -7, -33)):
    """all n^3 voxels of origin + [0, n)^3.  The default origin puts zero and a 4-, a 16- and a 64-block boundary inside the cube
    for n >= 8 (x: -3..: crosses 0 and 4; y: -7..: crosses -4 and 0; z: -33..: crosses -32 = a 16 and 32 boundary; n >= 34
    crosses 0 = a 64 boundary on z too)."""
    return np.asarray(origin, dtype=np.int64) + _grid(n)


def checkerboard(n, origin=(-16, -16, -16)):
    """one voxel of every 2x2x2 cell of a cube of n cells per axis (period-2 checkerboard, origin + 2 * [0, n)^3): no two voxels are
    k=3 neighbours at level 0 (only the centre offset is present), level 1 is a solid n-cube of cells."""
    return np.asarray(origin, dtype=np.int64) + 2 * _grid(n)


def axis_lines(n, origin=(-5, -5, -5)):
    """seven scans: straight lines of n voxels from `origin` along x, y, z and the four space diagonals (+,+,+), (+,+,-), (+,-,+),
    (+,-,-).  Every interior voxel of a line has exactly 3 k=3 entries at level 0 (itself and the two along the line)."""
    o = np.asarray(origin, dtype=np.int64)
    t = np.arange(n, dtype=np.int64)[:, None]
    dirs = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)]
    return [o + t * np.asarray(d, dtype=np.int64) for d in dirs]


def pow2_pairs(cb):
    """cb - 1 scans of two voxels each, scan k = voxels 2^k apart along axis k % 3, placed so that they are k=3 neighbours at level
    k and at no other level (below: further than one step apart; above: one cell — the first sits on a multiple of 2^(k+1),
    alternately at 0 and at -2^(k+1), so that the pairs sit on either side of zero).  Pairs with k >= 8 are never neighbours at
    levels 0..7.  One pair per scan: a batch of many two-row scans."""
    out = []
    for k in range(cb - 1):
        p = 0 if k % 2 == 0 else -(1 << (k + 1))
        a = np.zeros((2, 3), dtype=np.int64)
        a[0, k % 3], a[1, k % 3] = p, p + (1 << k)
        out.append(a)
    return out


def row_count_scan(level, n_rows, seed=0):
    """a scan with exactly n_rows distinct level-`level` cells: a seeded random subset of a cube of cells centred on zero (about
    two thirds full, so that the masks vary), one or two voxels per cell."""
    rng = np.random.default_rng(1000 * level + n_rows + 7919 * seed)
    m = 1
    while m ** 3 * 2 < n_rows * 3:
        m += 1
    cells = _grid(m)[np.sort(rng.choice(m ** 3, size=n_rows, replace=False))] - m // 2
    s = 1 << level
    vox = [cells * s + rng.integers(0, s, size=(n_rows, 3))]
    if s > 1:
        twice = rng.random(n_rows) < 0.5
        vox.append(cells[twice] * s + (vox[0][twice] - cells[twice] * s + 1 + rng.integers(0, s - 1, size=(int(twice.sum()), 3))) % s)
    v = np.unique(np.concatenate(vox), axis=0)
    assert len(np.unique(np.floor_divide(v, s), axis=0)) == n_rows
    return v


def batch_of(scans):
    """scans: list whose entries are an (n, 3) array, None (an empty scan) or an int (a duplicate of that earlier entry under this
    batch index).  Returns ((N, 4) int32 [b, x, y, z] rows in scan order, batch_size)."""
    rows = []
    for b, s in enumerate(scans):
        if isinstance(s, (int, np.integer)):
            s = scans[int(s)]
        if s is None or len(s) == 0:
            continue
        c = np.empty((len(s), 4), dtype=np.int32)
        c[:, 0] = b
        c[:, 1:] = s
        rows.append(c)
    return (np.concatenate(rows) if rows else np.zeros((0, 4), dtype=np.int32)), len(scans)


# --------------------------------------------------------------------------------------
# Kernel maps as sets of (output voxel, weight slot, input voxel), the row-group form of a map, and the comparisons between them.
# --------------------------------------------------------------------------------------
MAP_K = {0: 27, 1: 8, 2: 8}


def map_levels(kind, level_out):
    """(input level, output level) of map kind 0 (k=3 on level_out), 1 (k=2,s=2 into level_out), 2 (transposed onto level_out)"""
    return (level_out, level_out - 1, level_out + 1)[kind], level_out


def oracle_pairs(levels, kind, level_out):
    """(P, 3) int64 rows (out row, slot k, in row) of the oracle's map, rows numbered as in `levels` (oracle.egonn_ref.SparseLevels)"""
    if kind == 0:
        maps = levels.kmap(level_out, level_out, 3)
    elif kind == 1:
        maps = levels.kmap(level_out - 1, level_out, 2)
    else:
        maps = [(o, j) for j, o in levels.kmap(level_out, level_out + 1, 2)]
    out = [np.stack([o, np.full(len(o), k, dtype=np.int64), j], axis=1) for k, (j, o) in enumerate(maps)]
    return np.concatenate(out).astype(np.int64) if out else np.zeros((0, 3), dtype=np.int64)


def triples_by_coord(pairs, c_out, c_in):
    """(out row, k, in row) -> (out key, k, in key), sorted: the row-order-free form of a map (a set, as a sorted array)"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
    if len(p):
        assert p[:, 0].min() >= 0 and p[:, 0].max() < len(c_out), "output row outside the level"
        assert p[:, 2].min() >= 0 and p[:, 2].max() < len(c_in), "input row outside the level"
    t = np.stack([rowkey(c_out)[p[:, 0]], p[:, 1], rowkey(c_in)[p[:, 2]]], axis=1) if len(p) else np.zeros((0, 3), dtype=np.int64)
    t = t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]
    assert len(t) < 2 or (np.diff(t, axis=0) != 0).any(axis=1).all(), "a (output, slot, input) entry appears twice"
    return t


def decode_rowgroups(perm, snbr):
    """perm [G, 16], snbr [G, K, 16] -> (P, 3) rows (out row, slot k, in row) of every entry >= 0 in a slot that holds a row"""
    perm, snbr = np.asarray(perm, dtype=np.int64), np.asarray(snbr, dtype=np.int64)
    g, k, s = np.nonzero((snbr >= 0) & (perm[:, None, :] >= 0))
    return np.stack([perm[g, s], k, snbr[g, k, s]], axis=1)


def check_rowgroup_form(perm, snbr, gmask, n_rows, first_group, batch_offsets):
    """The invariants of the row-group form (csrc/rowgroup.hip) that do not need the reference map; AssertionError on a breach.
    gmask bit order, read from rowgroup.hip: bit k (k < K) is kernel offset k itself — the OR of `(row[k] >= 0) << k` over the
    group's rows; the sort key is remapped (remap27), the stored mask is not — and bit 31 says that the group holds a real row."""
    perm, snbr = np.asarray(perm, dtype=np.int64), np.asarray(snbr, dtype=np.int64)
    gmask = np.asarray(gmask).astype(np.int64) & 0xFFFFFFFF
    G, K, _ = snbr.shape
    assert perm.shape == (G, 16) and gmask.shape == (G,)
    real = perm >= 0
    assert perm.min(initial=0) >= -1 and perm.max(initial=-1) < n_rows, "perm names a row outside the level"
    assert np.array_equal(np.sort(perm[real]), np.arange(n_rows)), "every output row must appear in perm exactly once"
    assert (snbr[~np.broadcast_to(real[:, None, :], snbr.shape)] == -1).all(), "a padding slot has an snbr entry other than -1"
    want = (real.any(axis=1).astype(np.int64) << 31)
    for k in range(K):
        want |= (snbr[:, k, :] >= 0).any(axis=1).astype(np.int64) << k
    assert np.array_equal(gmask, want), "gmask differs from the OR of its group's slots"
    B = len(batch_offsets) - 1
    assert len(first_group) == B + 1 and first_group[0] == 0 and first_group[B] == G
    for b in range(B):
        lo, hi = batch_offsets[b], batch_offsets[b + 1]
        rows = perm[first_group[b]:first_group[b + 1]]
        rows = rows[rows >= 0]
        assert first_group[b] <= first_group[b + 1]
        assert ((rows >= lo) & (rows < hi)).all(), f"the groups of scan {b} hold rows of another scan"
        assert len(rows) == hi - lo, f"scan {b}: {len(rows)} rows in its groups, {hi - lo} in the level"
        if hi == lo:
            assert first_group[b] == first_group[b + 1], f"the empty scan {b} owns groups"


def encode_rowgroups(pairs, K, batch_offsets, win=64):
    """Row-group form of a map given as (out row, k, in row) rows, built on the host the plain way (per scan: windows of `win`
    rows, groups of 16 in row order, no mask sort): the synthetic CORRECT table set of the CPU tests.
    Returns perm, snbr, gmask (uint32 values in int64), first_group."""
    gpw = win // 16
    first, perm = [0], []
    for b in range(len(batch_offsets) - 1):
        lo, hi = int(batch_offsets[b]), int(batch_offsets[b + 1])
        for w0 in range(lo, hi, win):
            p = np.full(win, -1, dtype=np.int64)
            p[:min(win, hi - w0)] = np.arange(w0, min(w0 + win, hi))
            perm.append(p.reshape(gpw, 16))
        first.append(sum(len(p) for p in perm))
    perm = np.concatenate(perm) if perm else np.zeros((0, 16), dtype=np.int64)
    G = len(perm)
    n_rows = int(batch_offsets[-1])
    slot = np.full(n_rows, -1, dtype=np.int64)
    g, s = np.nonzero(perm >= 0)
    slot[perm[g, s]] = g * 16 + s
    snbr = np.full((G, K, 16), -1, dtype=np.int64)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
    snbr[slot[p[:, 0]] // 16, p[:, 1], slot[p[:, 0]] % 16] = p[:, 2]
    gmask = ((perm >= 0).any(axis=1).astype(np.int64) << 31)
    for k in range(K):
        gmask |= (snbr[:, k, :] >= 0).any(axis=1).astype(np.int64) << k
    return perm, snbr, gmask, first


def assert_same_map(got_triples, want_triples, what=""):
    """set equality of two maps in the sorted (out key, k, in key) form"""
    got, want = np.asarray(got_triples), np.asarray(want_triples)
    assert got.shape == want.shape, f"{what}: {len(got)} map entries, the reference has {len(want)}"
    assert np.array_equal(got, want), f"{what}: map entries differ from the reference"


# the first layer: W[k, 0, k // 4] = 2^(k % 4) makes output channel c of a unit-feature k=5 convolution the presence bits of
# offsets 4c .. 4c+3
def k5_probe_kernel():
    w = np.zeros((125, 1, 32), dtype=np.float32)
    k = np.arange(125)
    w[k, 0, k // 4] = 2.0 ** (k % 4)
    return w


def decode_k5_presence(out):
    """(N, 32) output of the probe convolution on unit features -> (N, 125) bool presence of every 5x5x5 offset"""
    out = np.asarray(out)
    v = np.rint(out).astype(np.int64)
    assert np.array_equal(v.astype(out.dtype), out) and v.min(initial=0) >= 0 and v.max(initial=0) <= 15, "not a 4-bit presence code"
    k = np.arange(125)
    return ((v[:, k // 4] >> (k % 4)) & 1).astype(bool)


def oracle_k5_presence(maps, n_rows):
    """kernel_map(c0, c0, 5, 1) -> (N, 125) bool, rows in the oracle's order"""
    p = np.zeros((n_rows, 125), dtype=bool)
    for k, (j, o) in enumerate(maps):
        p[o, k] = True
    return p


def int_conv_reference(pairs, x, w, n_out):
    """exact integer convolution out[o] = sum over (o, k, j) of x[j] @ w[k]: float64 arithmetic on integer data (every product
    and partial sum an integer far below 2^53, so float64 is exact), returned as int64"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    out = np.zeros((n_out, w.shape[-1]), dtype=np.float64)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
    for k in range(w.shape[0]):
        sel = p[p[:, 1] == k]
        if len(sel):
            np.add.at(out, sel[:, 0], x[sel[:, 2]] @ w[k])
    r = np.rint(out).astype(np.int64)
    assert np.array_equal(r.astype(np.float64), out)
    return r


# --------------------------------------------------------------------------------------
# Edge batches and the stage comparison of tests/test_forward_f64_host.py / tests/test_gpu_forward_stages.py
# --------------------------------------------------------------------------------------
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLAR_STEP = [1.0, 0.3, 0.2]            # the polar fixture's steps (tests/golden/make_golden.py): 360 azimuth bins
EDGE_WEIGHT_SEED = 23


def kernel_constant(name):
    """the value of `constexpr int <name> = N;` in egonn_amd/csrc (LH_WAVES, SEG_CHUNKS): the tiles the edge batches straddle"""
    import re
    for f in ("dense.hip", "kernels.h"):
        with open(os.path.join(_REPO, "egonn_amd", "csrc", f)) as fh:
            m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", fh.read())
        if m:
            return int(m.group(1))
    raise KeyError(name)


def head_tile_counts():
    """level-3 row counts on each side of a wave's 16 rows, of 64 rows and of a workgroup's 16 * LH_WAVES rows"""
    wg = 16 * kernel_constant("LH_WAVES")
    return sorted({1, 15, 16, 17, 63, 64, 65, wg - 1, wg, wg + 1})


def pool_chunk_counts():
    """level-5 row counts: fewer rows than SEG_CHUNKS chunks (chunks with zero rows and with one row), one on each side of it,
    and one more than a 256-row window"""
    ch = kernel_constant("SEG_CHUNKS")
    return [1, ch - 1, ch, ch + 1, 257]


def lidar_voxels(seed, n_points, step=0.1):
    from egonn_amd.synth import lidar_scan
    return np.unique(np.floor(lidar_scan(seed, n_points) / np.float32(step)).astype(np.int64), axis=0)


def _many_tiny_scans():
    """64 scans of 1-5 voxels with empty scans inside (the geometry of tests/test_gpu_maps.py:_many_scans)"""
    rng = np.random.default_rng(64)
    return [None if b in (0, 13, 14, 40, 63) else row_count_scan(0, 1 + b % 5, seed=b) + rng.integers(-200, 200, size=3)
            for b in range(64)]


def _seam_scan():
    """polar voxels (azimuth bin, ring, z) in the first and the last azimuth bins of POLAR_STEP: next to the +-180 degree seam"""
    nb = int(360.0 // POLAR_STEP[0])
    return np.array([(t, r, z) for t in (0, 1, nb - 2, nb - 1) for r in (3, 40, 200) for z in (-5, 0)], dtype=np.int64)


# name -> (coord_bits, coordinates, scans)
EDGE_BATCHES = {
    "ragged": (12, "cartesian", lambda: [np.array([[3, -2, 5]]), np.array([[-900, 0, 0], [900, 0, 0]]), lidar_voxels(9, 40), None,
                                         lidar_voxels(8, 3000), None]),
    "head_tiles": (12, "cartesian", lambda: [row_count_scan(3, n) for n in head_tile_counts()]),
    "pool_chunks": (12, "cartesian", lambda: [row_count_scan(5, n) for n in pool_chunk_counts()]),
    "many_scans": (10, "cartesian", _many_tiny_scans),
    "corners_cb10_cart": (10, "cartesian", lambda: [corners(10)]),
    "corners_cb16_cart": (16, "cartesian", lambda: [corners(16)]),
    "corners_cb10_polar": (10, "polar", lambda: [corners(10), _seam_scan()]),
    "corners_cb16_polar": (16, "polar", lambda: [corners(16), _seam_scan()]),
    "lidar10k": (12, "cartesian", lambda: [lidar_voxels(77, 10000)]),
}
RANGE_CORNER_BATCHES = [n for n in EDGE_BATCHES if n.startswith("corners")]
_EDGE_CACHE = {}


class EdgeBatch:
    """an edge batch: c4 (N, 4) int32, B scans, coord_bits, the quantizer (mode, step), the oracle's pyramid lv (batch_size = B,
    trailing empty scans included) and seeded non-constant level-0 features"""

    def __init__(self, name):
        from oracle import egonn_ref as ref
        self.name = name
        self.cb, coordinates, make = EDGE_BATCHES[name]
        self.c4, self.B = batch_of(make())
        lo, hi = -(1 << (self.cb - 1)), (1 << (self.cb - 1)) - 1
        assert self.c4[:, 1:].min() >= lo and self.c4[:, 1:].max() <= hi and len(self.c4) <= 9100, name        # "about 8 500": the 10 k-point scan has 9 015 voxels
        self.coordinates = coordinates
        self.mode = 0 if coordinates == "cartesian" else 1
        self.step = [0.1] if self.mode == 0 else list(POLAR_STEP)
        self.lv = ref.SparseLevels(self.c4)
        self.lv.batch_size = self.B
        self.scan = {l: self.lv.coords[l][:, 0].astype(np.int64) for l in range(8)}

    def features(self):
        """non-constant level-0 features in (0.5, 1.5), one per row of lv.coords[0], a function of the coordinate"""
        k = rowkey(self.lv.coords[0]).astype(np.uint64)
        h = (k * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
        return (0.5 + h.astype(np.float64) / float(1 << 24)).astype(np.float32).reshape(-1, 1)


def edge_batch(name):
    if name not in _EDGE_CACHE:
        _EDGE_CACHE[name] = EdgeBatch(name)
    return _EDGE_CACHE[name]


def edge_weights():
    return seeded_weights(EDGE_WEIGHT_SEED)


# ---- the comparison: e = max |got - want| / max |want|, over a stage's output and per scan of the batch
FP32_FLOOR = 16 * 2.0 ** -24           # floor of a bound whose e_ref happens to be tiny
SPLIT_CONV = 3e-6                      # README / include/egonn_hip.h / test_split_conv_matches_exact_fp32: one split-pipe convolution
SPLIT_HEADS = 3e-6                     # test_local_heads_input_beyond_fp16_range_is_reported: the split heads against exact
SPARSE_CONVS = {"conv0": 0, "block": 3, "local": 1, "global": 2}       # sparse convolutions per stage (conv0 is exact: bf16 x 3)
BF16_ROUNDINGS = {"conv0": 1, "block": 4, "local": 2, "global": 4}     # bf16 stores between a stage's observed input and output


def stage_kind(stage):
    return "block" if stage.startswith("block") else stage.split(".")[0]


def rel_err(got, want):
    """max |got - want| / max |want| in float64; 0 for two all-zero arrays, inf for a non-zero got against an all-zero want"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    d, m = float(np.abs(got - want).max()), float(np.abs(want).max())
    if not np.isfinite(d):
        return float("inf")
    return d / m if m > 0 else (0.0 if d == 0 else float("inf"))


def scan_errs(got, want, scan, B):
    """rel_err per scan (rows with scan[row] == b): each scan held to its own scale; None for a scan without rows"""
    return [rel_err(got[scan == b], want[scan == b]) if (scan == b).any() else None for b in range(B)]


def stage_bound(stage, config, e_ref):
    """config 'exact': 8 x e_ref (another summation order, not another algorithm), floor 16 x 2^-24; 'product': plus 3e-6 per split
    sparse convolution of the stage and 3e-6 for the split heads; 'bf16': roundings x 2^-8 (a derived count)"""
    kind = stage_kind(stage)
    if config == "bf16":
        return BF16_ROUNDINGS[kind] * 2.0 ** -8
    b = max(8.0 * e_ref, FP32_FLOOR)
    if config == "product":
        b += SPLIT_CONV * SPARSE_CONVS[kind] + (SPLIT_HEADS if kind == "local" else 0.0)
    return b


def worst_entry(got, want, rows=None):
    """(row, channel, got, want) of the largest |got - want| (row an index into `rows` if given)"""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    d = d.reshape(len(d), -1)
    r, c = np.unravel_index(int(np.argmax(d)), d.shape)
    g, w = np.asarray(got).reshape(len(d), -1)[r, c], np.asarray(want).reshape(len(d), -1)[r, c]
    return (int(rows[r]) if rows is not None else int(r)), int(c), float(g), float(w)


def check_stage(table, batch, config, stage, got, want, ref32, scan, B, gate=None, exact_zero=(), min_share=1.0):
    """One stage of one forward against float64.  got: the GPU's output (None on the host: only e_ref is recorded), want: the float64
    stage on the same input, ref32: the fp32 oracle's stage on that input (None for bf16).  The whole output and every scan (in its
    own scale; bound from the larger of the batch's and the scan's own e_ref: a scan of a few rows samples the stage's rounding
    poorly) must stay inside stage_bound; the scans listed in exact_zero have an all-zero float64 output and must be exactly zero.
    min_share < 1 (bf16 keypoints / sigma only, the rule of test_local_heads_range_bf16_maps): instead, that share of the rows lies
    within bound x max |want|.  Appends (batch, config, stage, e_ref, e_gpu, bound) to `table`; returns the failure messages."""
    want = np.asarray(want, dtype=np.float64)
    e_ref = rel_err(ref32, want) if ref32 is not None else 0.0
    bound = stage_bound(stage, config, e_ref)
    if got is None:
        table.append((batch, config, stage, e_ref, None, bound))
        return []
    got = np.asarray(got, dtype=np.float64)
    fails = []
    if not np.isfinite(got).all():
        fails.append(f"{batch}/{config}/{stage}: NaN or Inf in the output")
    e_gpu = rel_err(got, want)
    table.append((batch, config, stage, e_ref, e_gpu, bound))

    def describe(rows_mask, b):
        rows = np.nonzero(rows_mask)[0]
        r, c, g, w = worst_entry(got[rows_mask], want[rows_mask], rows)
        s = f"worst row {r} channel {c}: got {g!r}, float64 {w!r}"
        if gate is not None and b is not None and c < gate.shape[1]:
            s += f", float64 gate[{b}][{c}] = {gate[b, c]:.6f}"
        return s

    if min_share < 1.0:
        ok = np.abs(got - want).reshape(len(got), -1).max(axis=1) <= bound * np.abs(want).max()
        if ok.mean() < min_share:
            fails.append(f"{batch}/{config}/{stage}: {ok.mean():.4f} of the rows within {bound:.3e} x max|want|, {min_share} required")
        return fails
    if not e_gpu <= bound:
        r, c, _, _ = worst_entry(got, want)
        fails.append(f"{batch}/{config}/{stage}: e_gpu {e_gpu:.3e} > bound {bound:.3e} (e_ref {e_ref:.3e}); "
                     + describe(np.ones(len(got), dtype=bool), int(scan[r]) if len(scan) == len(got) else None))
    if len(scan) == len(got):
        eg = scan_errs(got, want, scan, B)
        er = scan_errs(ref32, want, scan, B) if ref32 is not None else [0.0] * B
        for b in range(B):
            if eg[b] is None:
                continue
            m = scan == b
            if b in exact_zero:
                assert not want[m].any()
                if got[m].any():
                    fails.append(f"{batch}/{config}/{stage} scan {b}: float64 output is all zero, the GPU's is not; " + describe(m, b))
                continue
            bb = stage_bound(stage, config, max(e_ref, er[b]))
            if not eg[b] <= bb:
                fails.append(f"{batch}/{config}/{stage} scan {b} ({int(m.sum())} rows): e_gpu {eg[b]:.3e} > bound {bb:.3e} "
                             f"(e_ref of the scan {er[b]:.3e}, of the batch {e_ref:.3e}); " + describe(m, b))
    return fails


def format_table(table):
    """stage x configuration x batch: e_ref, e_gpu, bound — one line per entry"""
    out = [f"{'batch':<20}{'config':<10}{'stage':<14}{'e_ref':>11}{'e_gpu':>11}{'bound':>11}"]
    for batch, config, stage, e_ref, e_gpu, bound in table:
        g = "-" if e_gpu is None else f"{e_gpu:.2e}"
        out.append(f"{batch:<20}{config:<10}{stage:<14}{e_ref:>11.2e}{g:>11}{bound:>11.2e}")
    return "\n".join(out)
