"""Plain-numpy statement of the two radix sorts of egonn_amd/csrc/sort.hip and the inputs tests/test_gpu_sort.py feeds them
(tests/test_sort_host.py pins both without a GPU).

The contract (egonn_amd/csrc/common.h): a stable sort that carries keys whole and values with them, and reads WHOLE DIGITS
above the first sorted bit — 8 bits per pass and ceil(nbits / 8) passes for the flat sort, 9 bits per pass and ceil(nbits / 9)
passes for the segmented one.  The order is therefore np.argsort(key & read_mask, kind="stable") per segment, where the mask
covers bits [idx_bits, digits_end): the bits between idx_bits + nbits and digits_end take part, the bits from digits_end on are
carried and never read.  Keys are np.uint64, values np.uint32."""
import numpy as np

TILE = 2048            # keys per workgroup (SORT_TILE)
SUPER = 32             # tiles per supertile of the flat sort (SORT_SUPER)
IN_FLIGHT = 8          # histogram rows a scatter workgroup loads per round of its loops over earlier tiles / supertiles
FLAT_DIGIT, SEG_DIGIT = 8, 9
MAX_BATCH = 4096       # EGONN_MAX_BATCH
U64 = np.uint64
ALL_ONES = U64(0xFFFFFFFFFFFFFFFF)


def passes(nbits, digit):
    return (nbits + digit - 1) // digit


def digits_end(nbits, digit, idx_bits=0):
    """one past the highest key bit the sort reads"""
    return min(64, idx_bits + digit * passes(nbits, digit))


def bit_mask(lo, hi):
    """bits [lo, hi) as np.uint64"""
    assert 0 <= lo <= hi <= 64
    return U64(((1 << hi) - 1) ^ ((1 << lo) - 1))


def read_mask(nbits, digit, idx_bits=0):
    return bit_mask(idx_bits, digits_end(nbits, digit, idx_bits))


def result_pair_flat(nbits, either_pair):
    """0: the result is in the "in" pair, 1: in the "out" pair.  Only a caller that takes either pair can end in "in"."""
    return 0 if either_pair and passes(nbits, FLAT_DIGIT) % 2 == 0 else 1


def result_pair_segments(nbits):
    return passes(nbits, SEG_DIGIT) % 2


def flat_sort(keys, vals, nbits, count=None):
    """-> (keys, vals) of the first min(count, n) pairs in sorted order; count None = n"""
    keys, vals = np.asarray(keys, dtype=U64), np.asarray(vals, dtype=np.uint32)
    m = len(keys) if count is None else max(0, min(int(count), len(keys)))
    order = np.argsort(keys[:m] & read_mask(nbits, FLAT_DIGIT), kind="stable")
    return keys[:m][order], vals[:m][order]


def clip_offsets(off, n):
    return np.minimum(np.asarray(off, dtype=np.int64), n)


def segment_sort(keys, vals, off, nbits, idx_bits=0, prior_keys=None, prior_vals=None):
    """-> (keys, vals), n rows each, as the result pair holds them: every segment [off[b], off[b+1]) (clipped to n) sorted on
    its own, every other row as prior_* has it (default: the input).  idx_bits > 0: `keys` are packed elements, `vals` is not
    read, and the output is key = (segment << nbits) | (packed >> idx_bits), value = clipped off[segment] + index field."""
    keys = np.asarray(keys, dtype=U64)
    n = len(keys)
    out_k = np.array(keys if prior_keys is None else prior_keys, dtype=U64)
    out_v = np.array(vals if prior_vals is None else prior_vals, dtype=np.uint32)
    assert len(out_k) == n == len(out_v)
    o = clip_offsets(off, n)
    mask = read_mask(nbits, SEG_DIGIT, idx_bits)
    for b in range(len(o) - 1):
        lo, hi = int(o[b]), int(o[b + 1])
        if hi <= lo:
            continue
        order = np.argsort(keys[lo:hi] & mask, kind="stable")
        k = keys[lo:hi][order]
        if idx_bits == 0:
            out_k[lo:hi] = k
            out_v[lo:hi] = np.asarray(vals, dtype=np.uint32)[lo:hi][order]
        else:
            out_k[lo:hi] = (U64(b) << U64(nbits)) | (k >> U64(idx_bits))
            out_v[lo:hi] = (U64(lo) + (k & bit_mask(0, idx_bits))).astype(np.uint32)
    return out_k, out_v


# ------------------------------------------------------------------ inputs
# flat sort: n -> the edge it sits on
FLAT_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 65536, 65537, 524288, 524289]
FLAT_NBITS = [1, 8, 9, 16, 37, 40, 64]
NDEV_CAPACITY = 5000                                      # 3 tiles, the last one partial
NDEV_COUNTS = [0, 1, 3000, NDEV_CAPACITY - 1, NDEV_CAPACITY, NDEV_CAPACITY + 2000]
# segmented sort
SEG_LENGTHS = [0, 1, 2047, 2048, 2049, 0, 16384, 16385, 40000]
SEG_NBITS = [9, 27, 36, 48, 64]
SEG_IDX_BITS = [0, 16, 28]
PATTERNS = ["equal", "alternating", "random", "top_bit", "one_digit", "descending", "runs"]


def tiles(n):
    return (n + TILE - 1) // TILE


def supertiles(n):
    return (tiles(n) + SUPER - 1) // SUPER


def rounds(rows):
    """times a loop that takes IN_FLIGHT rows per round goes round for `rows` rows"""
    return (rows + IN_FLIGHT - 1) // IN_FLIGHT


def offsets_of(lengths, first=0):
    return np.concatenate([[first], first + np.cumsum(lengths)]).astype(np.int64)


def seg_combos():
    """(nbits, idx_bits) the segmented sort accepts out of SEG_NBITS x SEG_IDX_BITS"""
    return [(nb, ib) for ib in SEG_IDX_BITS for nb in SEG_NBITS if nb + ib <= 64]


def seg_offset_cases():
    """name -> (n, offsets): n is the capacity of the buffers, the offsets are what the sort is handed (not clipped)"""
    mid = MAX_BATCH // 2
    lens = np.zeros(MAX_BATCH, dtype=np.int64)
    lens[mid] = 4100
    return {
        "edges": (int(np.sum(SEG_LENGTHS)), offsets_of(SEG_LENGTHS)),
        "one_segment": (5000, offsets_of([5000])),
        "max_batch": (4100, offsets_of(lens)),
        "inner": (9000, np.array([300, 2500, 2500, 8000], dtype=np.int64)),            # off[0] > 0, off[B] < n
        "past_n": (6000, np.array([0, 3000, 7000, 12000], dtype=np.int64)),            # segment 1 is cut 952 keys into its 2nd tile
        "all_past_n": (100, np.array([100, 150, 400], dtype=np.int64)),
    }


def pattern_keys(name, n, seed=0, digit=FLAT_DIGIT):
    """n keys (np.uint64) of one of PATTERNS"""
    rng = np.random.default_rng([seed, n, PATTERNS.index(name)])
    i = np.arange(n, dtype=U64)
    if name == "equal":
        return np.full(n, 0x5A5A5A5A5A5A5A5A, dtype=U64)
    if name == "alternating":
        return np.where(i % U64(2) == 0, U64(0xFFFF0000FFFF0001), U64(0x0000FFFF0000FFFE))
    if name == "random":
        return rng.integers(0, 1 << 64, size=n, dtype=U64)
    if name == "top_bit":                       # ~0 (the downsampler's invalid key) and the same key without bit 63
        return np.where(rng.integers(0, 2, size=n) == 1, ALL_ONES, ALL_ONES >> U64(1))
    if name == "one_digit":                     # every digit constant but digit 2
        base = U64(0x0123456789ABCDEF) & ~bit_mask(2 * digit, 3 * digit)
        return base | (rng.integers(0, 1 << digit, size=n, dtype=U64) << U64(2 * digit))
    if name == "descending":
        return (U64(n) - i) * U64(0x0000010000000101)
    if name == "runs":                          # five distinct keys in runs of half a tile to three tiles
        five = rng.integers(0, 1 << 64, size=5, dtype=U64)
        m = n // (TILE // 2) + 1
        ids = np.repeat(rng.integers(0, 5, size=m), rng.integers(TILE // 2, 3 * TILE, size=m))[:n]
        assert len(ids) == n
        return five[ids]
    raise KeyError(name)


def scrambled_u32(n):
    """n distinct values that are not the identity and use all 32 bits: element i is found again by its value"""
    return ((np.arange(n, dtype=U64) * U64(2654435761) + U64(0x9E3779B9)) & U64(0xFFFFFFFF)).astype(np.uint32)


def pack(sort_bits, off, nbits, idx_bits, seed=0):
    """packed elements of the plan sort: (sort bits << idx_bits) | index inside the segment, the index field being a PERMUTATION
    of each segment's positions (clipped to n), not the identity"""
    n = len(sort_bits)
    o = clip_offsets(off, n)
    idx = np.zeros(n, dtype=U64)
    rng = np.random.default_rng([seed, n, idx_bits])
    for b in range(len(o) - 1):
        lo, hi = int(o[b]), int(o[b + 1])
        if hi > lo:
            assert hi - lo <= (1 << idx_bits)
            idx[lo:hi] = rng.permutation(hi - lo).astype(U64)
    return ((np.asarray(sort_bits, dtype=U64) & bit_mask(0, nbits)) << U64(idx_bits)) | idx
