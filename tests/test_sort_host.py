"""CPU tests of tests/sort_ref.py: the numpy statement of the radix sorts against Python's sorted() on small inputs, and the
inputs of tests/test_gpu_sort.py — how many there are and which edge of egonn_amd/csrc/sort.hip each one sits on."""
import numpy as np
import pytest

from tests import sort_ref as R


def _small(n, seed):
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    keys[rng.integers(0, 2, size=n) == 1] &= np.uint64(0xFF00000000000F0F)      # many equal digits: stability shows
    return keys, R.scrambled_u32(n)


def test_masks_and_pass_counts():
    assert [R.passes(b, 8) for b in R.FLAT_NBITS] == [1, 1, 2, 2, 5, 5, 8]      # odd and even pass counts
    assert [R.passes(b, 9) for b in R.SEG_NBITS] == [1, 3, 4, 6, 8]
    assert [R.digits_end(b, 8) for b in R.FLAT_NBITS] == [8, 8, 16, 16, 40, 40, 64]
    assert [R.digits_end(b, 9) for b in R.SEG_NBITS] == [9, 27, 36, 54, 64]    # 8 passes of 9 bits: the last shift is 63
    assert R.digits_end(36, 9, 28) == 64 and R.digits_end(48, 9, 16) == 64 and R.digits_end(27, 9, 16) == 43
    assert int(R.read_mask(37, 8)) == (1 << 40) - 1 and int(R.read_mask(64, 9)) == (1 << 64) - 1
    assert int(R.read_mask(27, 9, 16)) == ((1 << 43) - 1) ^ 0xFFFF
    assert [R.result_pair_flat(b, True) for b in R.FLAT_NBITS] == [1, 1, 0, 0, 1, 1, 0]
    assert all(R.result_pair_flat(b, False) == 1 for b in R.FLAT_NBITS)
    assert [R.result_pair_segments(b) for b in R.SEG_NBITS] == [1, 1, 0, 0, 0]


@pytest.mark.parametrize("nbits", [1, 7, 8, 9, 37, 64])
def test_flat_reference_is_pythons_stable_sort(nbits):
    keys, vals = _small(300, nbits)
    mask = (1 << (8 * ((nbits + 7) // 8))) - 1
    for count in (None, 0, 1, 299, 300, 1000):
        m = 300 if count is None else min(count, 300)
        order = sorted(range(m), key=lambda i: int(keys[i]) & mask)              # sorted() is stable
        k, v = R.flat_sort(keys, vals, nbits, count)
        assert np.array_equal(k, keys[order]) and np.array_equal(v, vals[order]) and k.dtype == np.uint64 and v.dtype == np.uint32


@pytest.mark.parametrize("nbits", [9, 20, 48])
def test_segment_reference_pairs(nbits):
    keys, vals = _small(400, 100 + nbits)
    off = [30, 30, 31, 200, 350, 900]                                           # rows 0..29 and 350..399... are outside / clipped
    prior_k, prior_v = keys ^ np.uint64(1), vals ^ np.uint32(7)
    k, v = R.segment_sort(keys, vals, off, nbits, 0, prior_k, prior_v)
    mask = (1 << min(64, 9 * ((nbits + 8) // 9))) - 1
    want_k, want_v = prior_k.copy(), prior_v.copy()
    for lo, hi in ((30, 31), (31, 200), (200, 350), (350, 400)):
        order = [lo + i for i in sorted(range(hi - lo), key=lambda i: int(keys[lo + i]) & mask)]
        want_k[lo:hi], want_v[lo:hi] = keys[order], vals[order]
    assert np.array_equal(k, want_k) and np.array_equal(v, want_v)
    assert np.array_equal(k[:30], prior_k[:30])                                  # rows in front of off[0]: as they were


@pytest.mark.parametrize("nbits,idx_bits", [(9, 16), (27, 16), (36, 28), (48, 16)])
def test_segment_reference_packed(nbits, idx_bits):
    n, off = 500, [10, 10, 260, 700]
    rng = np.random.default_rng(idx_bits + nbits)
    bits = rng.integers(0, 4, size=n, dtype=np.uint64) << np.uint64(nbits - 2)  # four distinct keys: long ties
    packed = R.pack(bits, off, nbits, idx_bits)
    k, v = R.segment_sort(packed, np.zeros(n, np.uint32), off, nbits, idx_bits)
    for b, (lo, hi) in enumerate(((10, 10), (10, 260), (260, 500))):
        idx = packed[lo:hi] & np.uint64((1 << idx_bits) - 1)
        assert sorted(idx.tolist()) == list(range(hi - lo)) and (hi - lo < 2 or idx.tolist() != list(range(hi - lo)))
        order = sorted(range(hi - lo), key=lambda i: int(packed[lo + i]) >> idx_bits)     # on the sort bits only, stable
        assert [int(x) for x in k[lo:hi]] == [(b << nbits) | (int(packed[lo + i]) >> idx_bits) for i in order]
        assert [int(x) for x in v[lo:hi]] == [lo + int(idx[i]) for i in order]
    assert np.array_equal(k[:10], packed[:10])                                   # outside the segments: the prior content


def test_flat_sizes_sit_on_their_edges():
    assert R.FLAT_SIZES == [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 65536, 65537, 524288, 524289]
    assert [R.tiles(n) for n in (2047, 2048, 2049)] == [1, 1, 2]
    assert [R.supertiles(n) for n in (65536, 65537)] == [1, 2]
    # the scatter kernel sums the supertile rows eight at a time: nine supertiles = a second round of one row
    assert [R.rounds(R.supertiles(n)) for n in (524288, 524289)] == [1, 2]
    # and the earlier tiles of its own supertile eight at a time: the last tile of a full supertile has 31 of them
    assert R.rounds(R.SUPER - 1) == 4 and R.tiles(65536) == R.SUPER
    assert max(R.FLAT_SIZES) * 12 < 6.5e6                                        # the largest input: about 6 MB of pairs
    assert R.NDEV_COUNTS == [0, 1, 3000, 4999, 5000, 7000] and R.tiles(R.NDEV_CAPACITY) == 3 and 3000 % R.TILE != 0


def test_segment_cases_sit_on_their_edges():
    assert [R.tiles(n) for n in R.SEG_LENGTHS] == [0, 1, 1, 1, 2, 0, 8, 9, 20]
    # a scatter workgroup sums the histogram rows of the EARLIER tiles of its segment eight at a time.  The last tile of the
    # 16 385-key segment has eight of them: one full round.  The loop goes round a second time from the tenth tile on, which
    # the 40 000-key segment has (19 earlier tiles for its last one: three rounds, the last one of three rows)
    assert R.rounds(R.tiles(16385) - 1) == 1 and R.rounds(R.tiles(40000) - 1) == 3 and (R.tiles(40000) - 1) % 8 == 3
    cases = R.seg_offset_cases()
    assert sorted(cases) == ["all_past_n", "edges", "inner", "max_batch", "one_segment", "past_n"]
    n, off = cases["edges"]
    assert n == 78914 and len(off) == 10 and off[-1] == n and np.array_equal(np.diff(off), R.SEG_LENGTHS)
    n, off = cases["max_batch"]
    assert len(off) == R.MAX_BATCH + 1 and (np.diff(off) != 0).sum() == 1 and np.diff(off)[R.MAX_BATCH // 2] == n == 4100
    n, off = cases["inner"]
    assert off[0] > 0 and off[-1] < n
    n, off = cases["past_n"]
    c = R.clip_offsets(off, n)
    assert c.tolist() == [0, 3000, 6000, 6000] and off[2] > n and (c[2] - c[1]) % R.TILE == 952       # cut inside its 2nd tile
    n, off = cases["all_past_n"]
    assert (R.clip_offsets(off, n) == n).all()
    assert all((np.diff(o) >= 0).all() for _, o in cases.values())
    assert R.seg_combos() == [(9, 0), (27, 0), (36, 0), (48, 0), (64, 0), (9, 16), (27, 16), (36, 16), (48, 16), (9, 28), (27, 28),
                              (36, 28)]
    assert max(np.diff(off).max() for _, off in cases.values()) <= 1 << 16       # every segment's positions fit 16 index bits


@pytest.mark.parametrize("digit", [8, 9])
def test_patterns(digit):
    n = 3 * R.TILE + 5
    p = {name: R.pattern_keys(name, n, digit=digit) for name in R.PATTERNS}
    assert all(k.dtype == np.uint64 and len(k) == n for k in p.values())
    assert len(np.unique(p["equal"])) == 1
    assert len(np.unique(p["alternating"])) == 2 and (p["alternating"][::2] != p["alternating"][1::2][0]).all()
    assert len(np.unique(p["random"])) == n
    top = np.unique(p["top_bit"])
    assert top.tolist() == [(1 << 63) - 1, (1 << 64) - 1]                        # differ in bit 63 only; ~0 among them
    d = p["one_digit"]
    for q in range(64 // digit + 1):
        vary = len(np.unique((d >> np.uint64(q * digit)) & np.uint64((1 << digit) - 1))) > 1 if q * digit < 64 else False
        assert vary == (q == 2), q
    assert (np.diff(p["descending"].astype(object)) < 0).all()
    r = p["runs"]
    assert len(np.unique(r)) <= 5 and (np.flatnonzero(r[1:] != r[:-1]).size + 1) <= n // (R.TILE // 2) + 1
    assert np.array_equal(R.pattern_keys("runs", n, digit=digit), r)             # reproducible
    for small in (0, 1, 65):
        assert all(len(R.pattern_keys(name, small)) == small for name in R.PATTERNS)
    v = R.scrambled_u32(R.FLAT_SIZES[-1])
    assert len(np.unique(v)) == len(v) and v.max() > (1 << 31) and not np.array_equal(v[:4], np.arange(4))
