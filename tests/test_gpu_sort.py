"""GPU tests of the two radix sorts of egonn_amd/csrc/sort.hip on their own, through the test hook egonn_debug_radix_sort, bit
for bit against the numpy statement in tests/sort_ref.py (np.array_equal everywhere: a sort has no tolerance).

Every run of a sort here also checks what it must NOT write: both buffer pairs carry 4096 canary elements in front of the first element and behind the capacity,
the scratch carries 256 canary bytes behind the size the library reports, the "out" pair is filled with a canary pattern
before the call, and every element of both pairs from the count on (n, or the device count n_dev) must come back as it was;
in the segmented sort the rows of the result pair outside [off[0], off[B]) as well.

What sits where (sizes and their edges are pinned by tests/test_sort_host.py):
  flat sort       sizes 0 .. 524 289 (wave, workgroup, tile, supertile edges; nine supertiles = a second round of the loop
                  over supertile rows) x nbits 1 .. 64 (1, 2, 5, 8 passes) x result in "out" / in either pair; the device
                  count n_dev; seven key patterns; the whole-digit contract; repeatability
  segmented sort  the offset cases of sort_ref.seg_offset_cases() x nbits 9 .. 64 (1 .. 8 passes) x idx_bits 0 (pairs) / 16 / 28
                  (packed elements: the index field is a permutation, carried and never sorted on); the same patterns; the
                  contract; a segment inside a batch against the same segment alone

The contract the kernels keep (egonn_amd/csrc/common.h): they read whole digits, so key bits between nbits and the end of
the last digit take part in the order, bits from there on are carried and never read.  No call site sets such bits."""
import numpy as np
import pytest
import torch

from tests import sort_ref as R

PAD = 4096                   # canary elements in front of and behind each buffer (two tiles: where a misplaced tile would land)
SCRATCH_PAD = 256            # canary bytes behind the scratch
CANARY_K = np.uint64(0xC0FFEE00DEADBEEF)
CANARY_V = np.uint32(0xABAD1DEA)
U64 = np.uint64


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as entry
    entry.build()
    from egonn_amd import _lib
    return _lib


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U64).view(np.int64)).cuda()


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _host64(t):
    return t.cpu().numpy().view(U64)


def _host32(t):
    return t.cpu().numpy().view(np.uint32)


def _canary_k(n, salt):
    return CANARY_K ^ (np.arange(n, dtype=U64) * U64(0x100000001) + U64(salt))


def _canary_v(n, salt):
    return CANARY_V ^ (np.arange(n, dtype=np.uint32) + np.uint32(salt))


def _launch(gpu, keys, vals, n, nbits, *, count=None, off=None, idx_bits=0, either=False):
    """one call of the hook on fresh buffers -> (result pair index, pairs before, pairs after); pairs = [(keys, vals) of the
    "in" pair, of the "out" pair] as numpy, n + PAD elements each (the PAD canaries IN FRONT of every buffer are checked
    here).  Asserts the scratch canary."""
    assert len(keys) == n == len(vals)
    before = [(np.concatenate([_canary_k(PAD, 5), np.asarray(keys, dtype=U64), _canary_k(PAD, 1)]),
               np.concatenate([_canary_v(PAD, 6), np.asarray(vals, dtype=np.uint32), _canary_v(PAD, 2)])),
              (_canary_k(n + 2 * PAD, 3), _canary_v(n + 2 * PAD, 4))]
    dev = [(_dev64(k), _dev32(v)) for k, v in before]
    B = 0 if off is None else len(off) - 1
    need = gpu.load().egonn_debug_radix_sort_scratch_bytes(n, B)
    assert need > 0 and need % 256 == 0
    scratch = torch.full((need + SCRATCH_PAD,), 0x5C, dtype=torch.uint8, device="cuda")
    assert scratch.data_ptr() % 256 == 0
    n_dev = None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda")
    off_dev = None if off is None else torch.from_numpy(np.asarray(off, dtype=np.int64)).cuda()
    pair = gpu.debug_radix_sort(dev[0][0][PAD:], dev[0][1][PAD:], dev[1][0][PAD:], dev[1][1][PAD:], n, nbits, n_dev=n_dev,
                                seg_offsets=off_dev, idx_bits=idx_bits, either_pair=either, scratch_buf=scratch)
    torch.cuda.synchronize()
    assert bool((scratch[need:] == 0x5C).all()), "the sort wrote behind the scratch size it reports"
    after = [(_host64(k), _host32(v)) for k, v in dev]
    for p in (0, 1):
        for q in (0, 1):
            assert np.array_equal(after[p][q][:PAD], before[p][q][:PAD]), f"the sort wrote in front of a buffer of pair {p}"
    return pair, [(k[PAD:], v[PAD:]) for k, v in before], [(k[PAD:], v[PAD:]) for k, v in after]


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} elements differ, first at {bad[:6].tolist()}: got "
                             f"{[hex(int(x)) for x in got[bad[:3]]]}, want {[hex(int(x)) for x in want[bad[:3]]]}")


def _flat(gpu, keys, vals, nbits, count=None, either=False, what=""):
    """runs the flat sort and checks everything; -> (keys, vals) of the result, m elements"""
    n = len(keys)
    what = f"{what} flat n={n} nbits={nbits} count={count} either={either}"
    pair, before, after = _launch(gpu, keys, vals, n, nbits, count=count, either=either)
    assert pair == R.result_pair_flat(nbits, either) or n == 0, (what, pair)      # (no pass runs on nothing: either answer holds)
    want_k, want_v = R.flat_sort(keys, vals, nbits, count)
    m = len(want_k)
    _same(after[pair][0][:m], want_k, what + " keys")
    _same(after[pair][1][:m], want_v, what + " values")
    for p in (0, 1):                                    # from the count on nothing is written, in either pair
        _same(after[p][0][m:], before[p][0][m:], what + f" keys of pair {p} from the count on")
        _same(after[p][1][m:], before[p][1][m:], what + f" values of pair {p} from the count on")
    return after[pair][0][:m], after[pair][1][:m]


def _segments(gpu, keys, vals, off, nbits, idx_bits=0, what=""):
    """runs the segmented sort and checks everything; -> (keys, vals) of the result pair, n rows"""
    n = len(keys)
    what = f"{what} segments n={n} B={len(off) - 1} nbits={nbits} idx_bits={idx_bits}"
    pair, before, after = _launch(gpu, keys, vals, n, nbits, off=off, idx_bits=idx_bits)
    assert pair == R.result_pair_segments(nbits), (what, pair)
    want_k, want_v = R.segment_sort(keys, vals, off, nbits, idx_bits, before[pair][0][:n], before[pair][1][:n])
    _same(after[pair][0][:n], want_k, what + " keys")            # rows outside [off[0], off[B]) included: as they were
    _same(after[pair][1][:n], want_v, what + " values")
    for p in (0, 1):
        _same(after[p][0][n:], before[p][0][n:], what + f" keys of pair {p} behind n")
        _same(after[p][1][n:], before[p][1][n:], what + f" values of pair {p} behind n")
    return after[pair][0][:n], after[pair][1][:n]


_KEYS = {}


def _random_keys(n):
    if n not in _KEYS:
        _KEYS[n] = R.pattern_keys("random", n, seed=7)
    return _KEYS[n]


# ------------------------------------------------------------------ flat sort
@pytest.mark.gpu
@pytest.mark.parametrize("n", R.FLAT_SIZES)
def test_flat_sizes_and_bits(gpu, n):
    """every size x every nbits x both forms of the result, on 64 random bits with values that use all 32 bits"""
    keys, vals = _random_keys(n), R.scrambled_u32(n)
    for nbits in R.FLAT_NBITS:
        for either in (False, True):
            _flat(gpu, keys, vals, nbits, either=either)


@pytest.mark.gpu
@pytest.mark.parametrize("count", R.NDEV_COUNTS)
def test_flat_device_count(gpu, count):
    """n_dev: only the first min(*n_dev, n) pairs are sorted and only they are written, in both pairs (16 bits: an even number
    of passes, the "out" form starts from a copy of the input; 40 bits: odd)"""
    n = R.NDEV_CAPACITY
    keys, vals = _random_keys(n), R.scrambled_u32(n)
    for nbits in (16, 40):
        for either in (False, True):
            _flat(gpu, keys, vals, nbits, count=count, either=either)
    big = 70000                                                  # a count that ends one key into the second supertile
    if count == 3000:
        for either in (False, True):
            _flat(gpu, _random_keys(big), R.scrambled_u32(big), 16, count=65537, either=either)


PATTERN_SIZES = [65, 257, 2049, 65537, 524289]


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_flat_patterns(gpu, pattern):
    """values = positions, so the returned values ARE the permutation: for equal keys it must be the identity (stability)"""
    for n in PATTERN_SIZES:
        keys = R.pattern_keys(pattern, n)
        pos = np.arange(n, dtype=np.uint32)
        for nbits in (9, 37, 64):
            k, v = _flat(gpu, keys, pos, nbits, either=True, what=pattern)
            if pattern == "equal":
                _same(v, pos, f"{pattern} n={n}: equal keys must keep their order")


@pytest.mark.gpu
def test_flat_reads_whole_digits(gpu):
    """nbits = 37 is five passes = bits [0, 40).  Noise in bits 40..63 changes nothing and comes back intact; bits 37..39 DO
    take part: the contract the kernels keep (common.h), which no call site relies on either way"""
    n = 3 * R.TILE + 77
    rng = np.random.default_rng(37)
    low = rng.integers(0, 1 << 37, size=n, dtype=U64) & U64(0x1F0000FFFF)      # few distinct keys: ties everywhere
    pos = np.arange(n, dtype=np.uint32)
    _, order = _flat(gpu, low, pos, 37)
    noise = rng.integers(0, 1 << 24, size=n, dtype=U64) << U64(40)
    k, v = _flat(gpu, low | noise, pos, 37)
    _same(v, order, "bits from the last digit's end on must not change the order")
    _same(k, (low | noise)[order], "... and come back intact")
    gap = rng.integers(0, 8, size=n, dtype=U64) << U64(37)
    k, v = _flat(gpu, low | gap, pos, 37)                        # (_flat compares with the whole-digit reference)
    on_nbits = np.argsort(low, kind="stable")
    assert not np.array_equal(v, on_nbits), "bits 37..39 were expected to take part in a 37-bit (five-pass) sort"
    _same(v, np.argsort(low | gap, kind="stable").astype(np.uint32), "order on bits [0, 40)")


@pytest.mark.gpu
def test_flat_repeats_bit_for_bit(gpu):
    n = R.FLAT_SIZES[-1]
    keys = R.pattern_keys("runs", n) ^ (_random_keys(n) & U64(0xFF))            # long ties and many digits
    vals = R.scrambled_u32(n)
    a = _flat(gpu, keys, vals, 64, either=True)
    b = _flat(gpu, keys, vals, 64, either=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------ segmented sort
def _seg_input(n, off, nbits, idx_bits, pattern="random"):
    """keys (packed when idx_bits > 0) and values for one segmented run"""
    keys = R.pattern_keys(pattern, n, seed=11, digit=R.SEG_DIGIT)
    if idx_bits:
        return R.pack(keys, off, nbits, idx_bits), np.zeros(n, dtype=np.uint32)      # the values of packed elements are not read
    return keys, R.scrambled_u32(n)


@pytest.mark.gpu
@pytest.mark.parametrize("nbits,idx_bits", R.seg_combos())
def test_segments_edges_batch(gpu, nbits, idx_bits):
    """segments of 0, 1, 2047, 2048, 2049, 0, 16 384, 16 385 and 40 000 keys in one batch"""
    n, off = R.seg_offset_cases()["edges"]
    keys, vals = _seg_input(n, off, nbits, idx_bits)
    _segments(gpu, keys, vals, off, nbits, idx_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in R.seg_offset_cases() if c != "edges"])
def test_segments_offsets(gpu, case):
    n, off = R.seg_offset_cases()[case]
    for nbits, idx_bits in ((27, 0), (64, 0), (48, 16), (36, 28)):
        keys, vals = _seg_input(n, off, nbits, idx_bits)
        _segments(gpu, keys, vals, off, nbits, idx_bits, what=case)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_segments_patterns(gpu, pattern):
    n, off = R.seg_offset_cases()["edges"]
    for nbits, idx_bits in ((64, 0), (27, 0), (48, 16), (36, 28)):
        keys, vals = _seg_input(n, off, nbits, idx_bits, pattern)
        if idx_bits == 0:
            vals = np.arange(n, dtype=np.uint32)
        k, v = _segments(gpu, keys, vals, off, nbits, idx_bits, what=pattern)
        if pattern == "equal" and idx_bits == 0:
            _same(v, vals, f"{pattern}: equal keys must keep their order")
        if pattern == "equal" and idx_bits:                       # the index field comes back in input order: carried, not sorted on
            _same(v, (R.clip_offsets(off, n)[np.searchsorted(off, np.arange(n), side="right") - 1].astype(U64)
                      + (keys & R.bit_mask(0, idx_bits))).astype(np.uint32), f"{pattern}: index fields in input order")


@pytest.mark.gpu
def test_segments_read_whole_digits(gpu):
    """nbits = 48 (the ICP grids) is six passes = bits [0, 54): noise in bits 54..63 changes nothing and comes back intact,
    bits 48..53 take part"""
    n, off = R.seg_offset_cases()["inner"]
    rng = np.random.default_rng(48)
    low = rng.integers(0, 1 << 48, size=n, dtype=U64) & U64(0xF0000003FE01)
    pos = np.arange(n, dtype=np.uint32)
    _, order = _segments(gpu, low, pos, off, 48)
    noise = rng.integers(0, 1 << 10, size=n, dtype=U64) << U64(54)
    k, v = _segments(gpu, low | noise, pos, off, 48)
    _same(v, order, "bits from the last digit's end on must not change the order")
    gap = rng.integers(0, 64, size=n, dtype=U64) << U64(48)
    k, v = _segments(gpu, low | gap, pos, off, 48)
    assert not np.array_equal(v, order), "bits 48..53 were expected to take part in a 48-bit (six-pass) segmented sort"


@pytest.mark.gpu
def test_segments_repeat_and_do_not_depend_on_the_batch(gpu):
    n, off = R.seg_offset_cases()["edges"]
    b = R.SEG_LENGTHS.index(16385)
    lo, hi = int(off[b]), int(off[b + 1])
    alone = np.array([0, hi - lo], dtype=np.int64)
    for nbits, idx_bits in ((64, 0), (48, 16)):
        keys, vals = _seg_input(n, off, nbits, idx_bits, "runs")
        k1, v1 = _segments(gpu, keys, vals, off, nbits, idx_bits)
        k2, v2 = _segments(gpu, keys, vals, off, nbits, idx_bits)
        assert np.array_equal(k1, k2) and np.array_equal(v1, v2)
        ka, va = _segments(gpu, keys[lo:hi], vals[lo:hi], alone, nbits, idx_bits)
        if idx_bits == 0:
            assert np.array_equal(k1[lo:hi], ka) and np.array_equal(v1[lo:hi], va)
        else:                                                     # the packed result names the segment and its first row
            assert np.array_equal(k1[lo:hi] ^ (U64(b) << U64(nbits)), ka) and np.array_equal(v1[lo:hi] - np.uint32(lo), va)


@pytest.mark.gpu
def test_hook_refuses_a_short_scratch(gpu):
    """the same checks as tests/test_entry_points_host.py, on live buffers: nothing is launched, nothing is written"""
    n = 100
    k, v = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    need = gpu.load().egonn_debug_radix_sort_scratch_bytes(n, 0)
    buf = gpu.scratch(need, "cuda")
    with pytest.raises(gpu.EgonnError, match="scratch needs"):
        gpu.debug_radix_sort(k, v, k.clone(), v.clone(), n, 16, scratch_buf=buf, scratch_bytes=need - 1)
