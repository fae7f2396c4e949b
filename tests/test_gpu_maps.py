"""GPU tests of the coordinate plan itself (csrc/coords.hip, csrc/rowgroup.hip): the kernel maps and their row-group form are
compared ENTRY BY ENTRY, without a tolerance, with the numpy oracle's kernel map (oracle/me_ops.py:kernel_map, pinned on the
same geometries by tests/test_oracle.py), and the convolution kernels that consume them are run on integer data, where the
result does not depend on the summation order, and compared with np.array_equal / torch.equal.

Which geometry covers which edge (builders in tests/helpers.py; every geometry is legal input, every plan has room to spare):
  corners_cb{10,12,16}   the edge of the coordinate range at every level: 3x3x3 clusters in the eight corners (the +1 / -1
                         neighbour does not exist; the virtual top levels' range test) and voxel pairs on opposite faces (a
                         key that wrapped would pair them); coord_bits = 16 holds -32768; an empty scan in front, the same
                         cloud again under another batch index (identical clouds in scans b and b + 2 never pair up)
  solid_cube             mask extremes: all 27 offsets for 18^3 interior rows, every 4x4x4 occupancy mask full, the cube
                         straddling zero and the 4 / 16 / 32 block boundaries; 8 000 rows = 15 full windows + a partial one;
                         a second, small cube whose origin sits ON the 64 boundaries
  checkerboard           the other extreme: only the centre offset at level 0, solid at level 1
  lines                  seven scans, one line each along x, y, z and the four space diagonals; an empty scan at the end
  pow2_pairs_cb{..}      one scan per k with two voxels 2^k apart: neighbours at level k only; many scans of two rows
  many_scans             64 scans of 1-5 voxels with empty scans inside: windows and groups never straddle scans
  row_counts_L{1,4,7}    scans with exactly 1, 15, 16, 17, 511, 512, 513, 1024, 1025 rows AT level L (7: 1..17): partial windows,
                         trailing empty groups, padding slots, for the 512-row (L <= 3) and the 256-row windows; empty scans in
                         front, inside and at the end; one scan twice
Every geometry is planned three ways — egonn_coords_set (shuffled caller order, some rows twice), egonn_voxelize from points at
voxel centres (tables built on first use) and a reserved plan (egonn_ctx_reserve with room to spare, egonn_voxelize_device,
egonn_prepare_maps) — and every map of the plan is read: k=3 on levels 1..7, stride 2 into levels 1..7, transposed onto levels 0..6.

gmask bit order (read from rowgroup.hip): bit k is kernel offset k itself (the sort key is remapped, the stored mask is not),
bit 31 = the group holds a real row.  tests/helpers.py:check_rowgroup_form states and checks it.

Convolutions: on every map of every plan one channel plan (cycling through all nine instantiated pairs, 256 -> 256 and 128 -> 256
among them, so that each pair meets each map kind and each kernel family) runs through EVERY kernel family: the product
dispatch, the exact fp32 kernels (set_exact_fp32), the plain kernel (which reads the raw nbr tables, not the row groups), the
MFMA variants 2 / 4 / 16 / 32, the split variants 1142 / 1182 / 1542 / 1942, on levels >= 3 the offset-part rules of
tests/test_gpu_ksplit.py, and the bf16 maps.  Data: integers in [-8, 8] (bf16: {-1, 0, 1}), epilogue scale in {0.5, 1, 2},
integer shift, ReLU on every second map: every partial sum is an integer below 2^24 (27 x 256 x 64 = 442 368), exact in fp32 and
as fp16 hi + lo under a power-of-two pack scale.  No kernel family needed the fallback bound: all of them are held to equality.

Not covered here: the weight gradients (part d of the issue) — conv_backward_weight keeps its float64 test in
tests/test_gpu_train_ops.py."""
import time

import numpy as np
import pytest
import torch

from tests import helpers as H


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as entry
    entry.build()
    import egonn_amd
    from egonn_amd import _lib
    egonn_amd._lib = _lib
    return egonn_amd


COUNTS = [1, 15, 16, 17, 511, 512, 513, 1024, 1025]


def _row_counts(level, counts):
    s = [H.row_count_scan(level, n) for n in counts]
    if len(counts) < 9:
        return [None] + s + [None, 1, None]
    return [None] + s[:4] + [None] + s[4:7] + [6] + s[7:] + [None]       # entry 6 = the 511-row scan, a second time


def _many_scans():
    rng = np.random.default_rng(64)
    out = []
    for b in range(64):
        out.append(None if b in (0, 13, 14, 40, 63) else H.row_count_scan(0, 1 + b % 5, seed=b) + rng.integers(-200, 200, size=3))
    return out


GEOMETRIES = {}
for _cb in (10, 12, 16):
    GEOMETRIES[f"corners_cb{_cb}"] = (_cb, lambda cb=_cb: [None, H.corners(cb), 1])
    GEOMETRIES[f"pow2_pairs_cb{_cb}"] = (_cb, lambda cb=_cb: H.pow2_pairs(cb))
GEOMETRIES["solid_cube"] = (12, lambda: [H.solid_cube(20), H.solid_cube(6, origin=(-64, 0, 64))])
GEOMETRIES["checkerboard"] = (12, lambda: [H.checkerboard(16)])
GEOMETRIES["lines"] = (12, lambda: H.axis_lines(40) + [None])
GEOMETRIES["many_scans"] = (10, _many_scans)
GEOMETRIES["row_counts_L1"] = (12, lambda: _row_counts(1, COUNTS))
GEOMETRIES["row_counts_L4"] = (12, lambda: _row_counts(4, COUNTS))
GEOMETRIES["row_counts_L7"] = (12, lambda: _row_counts(7, COUNTS[:4]))
NAMES = list(GEOMETRIES)
WAYS = ("coords_set", "voxelize", "reserved")
MAPS = [(0, l) for l in range(1, 8)] + [(1, l) for l in range(1, 8)] + [(2, l) for l in range(0, 7)]
PLANS = [(32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (64, 32), (128, 64), (256, 256), (128, 256)]


def _build(gpu, way, c4, B, cb, seed):
    ctx = gpu._lib.Context(coord_bits=cb)
    rng = np.random.default_rng(seed)
    if way == "coords_set":
        rows = np.concatenate([c4, c4[rng.integers(0, len(c4), size=7)]])          # duplicate rows collapse
        rows = np.ascontiguousarray(rows[rng.permutation(len(rows))], dtype=np.int32)
        ctx.coords_set(torch.from_numpy(rows).cuda(), B)
        ctx.prepare_maps(with_level0_transpose=True)
        return ctx
    pts, off = [], [0]
    for b in range(B):
        s = c4[c4[:, 0] == b][:, 1:]
        if len(s):
            s = np.concatenate([s, s[rng.integers(0, len(s), size=3)]])            # some voxels hold two points
            s = s[rng.permutation(len(s))]
        pts.append(s.astype(np.float32) + np.float32(0.5))                          # voxel centres at step 1
        off.append(off[-1] + len(s))
    pts = np.concatenate(pts)
    if way == "voxelize":
        ctx.voxelize(torch.from_numpy(pts).cuda(), off, 0, [1.0])                   # tables are built on first use
        return ctx
    cap = len(pts) + 1000
    ctx.reserve(cap, B)
    buf = np.concatenate([pts, np.zeros((16, 3), dtype=np.float32)])                # rows beyond the last offset are ignored
    ctx.voxelize_device(torch.from_numpy(buf).cuda(), torch.tensor(off, dtype=torch.int64).cuda(), B, 0, [1.0])
    ctx.plan_status()
    ctx.prepare_maps(with_level0_transpose=True)
    return ctx


_CASES = {}


def _case(gpu, name):
    """the geometry, its oracle levels and its three plans (built once per module)"""
    if name not in _CASES:
        from oracle import egonn_ref as ref
        cb, make = GEOMETRIES[name]
        c4, B = H.batch_of(make())
        lo, hi = -(1 << (cb - 1)), (1 << (cb - 1)) - 1
        assert c4[:, 1:].min() >= lo and c4[:, 1:].max() <= hi and len(c4) <= 8500
        lv = ref.SparseLevels(c4)
        ctxs = {w: _build(gpu, w, c4, B, cb, 17 + i) for i, w in enumerate(WAYS)}
        _CASES[name] = (c4, B, lv, ctxs)
    return _CASES[name]


def _gpu_levels(ctx, lv, B):
    """level coordinates in plan row order; the levels hold the oracle's cells, batch-contiguous, with the stated offsets"""
    coords = {}
    for l in range(8):
        c = ctx.level_coords(l).cpu().numpy()
        H.join_perm(lv.coords[l], c)                                # identical coordinate sets (asserts)
        off = ctx.level_batch_offsets(l)
        want = [int((lv.coords[l][:, 0] < b).sum()) for b in range(B + 1)]
        assert off == want, (l, off, want)
        for b in range(B):
            assert (c[off[b]:off[b + 1], 0] == b).all(), (l, b)
        coords[l] = c
    return coords


def _tables(ctx, kind, level):
    ng, first = ctx.map_groups(kind, level)
    gm, sn = ctx.rowgroup_tables(kind, level)
    pm = ctx.rowgroup_perm(kind, level)
    assert gm.shape[0] == ng == pm.shape[0]
    return pm.cpu().numpy(), sn.cpu().numpy(), gm.cpu().numpy(), first


# ------------------------------------------------------------------ a. tables, entry by entry
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_tables_equal_the_reference_map(gpu, name):
    t0 = time.time()
    c4, B, lv, ctxs = _case(gpu, name)
    want = {}
    per_way = {}
    for way in WAYS:
        ctx = ctxs[way]
        coords = _gpu_levels(ctx, lv, B)
        for kind, level in MAPS:
            lin, _ = H.map_levels(kind, level)
            if (kind, level) not in want:
                want[kind, level] = H.triples_by_coord(H.oracle_pairs(lv, kind, level), lv.coords[level], lv.coords[lin])
            pm, sn, gm, first = _tables(ctx, kind, level)
            what = f"{name} / {way} / map kind {kind} onto level {level}"
            try:
                H.check_rowgroup_form(pm, sn, gm, len(coords[level]), first, ctx.level_batch_offsets(level))
            except AssertionError as e:
                raise AssertionError(f"{what}: {e}") from None
            got = H.triples_by_coord(H.decode_rowgroups(pm, sn), coords[level], coords[lin])
            H.assert_same_map(got, want[kind, level], what)
            per_way[way, kind, level] = got
        ctx.plan_status()
    for kind, level in MAPS:                                        # the three ways of building the plan agree with each other
        for way in WAYS[1:]:
            assert np.array_equal(per_way[way, kind, level], per_way[WAYS[0], kind, level]), (name, way, kind, level)
    print(f"{name}: {sum(len(v) for v in want.values())} map entries x 3 plans, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ b. convolutions through those tables, exact
def _operands(lv, kind, level, ci, co, bf16, seed):
    """integer operands in the oracle's row order and the exact result (float64 holding integers and halves)"""
    lin, _ = H.map_levels(kind, level)
    rng = np.random.default_rng(seed)
    m = 1 if bf16 else 8
    x = rng.integers(-m, m + 1, size=(lv.n(lin), ci))
    w = rng.integers(-m, m + 1, size=(H.MAP_K[kind], ci, co))
    scale = rng.choice([0.5, 1.0, 2.0], size=co)
    shift = rng.integers(-8, 9, size=co).astype(np.float64)
    acc = H.int_conv_reference(H.oracle_pairs(lv, kind, level), x, w, lv.n(level))
    assert np.abs(acc).max(initial=0) < (1 << 24)
    return x, w, scale, shift, acc.astype(np.float64) * scale + shift


def _group_sums_reference(out_rows, perm):
    """(G, C) sums of the output rows that perm assigns to every group (float64; exact: at most 16 values below 2^21)"""
    p = np.asarray(perm, dtype=np.int64)
    padded = np.concatenate([out_rows, np.zeros((1, out_rows.shape[1]))])
    return padded[np.where(p >= 0, p, len(out_rows))].sum(axis=1)


KSPLIT = {0: [(1, 0), (1, 2), (1, 3), (1, 4), (3, 0), (9, 0), (27, 0), (3, 2)],
          1: [(1, 0), (1, 2), (1, 3), (1, 4), (2, 0), (4, 0), (8, 0), (2, 2)]}


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_convolutions_are_exact_on_integer_data(gpu, name):
    t0 = time.time()
    c4, B, lv, ctxs = _case(gpu, name)
    gi = NAMES.index(name)
    n_conv = 0
    for mi, (kind, level) in enumerate(MAPS):
        ci, co = PLANS[(mi + gi) % len(PLANS)]
        relu = bool(mi % 2)
        lin, _ = H.map_levels(kind, level)
        ops32 = _operands(lv, kind, level, ci, co, False, 1000 * gi + mi)
        ops16 = _operands(lv, kind, level, ci, co, True, 5000 + 1000 * gi + mi)
        for way in WAYS:
            ctx = ctxs[way]
            what = (name, way, kind, level, ci, co)
            p_in = H.join_perm(lv.coords[lin], ctx.level_coords(lin).cpu().numpy())
            p_out = H.join_perm(lv.coords[level], ctx.level_coords(level).cpu().numpy())
            perm = ctx.rowgroup_perm(kind, level).cpu().numpy()

            def run(ops, dtype, variant, sums=True):
                x, w, scale, shift, out = ops
                want = np.maximum(out, 0.0) if relu else out
                want = want[p_out]
                xt = torch.from_numpy(x[p_in].astype(np.float32)).cuda().to(dtype).contiguous()
                wt = torch.from_numpy(w.astype(np.float32)).cuda()
                sc, sh = torch.from_numpy(scale.astype(np.float32)).cuda(), torch.from_numpy(shift.astype(np.float32)).cuda()
                r = ctx.sparse_conv(kind, level, xt, wt, sc, sh, relu=relu, group_sums=sums)
                got, gs = r if sums else (r, None)
                want_t = torch.from_numpy(want).to(torch.float32)                   # exact: integers and halves below 2^24
                assert np.array_equal(want_t.double().numpy(), want)
                if dtype == torch.bfloat16:
                    want_t = want_t.to(torch.bfloat16)                              # the exact value, rounded once on the CPU
                if not torch.equal(got.cpu(), want_t):
                    bad = (got.cpu().float() != want_t.float()).any(dim=1).nonzero().squeeze(1)
                    raise AssertionError(f"{what} variant {variant} {dtype}: {len(bad)} of {len(want)} rows differ, first rows "
                                         f"{bad[:8].tolist()}")
                if sums and dtype == torch.float32:
                    assert np.array_equal(gs.cpu().double().numpy(), _group_sums_reference(want, perm)), (what, variant, "group sums")
                return 1

            lib, h = ctx.lib, ctx.h
            n_conv += run(ops32, torch.float32, "product")
            ctx.set_exact_fp32(True)
            n_conv += run(ops32, torch.float32, "exact fp32")
            ctx.set_exact_fp32(False)
            ctx.set_naive_conv(True)
            n_conv += run(ops32, torch.float32, "plain", sums=False)
            mc = 0 if kind == 0 else 1
            for var in (2, 4, 16, 32, 1142, 1182, 1542, 1942):
                lib.egonn_debug_set_naive_conv(h, var)
                if var > 1142:              # offset parts exist for the 4-wave workgroups (cfg 142) only: the other decompositions
                    ctx.set_ksplit(mc, level, kparts=1, kw=0, col_parts=0)          # run without them, as in tests/test_gpu_graph.py
                n_conv += run(ops32, torch.float32, var)
            if level >= 3 and ci >= 64:     # the offset-part rules of tests/test_gpu_ksplit.py (instantiated for Cin >= 64)
                lib.egonn_debug_set_naive_conv(h, 1142)
                for kp, kw in KSPLIT[mc]:
                    ctx.set_ksplit(mc, level, kparts=kp, kw=kw, col_parts=0)
                    n_conv += run(ops32, torch.float32, ("ksplit", kp, kw))
            ctx.set_ksplit(mc, level, kparts=1, kw=(2 if 3 <= level <= 5 else 0), col_parts=0)          # back to the product rule
            for var in (0, 2, 4, 16, 32):
                lib.egonn_debug_set_naive_conv(h, var)
                n_conv += run(ops16, torch.bfloat16, var)
            lib.egonn_debug_set_naive_conv(h, 0)
    for way in WAYS:
        ctxs[way].plan_status()                                                     # the range-guard flag stayed down
    print(f"{name}: {n_conv} convolutions exact, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ c. the first layer's 5x5x5 map
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_first_layer_map_bit_for_bit(gpu, name):
    from oracle import me_ops as ops
    c4, B, lv, ctxs = _case(gpu, name)
    maps5 = lv.kmap(0, 0, 5)
    want = H.oracle_k5_presence(maps5, lv.n(0))
    w = H.k5_probe_kernel()
    rng = np.random.default_rng(NAMES.index(name))
    x = rng.integers(-8, 9, size=(lv.n(0), 1))
    w2 = rng.integers(-8, 9, size=(125, 1, 32))
    pairs5 = np.concatenate([np.stack([o, np.full(len(o), k), j], axis=1) for k, (j, o) in enumerate(maps5)])
    want2 = H.int_conv_reference(pairs5, x, w2, lv.n(0))
    for way in WAYS:
        ctx = ctxs[way]
        p0 = H.join_perm(lv.coords[0], ctx.level_coords(0).cpu().numpy())
        out = ctx.conv(0, 0, 5, None, torch.from_numpy(w)).cpu().numpy()            # the unit-feature path
        got = H.decode_k5_presence(out)
        if not np.array_equal(got, want[p0]):
            r, k = np.argwhere(got != want[p0])[0]
            raise AssertionError(f"{name} / {way}: {(got != want[p0]).sum()} presence bits differ, first: row {r} "
                                 f"{ctx.level_coords(0)[r].tolist()} offset {ops.kernel_offsets(5, 1)[k].tolist()}")
        ones = torch.ones((lv.n(0), 1), device="cuda")
        assert np.array_equal(ctx.conv(0, 0, 5, ones, torch.from_numpy(w)).cpu().numpy(), out), (name, way)     # the general path
        out2 = ctx.conv(0, 0, 5, torch.from_numpy(x[p0].astype(np.float32)).cuda(), torch.from_numpy(w2.astype(np.float32)))
        assert np.array_equal(out2.cpu().double().numpy(), want2[p0].astype(np.float64)), (name, way, "integer features")
        ctx.plan_status()
