"""GPU tests of the weight-resident form of the 32 -> 32 fp16-split sparse convolutions (csrc/sconv_split.hip:
sconv_split_resident_kernel; configuration 183, egonn_debug_set_resident).  There is no tolerance anywhere: per output row the
resident form runs the lock-step kernel's operations in the lock-step kernel's order, so it is held to EQUALITY with the lock-step
form (configuration 142) and, on integer data, with the exact integer reference.

a. edge shapes through ctx.sparse_conv: map kinds 0 and 1 onto levels 1 and 2; scans of exactly 1, 15, 16, 17, 127, 128, 129 and
   513 rows at the output level (8 waves x 16 rows is one round of a workgroup, 512 the row-group window) with an empty scan in
   front, between two scans and at the end; a solid cube (all 27 offsets in interior groups); a checkerboard of cells (the centre
   offset only).  Every case at the default grid, with ONE workgroup (it walks every group: the loop over groups wraps many
   times) and with THREE (the group count is no multiple of waves x workgroups).
b. the forms sparse_conv cannot reach (gated input, split-form in / out, the column sums that feed the ECA gate): one eager
   extraction per resident mask, all five returned arrays equal; then the captured pipeline, one capture and two replays.
c. the range guard raises with the resident form on exactly as with it off.
d. a reserved plan with room to spare: canary rows behind the level's rows come back untouched."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

CFG_LOCK, CFG_RESIDENT = 1142, 1183
GRIDS = (0, 1, 3)                       # workgroups per resident launch: default, one, three
COUNTS = (1, 15, 16, 17, 127, 128, 129, 513)


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as entry
    entry.build()
    import egonn_amd
    from egonn_amd import _lib
    egonn_amd._lib = _lib
    return egonn_amd


def _scans(geometry, level):
    s = 1 << level
    if geometry == "row_counts":
        r = [H.row_count_scan(level, n) for n in COUNTS]
        return [None] + r[:4] + [None] + r[4:] + [None]
    if geometry == "solid_cube":        # 6^3 cells and more at the output level, every child voxel present
        return [H.solid_cube(6 * s)]
    assert geometry == "checkerboard"   # cells two apart at the output level: no k=3 neighbour but the cell itself
    return [H.checkerboard(6) * s, None, H.checkerboard(3, origin=(40, 40, 40)) * s]


def _conv(ctx, cfg, grid, kind, level, x, w, sc, sh, relu):
    ctx.lib.egonn_debug_set_naive_conv(ctx.h, cfg)
    ctx.set_resident(-1, grid)
    try:
        return ctx.sparse_conv(kind, level, x, w, sc, sh, relu=relu, group_sums=True)
    finally:
        ctx.lib.egonn_debug_set_naive_conv(ctx.h, 0)
        ctx.set_resident(-1, 0)


# ------------------------------------------------------------------ a. edge shapes
@pytest.mark.parametrize("geometry", ["row_counts", "solid_cube", "checkerboard"])
@pytest.mark.parametrize("kind,level", [(0, 1), (0, 2), (1, 1), (1, 2)])
def test_resident_equals_lock_step_and_the_integer_reference(gpu, geometry, kind, level):
    from oracle import egonn_ref as ref
    c4, B = H.batch_of(_scans(geometry, level))
    lv = ref.SparseLevels(c4)
    ctx = gpu._lib.Context(coord_bits=12)
    ctx.coords_set(torch.from_numpy(np.ascontiguousarray(c4, dtype=np.int32)).cuda(), B)
    lin, _ = H.map_levels(kind, level)
    if geometry == "row_counts":
        off = ctx.level_batch_offsets(level)
        assert [off[b + 1] - off[b] for b in range(B)] == [0, 1, 15, 16, 17, 0, 127, 128, 129, 513, 0]
    pairs = H.oracle_pairs(lv, kind, level)
    if geometry == "solid_cube" and kind == 0:
        assert (np.bincount(pairs[:, 0]) == 27).sum() >= 4 ** 3
    if geometry == "checkerboard" and kind == 0:
        assert len(pairs) == lv.n(level) and (pairs[:, 1] == 13).all()
    p_in = H.join_perm(lv.coords[lin], ctx.level_coords(lin).cpu().numpy())
    p_out = H.join_perm(lv.coords[level], ctx.level_coords(level).cpu().numpy())
    K = H.MAP_K[kind]
    rng = np.random.default_rng(100 * kind + 10 * level + len(geometry))
    x = rng.integers(-8, 9, size=(lv.n(lin), 32))
    w = rng.integers(-8, 9, size=(K, 32, 32))
    scale = rng.choice([0.5, 1.0, 2.0], size=32)
    shift = rng.integers(-8, 9, size=32).astype(np.float64)
    acc = H.int_conv_reference(pairs, x, w, lv.n(level))
    assert np.abs(acc).max(initial=0) < (1 << 24)
    xt = torch.from_numpy(x[p_in].astype(np.float32)).cuda().contiguous()
    wt = torch.from_numpy(w.astype(np.float32)).cuda()
    sc, sh = torch.from_numpy(scale.astype(np.float32)).cuda(), torch.from_numpy(shift.astype(np.float32)).cuda()
    g = torch.Generator(device="cuda").manual_seed(7 + 10 * kind + level)
    xr = torch.randn(xt.shape, device="cuda", generator=g)
    wr = torch.randn(wt.shape, device="cuda", generator=g) / np.sqrt(32 * 9)
    for relu in (False, True):
        want = acc.astype(np.float64) * scale + shift
        want = (np.maximum(want, 0.0) if relu else want)[p_out]
        lock, lock_sums = _conv(ctx, CFG_LOCK, 0, kind, level, xt, wt, sc, sh, relu)
        lock_r, lock_r_sums = _conv(ctx, CFG_LOCK, 0, kind, level, xr, wr, sc, sh, relu)
        assert np.array_equal(lock.cpu().double().numpy(), want), (geometry, kind, level, relu, "lock-step vs reference")
        for grid in GRIDS:
            what = (geometry, kind, level, relu, grid)
            got, sums = _conv(ctx, CFG_RESIDENT, grid, kind, level, xt, wt, sc, sh, relu)
            assert np.array_equal(got.cpu().double().numpy(), want), (what, "integer reference")
            assert torch.equal(got, lock) and torch.equal(sums, lock_sums), (what, "integer data vs cfg 142")
            got, sums = _conv(ctx, CFG_RESIDENT, grid, kind, level, xr, wr, sc, sh, relu)
            assert torch.equal(got, lock_r) and torch.equal(sums, lock_r_sums), (what, "normal data vs cfg 142")
    ctx.plan_status()


# ------------------------------------------------------------------ b. the forms of the forward
KEYS = ("global", "keypoints", "descriptors", "count", "rows")


def test_forward_is_bitwise_the_same_under_every_resident_mask(gpu):
    from egonn_amd.synth import lidar_scan, seeded_state_dict
    E = gpu
    model = E.model_factory(E.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.1))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(7, shapes).items()})
    model = model.to("cuda:0").eval()
    scans = [lidar_scan(2 + i, n_points=6000) for i in range(2)]
    n0, n1 = len(scans[0]), len(scans[1])
    off = [0, n0, n0 + n1, n0 + n1]                       # a third, empty scan
    pts = torch.from_numpy(np.concatenate(scans)).cuda()
    ex = E.DescriptorExtractor(model, n_k=128)
    eager = model.context(1)
    outs = {}
    for mask in (0, 1, 2, 4, 7):
        eager.set_resident(mask, 0)
        outs[mask] = {k: v.clone() for k, v in ex.extract_packed(pts, off, slot=1).items()}
        eager.plan_status()
    eager.set_resident(-1, 0)
    for mask in (1, 2, 4, 7):
        for k in KEYS:
            assert torch.equal(outs[mask][k], outs[0][k]), (mask, k)
    caps = ex.calibrate(pts, off, margin=1.5)
    model.context(0).set_resident(7, 0)
    gx = ex.graph(batch_size=3, max_points=n0 + n1 + 64, level_capacity=caps)
    for rnd in range(3):                                  # the capture and two replays
        out = gx.run(pts, off)
        gx.status()
        for k in KEYS:
            assert torch.equal(out[k], outs[0][k]), (rnd, k)
    assert gx.graph is not None


# ------------------------------------------------------------------ c. range guard
def test_range_guard_raises_with_the_resident_form_as_without(gpu):
    """One level-0 row of 1e4 in every channel and a kernel column of ones: the strided convolution into level 1 leaves ONE
    activation of 3.2e5 (finite in fp32, nothing raised: its operands are in range); the k=3 convolution of level 1 that gathers it
    raises EGONN_STATUS_FP16_RANGE (code 6), resident or not, with the same output bits where they are finite."""
    from egonn_amd.synth import lidar_scan
    Lib = gpu._lib
    scans = [lidar_scan(s, 20000) for s in (21, 22)]
    off = [0, len(scans[0]), len(scans[0]) + len(scans[1])]
    pts = torch.from_numpy(np.concatenate(scans)).cuda()
    ctx = Lib.Context(coord_bits=12)
    ctx.voxelize(pts, off, 0, [0.1])
    g = torch.Generator(device="cuda").manual_seed(11)
    x0 = torch.randn(ctx.level_count(0), 32, device="cuda", generator=g)
    x0[ctx.level_count(0) // 2, :] = 1e4
    w2 = torch.randn(8, 32, 32, device="cuda", generator=g) * 0.05
    w2[:, :, 9] = 1.0
    w3 = torch.randn(27, 32, 32, device="cuda", generator=g) / np.sqrt(32 * 9)
    res = {}
    for mask in (0, 3):
        ctx.voxelize(pts, off, 0, [0.1])                   # a fresh plan: the flag word is per plan
        ctx.set_resident(mask, 0)
        y = ctx.sparse_conv(1, 1, x0, w2)
        ctx.plan_status()                                  # operands in range: no report
        assert int((y.abs() > 65504).sum()) == 1 and bool(torch.isfinite(y).all())
        z = ctx.sparse_conv(0, 1, y, w3)
        with pytest.raises(Lib.Fp16RangeError) as ei:
            ctx.plan_status()
        assert ei.value.code == 6 and not bool(torch.isfinite(z).all())
        res[mask] = (y, z)
    ctx.set_resident(-1, 0)
    assert torch.equal(res[0][0], res[3][0])
    fin = torch.isfinite(res[0][1])
    assert torch.equal(fin, torch.isfinite(res[3][1])) and torch.equal(res[0][1][fin], res[3][1][fin])


# ------------------------------------------------------------------ d. nothing written out of bounds
def test_reserved_plan_canary_rows_stay_untouched(gpu):
    CANARY, EXTRA = 12345.0, 64
    scans = [None, H.row_count_scan(2, 129), H.row_count_scan(2, 17, seed=1) + 300, None]
    c4, B = H.batch_of(scans)
    pts, off = [], [0]
    for b in range(B):
        s = c4[c4[:, 0] == b][:, 1:]
        pts.append(s.astype(np.float32) + np.float32(0.5))  # voxel centres at step 1
        off.append(off[-1] + len(s))
    pts = np.concatenate(pts)
    ctx = gpu._lib.Context(coord_bits=12)
    ctx.reserve(len(pts) + 1000, B, [len(pts) + 1000] * 8)   # room to spare at every level
    buf = np.concatenate([pts, np.zeros((16, 3), dtype=np.float32)])
    ctx.voxelize_device(torch.from_numpy(buf).cuda(), torch.tensor(off, dtype=torch.int64).cuda(), B, 0, [1.0])
    ctx.plan_status()
    ctx.prepare_maps(False)
    g = torch.Generator(device="cuda").manual_seed(3)
    for kind, level in [(0, 1), (0, 2), (1, 1), (1, 2)]:
        lin, _ = H.map_levels(kind, level)
        n, groups = ctx.level_count(level), ctx.map_groups(kind, level)[0]
        assert ctx.level_capacity(level) > n              # the grid is sized by the capacity, the kernel stops at the rows in use
        x = torch.randn(ctx.level_count(lin), 32, device="cuda", generator=g)
        w = torch.randn(H.MAP_K[kind], 32, 32, device="cuda", generator=g) / np.sqrt(32 * 9)
        lock, lock_sums = _conv(ctx, CFG_LOCK, 0, kind, level, x, w, None, None, True)
        for grid in GRIDS:
            out = torch.full((n + EXTRA, 32), CANARY, device="cuda")
            sums = torch.full((groups + EXTRA, 32), CANARY, device="cuda")
            ctx.lib.egonn_debug_set_naive_conv(ctx.h, CFG_RESIDENT)
            ctx.set_resident(-1, grid)
            try:
                ctx._call(ctx.lib.egonn_sparse_conv, ctx.h, kind, level, x.data_ptr(), 32, w.data_ptr(), 32, 0, None, None, 1,
                          out.data_ptr(), sums.data_ptr())
            finally:
                ctx.lib.egonn_debug_set_naive_conv(ctx.h, 0)
                ctx.set_resident(-1, 0)
            assert torch.equal(out[:n], lock), (kind, level, grid)
            assert bool((out[n:] == CANARY).all()), (kind, level, grid, "rows behind the level were written")
            # (sparse_conv hands in zeroed sums: groups without rows keep what was there)
            live = sums[:groups] != CANARY
            assert torch.equal(torch.where(live, sums[:groups], torch.zeros_like(lock_sums)), lock_sums), (kind, level, grid)
            assert bool((sums[groups:] == CANARY).all()), (kind, level, grid, "sums behind the groups were written")
    ctx.plan_status()
