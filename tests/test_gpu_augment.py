"""GPU tests of the device augmentation (egonn_amd/csrc/augment.hip, egonn_amd/augment.py) against the host restatement
(tests/augment_ref.py): the parameter record, the per-point flags and the positions, at the kernels' tile and workgroup
sizes, with every stage switched off on its own, and the bitwise invariants (rerun, batch independence, graph replay).

Bounds: integers and decisions are exact; the record's doubles are within 8 float64 ulps (log / cos / sin are within
4 ulps of the true value on the device and in NumPy alike); positions are within the counted bound E of augment_ref; a
row's block membership may differ from the float64 answer only inside E + band of a block face, for at most 0.1 % of a
scan's rows (augment_ref.check)."""
import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests.test_augment_host import gpu_inputs, _block_seed

pytestmark = pytest.mark.gpu
FILL = -777.25
ULP8 = 8 * 2.0 ** -52


@pytest.fixture(scope="module")
def aug():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    from egonn_amd import augment
    return augment


def _params(aug, P):
    return aug.AugmentParams(seed=P.seed, stages=P.stages, sigma=P.sigma, clip=P.clip if P.stages & R.JITTER_CLIP else None,
                             r_min=P.r_min, r_max=P.r_max, max_delta=P.max_delta, max_theta=P.max_theta, block_p=P.block_p,
                             scale=P.scale, ratio=P.ratio, set_max_theta=P.set_max_theta, flip_p=P.flip_p, rot_max=P.rot_max,
                             trans_max=P.trans_max)


def _run(aug, pts, off, ids, P, cap=None, T_in=None):
    """-> (out (cap,3), removed, erased, rec_i, rec_d, T_out) as numpy; the output starts filled with FILL"""
    from egonn_amd import _lib
    dev = _lib.require_gpu()
    n = len(pts) if cap is None else cap
    d_pts = torch.full((max(n, 1), 3), 5.0, dtype=torch.float32, device=dev)[:n]
    d_pts[:len(pts)] = torch.from_numpy(np.asarray(pts, np.float32)).to(dev)
    out = torch.full((n, 3), FILL, dtype=torch.float32, device=dev)
    d_off = torch.tensor(np.asarray(off, np.int64), device=dev)
    d_ids = torch.tensor(np.asarray(ids, np.int32), device=dev)
    res = aug.augment_points(d_pts.contiguous(), d_off, d_ids, _params(aug, P), draw=P.draw, set_id=P.set_id, out=out,
                             record=True, flags=True, T_in=None if T_in is None else torch.from_numpy(T_in).to(dev))
    torch.cuda.synchronize()
    fl = res.flags.cpu().numpy()
    return (out.cpu().numpy(), (fl & 1) > 0, (fl & 2) > 0, res.rec_i.cpu().numpy(), res.rec_d.cpu().numpy(),
            None if res.T_out is None else res.T_out.cpu().numpy())


def _close(a, b, scale=1.0):
    return abs(a - b) <= ULP8 * max(abs(a), abs(b), scale)


def _check_all(aug, pts, off, ids, P, cap=None, what=None):
    out, removed, erased, ri, rd, _ = _run(aug, pts, off, ids, P, cap)
    live = int(off[-1])
    assert (out[live:] == np.float32(FILL)).all(), (what, "rows beyond the live count were written")
    r32 = R.augment(pts[:live], off, ids, P, np.float32)
    wi, wd = R.records(r32, P)
    assert np.array_equal(ri.astype(np.int64) & 0xFFFFFFFF, wi & 0xFFFFFFFF), (what, ri, wi)
    for b, d in enumerate(r32["scans"]):
        e_max = float(r32["E"][int(off[b]):int(off[b + 1])].max(initial=0.0)) if d["n"] else 0.0
        for k in (0, 4, 7, 20, 23, 24, 30):
            assert _close(rd[b, k], wd[b, k], 0.0), (what, b, k, rd[b, k], wd[b, k])
        for k in (1, 2, 3):
            assert _close(rd[b, k], wd[b, k], 7.0 * P.max_delta), (what, b, k)
        for k in (5, 6, 21, 22, 25, 26):
            assert _close(rd[b, k], wd[b, k], 1.0), (what, b, k)
        assert rd[b, 27] == wd[b, 27] and rd[b, 28] == wd[b, 28]
        if P.stages & R.BLOCK and d["n"]:
            assert np.abs(rd[b, 8:14] - wd[b, 8:14]).max() <= 2 * e_max, (what, b, "box")
            if d["block_on"]:
                band = max(d["band"]) + 2 * e_max
                assert np.abs(rd[b, 14:20] - wd[b, 14:20]).max() <= band, (what, b, "block", rd[b, 14:20], wd[b, 14:20])
    shares = R.check(pts[:live], off, ids, P, out[:live], removed[:live], erased[:live])
    assert max(shares, default=0.0) <= 0.001, (what, shares)
    return out, removed, erased, r32


@pytest.mark.parametrize("mode", [1, 2])
def test_record_flags_and_positions_against_the_restatement(aug, mode):
    pts, off, ids = gpu_inputs()
    P = _block_seed((R.MODE1 | R.SET1) if mode == 1 else (R.MODE2 | R.SET2))
    out, removed, erased, r32 = _check_all(aug, pts, off, ids, P, what=mode)
    assert removed.sum() == sum(d["k"] for d in r32["scans"]) and erased[:5000].sum() > 10
    # against the fp32 restatement the device may differ only where a normal sits one fp32 step off: next to never
    assert (out != r32["out"]).any(axis=1).mean() <= 0.001
    P2 = _block_seed((R.MODE1 | R.SET1) if mode == 1 else (R.MODE2 | R.SET2), on=False)
    _check_all(aug, pts, off, ids, P2, what=(mode, "no block"))


@pytest.mark.parametrize("sizes", [
    [0], [1], [0, 0, 0], [5, 0, 9], [9], [10], [11],                      # int(n r) = 0 for n <= 10 (r < 0.1)
    [255], [256], [257], [1023], [1024], [1025],                          # the apply tile (256) and the select workgroup (1024)
    [15], [16], [17], [4095, 4096, 4097],                                 # the 16 chunks and 16 x 256 lanes of the box pass
    [300, 0, 0, 700, 0], [256, 256, 512],                                 # empty scans inside; boundaries on tile boundaries
])
def test_sizes_at_the_tile_and_workgroup_edges(aug, sizes):
    from egonn_amd import augment as A
    assert (A.TILE, A.SELECT_WG, A.BOX_CHUNKS, A.BOX_WG) == (256, 1024, 16, 256)
    pts, off = R.batch(sum(sizes) + 1, sizes)
    ids = [3 + 5 * b for b in range(len(sizes))]
    for stages in (R.MODE2 | R.SET1, R.MODE1 | R.SET2):
        P = R.Params(seed=len(sizes), draw=5, set_id=1, stages=stages, block_p=1.0)
        _check_all(aug, pts, off, ids, P, what=sizes)


@pytest.mark.parametrize("r", [0.0, 0.1, 1.0])
def test_removal_ratio_at_both_ends(aug, r):
    pts, off = R.batch(8, [3000, 1])
    P = R.Params(seed=4, stages=R.MODE1 | R.SET1, r_min=r, r_max=r)
    out, removed, _, _ = _check_all(aug, pts, off, [1, 2], P, what=r)
    assert removed[:3000].sum() == int(3000 * r) and removed[3000:].sum() == int(1 * r)


def test_large_scan_and_full_batch(aug):
    pts, off = R.batch(200, [200_000])
    _check_all(aug, pts, off, [11], R.Params(seed=6, draw=9, stages=R.MODE2 | R.SET1, block_p=1.0), what="200k")
    rng = np.random.default_rng(32)
    sizes = rng.integers(48_000, 52_000, 32).tolist()
    pts, off = R.batch(32, sizes)
    _check_all(aug, pts, off, list(range(100, 132)), R.Params(seed=7, draw=2, set_id=5, stages=R.MODE1 | R.SET1), what="32 x 50k")


def test_identical_points_and_capacity(aug):
    pts = np.tile(np.array([[3.5, -2.25, 0.5]], np.float32), (2000, 1))
    off = np.array([0, 2000], np.int64)
    # all stages that move points differently are off: the box has zero area, the strict comparisons erase nothing
    P = R.Params(seed=1, stages=R.TRANSLATE | R.BLOCK | R.FLIP, block_p=1.0)
    out, _, erased, r32 = _check_all(aug, pts, off, [4], P, what="zero-area box")
    assert not erased.any() and r32["scans"][0]["block_on"] and r32["scans"][0]["block"]["w"] == 0.0
    _check_all(aug, pts, off, [4], R.Params(seed=1, stages=R.MODE2 | R.SET1, block_p=1.0), what="identical, jittered")
    # n is a capacity: rows behind offsets[B] are neither read (they hold 5.0) nor written (FILL stays)
    pts, off = R.batch(9, [700, 0, 1300])
    for extra in (1, 256, 5000):
        _check_all(aug, pts, off, [1, 2, 3], R.Params(seed=2, stages=R.MODE2 | R.SET1, block_p=1.0), cap=2000 + extra, what=extra)


@pytest.mark.parametrize("off_stage", [R.JITTER, R.JITTER_CLIP, R.REMOVE_POINTS, R.TRANSLATE, R.ROTATE, R.BLOCK, R.SET_ROTATE,
                                       R.FLIP, R.RIGID])
def test_every_stage_switched_off_alone(aug, off_stage):
    pts, off, ids = gpu_inputs()
    full = R.MODE2 | R.SET1 | R.RIGID
    stages = full & ~off_stage
    if off_stage == R.JITTER:
        stages &= ~R.JITTER_CLIP
    P = R.Params(seed=13, draw=1, set_id=3, stages=stages, block_p=1.0, rot_max=0.5, trans_max=2.0)
    out, removed, erased, _ = _check_all(aug, pts, off, ids, P, what=off_stage)
    assert (removed.sum() == 0) == (off_stage == R.REMOVE_POINTS) and (erased.sum() == 0) == (off_stage == R.BLOCK)
    if off_stage == R.JITTER_CLIP:
        assert R.augment(pts, off, ids, P, np.float64)["scans"][0]["jitter_normal"].max() > 2.0      # the clip mattered


def test_all_stages_off_is_a_copy(aug):
    pts, off, ids = gpu_inputs()
    out = _run(aug, pts, off, ids, R.Params(stages=0))[0]
    assert np.array_equal(out, pts)


def test_in_place_equals_out_of_place(aug):
    """out_points may be points itself (include/egonn_hip.h): the same bits, with the block's box taken before any store"""
    from egonn_amd import _lib
    dev = _lib.require_gpu()
    pts, off, ids = gpu_inputs()
    P = R.Params(seed=19, draw=2, set_id=4, stages=R.MODE2 | R.SET1 | R.RIGID, block_p=1.0, rot_max=0.4, trans_max=1.5)
    want = _run(aug, pts, off, ids, P)[0]
    d_pts = torch.from_numpy(pts).to(dev)
    d_off = torch.tensor(np.asarray(off, np.int64), device=dev)
    d_ids = torch.tensor(np.asarray(ids, np.int32), device=dev)
    res = aug.augment_points(d_pts, d_off, d_ids, _params(aug, P), draw=P.draw, set_id=P.set_id, out=d_pts)
    torch.cuda.synchronize()
    assert res.points.data_ptr() == d_pts.data_ptr() and np.array_equal(d_pts.cpu().numpy(), want)


def test_parameters_of_a_switched_off_stage_are_not_judged(aug):
    pts, off = R.batch(6, [800, 400])
    # out-of-range values everywhere but in the two stages that run
    P = R.Params(seed=2, stages=R.TRANSLATE | R.FLIP, sigma=0.0, clip=-1.0, r_min=0.9, r_max=0.1, max_theta=1e9, block_p=7.0,
                 scale=(1.0, 0.0), ratio=(0.0, -1.0), set_max_theta=1e9, rot_max=-1.0, trans_max=-1.0)
    _check_all(aug, pts, off, [1, 2], P, what="off-stage parameters")
    for bad in (dict(stages=R.JITTER, sigma=0.0), dict(stages=R.REMOVE_POINTS, r_min=0.9, r_max=0.1),
                dict(stages=R.BLOCK, ratio=(0.0, 1.0)), dict(stages=R.RIGID, rot_max=-1.0), dict(stages=R.TRANSLATE, max_delta=-0.1)):
        with pytest.raises(Exception, match="augment"):
            _run(aug, pts, off, [1, 2], R.Params(seed=2, **bad))


def test_rigid_pose_update(aug):
    pts, off = R.batch(5, [900, 1100])
    T_in = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    T_in[0, :3, 3] = [1.5, -2.0, 0.25]
    T_in[1, :2, :2] = [[0.6, -0.8], [0.8, 0.6]]
    P = R.Params(seed=21, draw=4, stages=R.RIGID, rot_max=np.pi, trans_max=5.0)
    out, _, _, ri, rd, T = _run(aug, pts, off, [8, 9], P, T_in=T_in)
    r32 = R.augment(pts, off, [8, 9], P, np.float32, T_in=T_in)
    for b in range(2):
        m = np.eye(4, dtype=np.float32)
        c, s = np.float32(np.cos(rd[b, 24])), np.float32(np.sin(rd[b, 24]))
        m[0, 0], m[0, 1], m[1, 0], m[1, 1], m[0, 3], m[1, 3] = c, s, -s, c, rd[b, 27], rd[b, 28]
        # T_gt = m @ transform of the RECORDED draw, fp32, 4-term sums in ascending order: bit for bit
        want = np.zeros((4, 4), np.float32)
        for r in range(4):
            for q in range(4):
                acc = np.float32(0)
                for k in range(4):
                    acc = np.float32(acc + np.float32(m[r, k] * T_in[b, k, q]))
                want[r, q] = acc
        assert np.array_equal(T[b], want) and np.array_equal(T[b], r32["T_out"][b])
    R.check(pts, off, [8, 9], P, out, np.zeros(2000, bool), np.zeros(2000, bool))


def test_rerun_and_batch_independence_are_bitwise(aug):
    pts, off, ids = gpu_inputs()
    P = R.Params(seed=17, draw=3, set_id=9, stages=R.MODE2 | R.SET1 | R.RIGID, block_p=1.0, rot_max=0.3, trans_max=1.0)
    a = _run(aug, pts, off, ids, P)
    b = _run(aug, pts, off, ids, P)
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x, y)
    # every scan alone, and inside another batch at another position: the same bits
    order = [6, 0, 3, 5, 2, 4, 1]
    parts = [pts[off[i]:off[i + 1]] for i in order]
    off2 = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    c = _run(aug, np.concatenate(parts), off2, [ids[i] for i in order], P)
    for pos, i in enumerate(order):
        assert np.array_equal(c[0][off2[pos]:off2[pos + 1]], a[0][off[i]:off[i + 1]]), i
        assert np.array_equal(c[4][pos], a[4][i])
        alone = _run(aug, pts[off[i]:off[i + 1]], [0, off[i + 1] - off[i]], [ids[i]], P)
        assert np.array_equal(alone[0], a[0][off[i]:off[i + 1]]), i
    # another draw counter or seed is another augmentation
    assert not np.array_equal(_run(aug, pts, off, ids, R.Params(**{**P.__dict__, "draw": 4}))[0], a[0])


def test_graph_replay_with_new_offsets_equals_eager(aug):
    from egonn_amd import _lib
    dev = _lib.require_gpu()
    cap, B = 30_000, 4
    P = R.Params(seed=23, draw=1, set_id=2, stages=R.MODE2 | R.SET1, block_p=1.0)
    d_pts = torch.zeros((cap, 3), dtype=torch.float32, device=dev)
    d_off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    d_ids = torch.zeros(B, dtype=torch.int32, device=dev)
    out = torch.zeros((cap, 3), dtype=torch.float32, device=dev)
    scratch = torch.empty(aug.scratch_bytes(cap, B) + 256, dtype=torch.uint8, device=dev)
    params = _params(aug, P)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        aug.augment_points(d_pts, d_off, d_ids, params, draw=P.draw, set_id=P.set_id, out=out, scratch=scratch)   # warm-up
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            aug.augment_points(d_pts, d_off, d_ids, params, draw=P.draw, set_id=P.set_id, out=out, scratch=scratch)
    for sizes, ids in (([5000, 0, 7000, 1], [1, 2, 3, 4]), ([12_000, 9000, 300, 8000], [9, 8, 7, 6])):
        pts, off = R.batch(sum(sizes), sizes)
        d_pts[:len(pts)] = torch.from_numpy(pts).to(dev)
        d_off.copy_(torch.from_numpy(off).to(dev))
        d_ids.copy_(torch.tensor(ids, dtype=torch.int32, device=dev))
        out.fill_(FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        eager = _run(aug, pts, off, ids, P, cap=cap)[0]
        assert np.array_equal(got, eager), sizes


def test_fields_that_do_not_fit_fail_loudly(aug):
    from egonn_amd import _lib
    dev = _lib.require_gpu()
    pts, off = R.batch(3, [500, 500])
    d_pts, d_off = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    p = aug.AugmentParams(seed=1, stages=R.MODE1)
    with pytest.raises(ValueError):
        aug.augment_points(d_pts, d_off, None, p, draw=1 << 14)
    with pytest.raises(ValueError):
        aug.augment_points(d_pts, d_off, None, p, set_id=1 << 22)
    with pytest.raises(ValueError):
        aug.scratch_bytes(1 << 24, 2)
    with pytest.raises(ValueError):
        aug.TrainTransform(1)(d_pts, off, [0, 1 << 22], 0)
    # ids that live on the device are checked there: the scan is marked and its points are NaN, its neighbour is untouched
    ids = torch.tensor([1 << 22, 5], dtype=torch.int32, device=dev)
    res = aug.augment_points(d_pts, d_off, ids, p, record=True)
    torch.cuda.synchronize()
    assert res.rec_i[:, 4].tolist() == [aug.STATUS_BAD_ID, 0]
    o = res.points.cpu().numpy()
    assert np.isnan(o[:500]).all() and np.isfinite(o[500:]).all()
    for cls, kw in ((aug.RandomScale, dict(min=0.9, max=1.1)), (aug.RandomShear, {}), (aug.JitterPoints, dict(p=0.5)),
                    (aug.RandomRotation, dict(axis=None)), (aug.RandomRotation, dict(axis=np.array([0, 0, 1]), max_theta2=5))):
        with pytest.raises(NotImplementedError):
            cls(**kw)


def test_reference_call_sites_on_one_cloud(aug):
    pts = R.cloud(77, 3000)
    t = aug.TrainTransform(2, seed=31)
    a = t(torch.from_numpy(pts))
    assert a.device.type == "cpu" and a.shape == (3000, 3) and a.dtype == torch.float32
    P = R.Params(seed=31, draw=0, set_id=0, stages=R.MODE2)
    R.check(pts, [0, 3000], [0], P, a.numpy(), *[R.augment(pts, [0, 3000], [0], P)[k] for k in ("removed", "erased")])
    b = t(torch.from_numpy(pts))                                       # the second call is another draw (scan id 1)
    assert not torch.equal(a, b)
    s = aug.TrainSetTransform(1, seed=31)(torch.from_numpy(pts))
    P = R.Params(seed=31, stages=R.SET1)
    R.check(pts, [0, 3000], [0], P, s.numpy(), np.zeros(3000, bool), np.zeros(3000, bool))
    j = aug.JitterPoints(sigma=0.1, clip=0.2)(pts)
    assert np.abs(j.numpy() - pts).max() <= 0.2 + 2.0 ** -24 * 200


def test_batcher_feeds_the_quantiser_and_a_train_step(aug):
    import egonn_amd
    from egonn_amd import _lib
    from egonn_amd.train import TrainStep
    from tests import helpers as H
    dev = _lib.require_gpu()
    sizes = [6000, 5000, 7000]
    pts, off = R.batch(55, sizes)
    pts = (pts * np.float32(0.25)).astype(np.float32)
    d_pts = torch.from_numpy(pts).to(dev)
    q = egonn_amd.CartesianQuantizer(0.3)
    batcher = egonn_amd.TrainBatcher(q, aug_mode=1, seed=3)
    batch = batcher(d_pts, off.tolist(), [10, 11, 12], draw=2, set_id=7)
    res = batcher.augment(d_pts, off.tolist(), [10, 11, 12], draw=2, set_id=7, record=True)
    # the coords are the quantiser applied to the device's own augmented points, bit for bit
    q2 = egonn_amd.CartesianQuantizer(0.3)
    want = []
    for b in range(3):
        c, _ = q2(res.points[off[b]:off[b + 1]])
        want.append(torch.cat([torch.full((len(c), 1), b, dtype=torch.int32, device=c.device), c], dim=1))
    assert torch.equal(batch["coords"], torch.cat(want)) and batch["batch_size"] == 3
    assert batch["features"].shape == (len(batch["coords"]), 1)
    P = R.Params(seed=3, draw=2, set_id=7, stages=R.MODE1 | R.SET1)
    fl = res.flags.cpu().numpy()
    shares = R.check(pts, off, [10, 11, 12], P, res.points.cpu().numpy(), (fl & 1) > 0, (fl & 2) > 0)
    assert max(shares) <= 0.001, shares
    # one training step on the augmented batch runs and is deterministic
    pos = torch.zeros((3, 3), dtype=torch.bool)
    pos[0, 1] = pos[1, 0] = True
    neg = torch.zeros((3, 3), dtype=torch.bool)
    neg[0, 2] = neg[2, 0] = neg[1, 2] = neg[2, 1] = True
    runs = []
    for _ in range(2):
        mp_ = egonn_amd.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.3)
        model = egonn_amd.model_factory(mp_)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in H.seeded_weights(5).items()})
        model = model.to(dev)
        step = TrainStep(model, torch.optim.SGD(model.parameters(), lr=0.0), margin=0.2)
        b2 = batcher(d_pts, off.tolist(), [10, 11, 12], draw=2, set_id=7)
        loss, _ = step(b2, pos, neg, step_optimizer=False)
        runs.append((float(loss), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}))
    assert np.isfinite(runs[0][0]) and runs[0][0] == runs[1][0]
    for k, g in runs[0][1].items():
        assert torch.equal(g, runs[1][1][k]), k
    # the 6-DoF batch: T_gt = m @ transform of the recorded draw
    T_rel = torch.eye(4).repeat(3, 1, 1)
    T_rel[:, 0, 3] = torch.tensor([1.0, 2.0, 3.0])
    lb = egonn_amd.TrainBatcher(q, aug_mode=None, seed=3, rot_max=np.pi, trans_max=5.0)
    loc = lb.local(d_pts, off, d_pts, off, [10, 11, 12], T_rel, draw=1)
    P = R.Params(seed=3, draw=1, stages=R.RIGID, rot_max=np.pi, trans_max=5.0)
    r32 = R.augment(pts, off, [10, 11, 12], P, np.float32, T_in=T_rel.numpy())
    assert np.array_equal(loc["T_gt"].cpu().numpy(), r32["T_out"])
    assert set(loc) >= {"anc_batch", "pos_batch", "anc_pcd", "pos_pcd", "T_gt"}
    assert loc["pos_batch"]["coords"].shape[1] == 4 and torch.equal(loc["anc_pcd"], d_pts)
