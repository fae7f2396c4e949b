"""GPU tests of the one-call MinkFPN path (egonn_minkfpn_forward through GlobalExtractor), of egonn_topdown_step on its own and
of the rotation sweep.  Inputs are the committed MinkLoc fixtures; the points handed to the voxeliser are the voxel centres
(coords + 0.5) * 0.3 in float32, which floor back to the fixture coordinates exactly.

Bars: the fixtures' own (tests/test_gpu_parity.py::test_minkloc_forward_matches_reference_graph: cosine error < 1e-4,
allclose(rtol=1e-3, atol=1e-4)); split arithmetic within 3e-6 x max |value| of the exact kernels (the header's contract);
everything the project promises to be reproducible (capacities, batch composition, eager vs replay) bit for bit."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu
STEP = 0.3
SPLIT_BOUND = 3e-6


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


@pytest.fixture(autouse=True)
def _collect_contexts():
    """A test that catches a library error leaves its frame — and the contexts in it — in a reference cycle (the exception's
    traceback), and a context freed by a later garbage collection synchronises the device and frees memory wherever that
    collection happens to run, for instance inside another module's stream capture.  Collect them here, where it is harmless."""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()


def _np(t):
    return t.detach().cpu().numpy()


def _case_model(gpu, name):
    case = H.load_case(name)
    if str(case["model"]) == "MinkLoc3D":
        mp = gpu.ModelParams(model="MinkLoc3D", coordinates="cartesian", quantization_step=STEP)
    else:
        mp = gpu.ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=STEP, block=str(case["block"]),
                             pooling=str(case["pooling"]) if "pooling" in case else "GeM")
    m = gpu.model_factory(mp)
    w = H.seeded_weights(case["weight_seed"], name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return case, m.to("cuda").eval()


def _centres(c3):
    """voxel centres of integer coordinates (n, 3): float32 points that quantise back to them"""
    return ((np.asarray(c3).astype(np.float32) + np.float32(0.5)) * np.float32(STEP)).astype(np.float32)


def _scans(c4):
    c4 = np.asarray(c4)
    return [torch.from_numpy(_centres(c4[c4[:, 0] == b][:, 1:])) for b in range(int(c4[:, 0].max()) + 1)]


def _pack(scans):
    off = [0]
    for s in scans:
        off.append(off[-1] + len(s))
    return torch.cat([s for s in scans], dim=0).cuda().contiguous(), off


def _map_rows(ctx, level, fmap):
    """(coords (n, 4), the n valid rows of a capacity-sized map) of `level`"""
    n = ctx.level_count(level)
    return _np(ctx.level_coords(level)), _np(fmap[:n])


@pytest.fixture(scope="module")
def m3d(gpu):
    """MinkLoc3D with the fixture's weights + two different batches cut from the fixture coordinates"""
    case, m = _case_model(gpu, "minkloc3d_cart03_b2")
    s0, s1 = _scans(case["coords"])
    batch_a = [s0, s1]
    batch_b = [s1[::2].contiguous(), s0[100:].contiguous()]
    return case, m, gpu.GlobalExtractor(m), batch_a, batch_b


# ------------------------------------------------------------------------------------ 1. fixtures
@pytest.mark.parametrize("name", ["minkloc3d_cart03_b2", "minkloc_eca_cart03", "minkloc_mac_cart03", "minkloc_spoc_cart03"])
def test_one_call_forward_matches_reference_graph(gpu, name):
    case, m = _case_model(gpu, name)
    c4 = case["coords"]
    ex = gpu.GlobalExtractor(m)
    out = ex.extract(_scans(c4), want_map=True)
    g = _np(out["global"])
    assert set(out) == {"global", "map"} and g.shape == case["global"].shape
    cerr = H.cosine_err(g, case["global"]).max()
    print(name, "global cosine err", cerr, "max abs dev", np.abs(g - case["global"]).max())
    assert cerr < 1e-4
    np.testing.assert_allclose(g, case["global"], rtol=1e-3, atol=1e-4)
    # the feature map the pooling reads, joined to the fixture's rows by coordinate
    ctx = m.context()
    assert m.out_level == 2 and out["map"].shape == (ctx.level_capacity(2), 256)
    rows, fmap = _map_rows(ctx, 2, out["map"])
    want = case["backbone_feats"].astype(np.float32)
    new = fmap[H.join_perm(rows, case["backbone_coords"])]
    # the eager per-operator map of the same fixture, in the same test: the yardstick of the new path's deviation
    with torch.no_grad():
        ctx1, feats = m._plan({"coords": torch.from_numpy(c4), "features": torch.ones((len(c4), 1))}, slot=1)
        level, x = m.backbone.run(ctx1, ctx1.gather_input(feats))
    assert level == 2
    old = _np(x)[H.join_perm(_np(ctx1.level_coords(2)), case["backbone_coords"])]
    dev_new, dev_old, top = np.abs(new - want).max(), np.abs(old - want).max(), np.abs(want).max()
    print(name, "map deviation from the fixture: one call", dev_new, "eager", dev_old, "max |fixture|", top,
          "allowance", SPLIT_BOUND * top)
    assert H.cosine_err(new, want).max() < 1e-4
    assert dev_new <= dev_old + SPLIT_BOUND * top


# ------------------------------------------------------------------------------------ 2. the generic loops
def test_generic_configuration_matches_the_eager_forward(gpu):
    """four levels, two blocks on the first, two top-down steps, ECA blocks, GeM: no fixture, the eager model(batch) is the
    yardstick (the path the fixtures pin)"""
    from egonn_amd.synth import seeded_state_dict
    mp = gpu.ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=STEP, block="ECABasicBlock",
                         planes=(32, 64, 64, 128), layers=(2, 1, 1, 1), num_top_down=2, pooling="GeM")
    m = gpu.model_factory(mp)
    assert m.minkfpn_spec() == ((32, 64, 64, 128), (2, 1, 1, 1), 2, 256, 1, 1)
    sd = seeded_state_dict(311, {k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to("cuda").eval()
    c4 = H.load_case("minkloc_se_cart03")["coords"]
    want = _np(m({"coords": torch.from_numpy(c4), "features": torch.ones((len(c4), 1))})["global"])
    out = gpu.GlobalExtractor(m).extract(_scans(c4), want_map=True)
    g = _np(out["global"])
    cerr = H.cosine_err(g, want).max()
    print("generic configuration: global cosine err", cerr, "max abs dev", np.abs(g - want).max())
    assert g.shape == want.shape == (2, 256) and np.isfinite(g).all() and np.abs(want).max() > 0
    assert cerr < 1e-4
    np.testing.assert_allclose(g, want, rtol=1e-3, atol=1e-4)
    assert out["map"].shape[0] == m.context().level_capacity(2)
    # and on the fp16 matrix pipe for the top-down steps: the same bars
    m.split_topdown = True
    try:
        gs = _np(gpu.GlobalExtractor(m).extract(_scans(c4))["global"])
    finally:
        m.split_topdown = False
    print("generic configuration, split top-down: global cosine err", H.cosine_err(gs, want).max())
    assert H.cosine_err(gs, want).max() < 1e-4
    np.testing.assert_allclose(gs, want, rtol=1e-3, atol=1e-4)


# ------------------------------------------------------------------------------------ 3. plans and replay
def _counts(ex, batch):
    pts, off = _pack(batch)
    return [c - 1024 for c in ex.calibrate(pts, off, margin=1.0)]


def _reserved_eager(ex, batch, caps, slot, max_points=4096):
    """one eager run on a reserved plan: (context, {'global', 'map'}); the caller reads the status"""
    m = ex.model
    ctx = m.context(slot)
    m._sync_weights()
    pts, off = _pack(batch)
    ctx.reserve(max_points, len(batch), caps)
    buf = torch.zeros((max_points, 3), dtype=torch.float32, device="cuda")
    buf[:len(pts)] = pts
    q = ex.quantizer
    ctx.voxelize_device(buf, torch.tensor(off, dtype=torch.int64, device="cuda"), len(batch), q.mode, q.step)
    out = ex._forward(ctx, ex._outputs(ctx, len(batch), True))
    torch.cuda.synchronize()
    return ctx, out


def test_result_does_not_depend_on_the_capacities(m3d):
    _, m, ex, batch_a, _ = m3d
    want = ex.extract(batch_a, want_map=True)
    n2 = m.context().level_count(2)
    counts = _counts(ex, batch_a)
    assert counts[2] == n2
    for slot, caps in ((2, [2 * c + 512 for c in counts]), (3, counts)):       # ample, and exactly the row counts
        ctx, out = _reserved_eager(ex, batch_a, caps, slot)
        ctx.plan_status()
        assert ctx.level_capacity(2) == caps[2] and ctx.level_count(2) == n2
        assert torch.equal(out["global"], want["global"]), slot
        assert torch.equal(out["map"][:n2], want["map"][:n2]), slot


def test_replay_on_another_batch_equals_the_eager_reserved_run(m3d):
    _, m, ex, batch_a, batch_b = m3d
    caps = [2 * c + 512 for c in _counts(ex, batch_a)]
    gx = ex.graph(batch_size=2, max_points=4096, level_capacity=caps, slot=4, want_map=True)
    gx.run(*_pack(batch_a))                               # eager once, captured, replayed on A
    gx.status()
    out = gx.run(*_pack(batch_b))                         # replay on B
    gx.status()
    ctx, want = _reserved_eager(ex, batch_b, caps, slot=5)
    ctx.plan_status()
    n2 = ctx.level_count(2)
    assert n2 == gx.ctx.level_count(2) and 0 < n2 < caps[2]
    assert torch.equal(out["global"], want["global"])
    assert torch.equal(out["map"][:n2], want["map"][:n2])
    assert not torch.equal(out["global"], ex.extract(batch_a)["global"])


def test_each_scan_alone_equals_its_row_in_the_batch(m3d):
    _, m, ex, batch_a, batch_b = m3d
    for batch in (batch_a, batch_b):
        g = ex.extract(batch)["global"].clone()
        for b, scan in enumerate(batch):
            assert torch.equal(ex.extract([scan])["global"][0], g[b]), b


def test_empty_and_single_voxel_scans(m3d):
    case, m, ex, batch_a, _ = m3d
    s0, s1 = batch_a
    one = s1[7:8].contiguous()
    g2 = ex.extract(batch_a)["global"].clone()
    out = ex.extract([s0, torch.zeros((0, 3)), s1, one])          # plan_status inside: status 0
    g4 = out["global"]
    assert g4.shape == (4, 256)
    assert torch.equal(g4[0], g2[0]) and torch.equal(g4[2], g2[1])
    # the degenerate rows: what the eager path returns for them (the fixtures' bars: the two paths differ in the first layer's kernel)
    c4 = case["coords"]
    cone = c4[c4[:, 0] == 1][7:8].copy()
    ca, cb = c4[c4[:, 0] == 0].copy(), c4[c4[:, 0] == 1].copy()
    cb[:, 0], cone[:, 0] = 2, 3
    cc = np.concatenate([ca, cb, cone])
    eager = m({"coords": torch.from_numpy(cc), "features": torch.ones((len(cc), 1)), "batch_size": 4})["global"]
    print("empty scan row", _np(g4[1])[:4], "eager", _np(eager[1])[:4], "| single voxel", _np(g4[3])[:4], "eager", _np(eager[3])[:4])
    for b in (1, 3):
        assert torch.allclose(g4[b], eager[b], rtol=1e-3, atol=1e-4, equal_nan=True), b
    assert H.cosine_err(_np(g4[[0, 2]]), _np(eager[[0, 2]])).max() < 1e-4


def test_level_overflow_is_clipped_and_reported(gpu, m3d):
    """the clipping contract of a reserved plan: a level-2 capacity below the row count is reported by plan_status, nothing
    faults, and the next fitting batch on the same context is bitwise the exact-plan result"""
    _, m, ex, batch_a, _ = m3d
    small = [s[s[:, 0] < s[:, 0].median()].contiguous() for s in batch_a]      # half of every scene: about half the rows per level
    counts, small_counts = _counts(ex, batch_a), _counts(ex, small)
    caps = [2 * c + 512 for c in counts]
    caps[2] = max(int(0.6 * counts[2]), small_counts[2] + 8)
    assert small_counts[2] < caps[2] < counts[2]
    ctx, _ = _reserved_eager(ex, batch_a, caps, slot=6)
    with pytest.raises(gpu._lib.CapacityError):
        ctx.plan_status()
    ctx, out = _reserved_eager(ex, small, caps, slot=6)
    ctx.plan_status()
    assert torch.equal(out["global"], ex.extract(small)["global"])


# ------------------------------------------------------------------------------------ 4. the top-down step on its own
def _children(ctx, level_out):
    """children per parent of the rows of level_out"""
    c = _np(ctx.level_coords(level_out)).astype(np.int64)
    parent = np.concatenate([c[:, :1], np.floor_divide(c[:, 1:], 2 ** (level_out + 1))], axis=1)
    return np.unique(parent, axis=0, return_counts=True)[1]


def _planted(name, level_out):
    """The fixture coordinates plus a planted parent far from the scene, so that every case has what the kernel's row handling
    can go wrong on: levels (3, 2) of minkloc3d_cart03_b2 have no parent with more than six children (measured: 26 / 72 / 21 /
    58 / 1 / 2 parents with 1..6), so one parent with all eight is added (a voxel in every octant of an aligned block); level 2
    of minkloc_eca_cart03 has 368 = 23 x 16 rows, so one single-voxel parent is added and neither row count is a multiple of 16."""
    c4 = H.load_case(name)["coords"]
    s = 2 ** level_out                       # edge of a level_out cell in voxels; the parent block is 2 s wide
    if name == "minkloc3d_cart03_b2":
        extra = [[0, 400 + s * i, 400 + s * j, s * k] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    else:
        extra = [[0, 400, 400, 0]]
    assert 400 % (2 * s) == 0 and np.abs(c4[:, 1:]).max() < 300
    return np.concatenate([c4, np.asarray(extra, dtype=c4.dtype)])


@pytest.mark.parametrize("name,level_out,C,Cl", [("minkloc3d_cart03_b2", 2, 256, 64), ("minkloc3d_cart03_b2", 2, 256, 256),
                                                  ("minkloc_eca_cart03", 1, 128, 128), ("minkloc_eca_cart03", 1, 64, 32)])
def test_topdown_step(gpu, name, level_out, C, Cl):
    c4 = _planted(name, level_out)
    B = int(c4[:, 0].max()) + 1
    coords = torch.from_numpy(c4).cuda().contiguous()
    ctx = gpu._lib.Context()
    ctx.coords_set(coords, B)
    n_out, n_in = ctx.level_count(level_out), ctx.level_count(level_out + 1)
    kids = _children(ctx, level_out)
    print(name, "rows", n_out, "parents", n_in, "children per parent", np.bincount(kids))
    assert len(kids) == n_in and kids.sum() == n_out and n_out % 16 != 0 and n_in % 16 != 0
    assert (kids == 1).any() and (kids == 8).any()
    g = torch.Generator().manual_seed(C + Cl + level_out)
    xc = torch.randn((n_in, C), generator=g).cuda()
    xl = torch.randn((n_out, Cl), generator=g).cuda()
    wt = (torch.randn((8, C, C), generator=g) / C ** 0.5).cuda()
    wl = (torch.randn((Cl, C), generator=g) / Cl ** 0.5).cuda()

    def both(lat):
        a = (xl, wl) if lat else (None, None)
        ctx.set_exact_fp32(False)
        split = ctx.topdown_step(level_out, xc, wt, *a)
        again = ctx.topdown_step(level_out, xc, wt, *a)
        ctx.plan_status()                                  # no range flag
        ctx.set_exact_fp32(True)
        exact = ctx.topdown_step(level_out, xc, wt, *a)
        ref = ctx.conv_transpose(level_out + 1, xc, wt)
        if lat:
            ref = ctx.add(ref, ctx.conv(level_out, level_out, 1, xl, wl))
        ctx.set_exact_fp32(False)
        return split, again, exact, ref

    for lat in (True, False):
        split, again, exact, ref = both(lat)
        assert split.shape == (n_out, C) and torch.equal(exact, ref), lat
        assert torch.equal(split, again), lat
        err, top = float((split - exact).abs().max()), float(exact.abs().max())
        print(name, C, Cl, "lateral" if lat else "no lateral", "max |split - exact|", err, "bound", SPLIT_BOUND * top)
        assert top > 1 and err <= SPLIT_BOUND * top, lat
    split = both(True)[0]

    # a reserved plan with room to spare: the same valid rows (buffers padded to the capacities)
    pts, off = _pack(_scans(c4))
    caps = [2 * ctx.level_count(l) + 64 for l in range(8)]
    ctx2 = gpu._lib.Context()
    ctx2.reserve(len(pts) + 100, B, caps)
    buf = torch.zeros((len(pts) + 100, 3), dtype=torch.float32, device="cuda")
    buf[:len(pts)] = pts
    ctx2.voxelize_device(buf, torch.tensor(off, dtype=torch.int64, device="cuda"), B, 0, [STEP])
    pad = lambda x, n: torch.cat([x, torch.zeros((n - len(x), x.shape[1]), device="cuda")])      # noqa: E731
    got = ctx2.topdown_step(level_out, pad(xc, caps[level_out + 1]), wt, pad(xl, caps[level_out]), wl, rows=caps[level_out])
    torch.cuda.synchronize()
    ctx2.plan_status()
    assert ctx2.level_count(level_out) == n_out and torch.equal(ctx2.level_coords(level_out), ctx.level_coords(level_out))
    assert torch.equal(got[:n_out], split)

    # one operand beyond the fp16 range: reported in split mode, fine on the exact kernels (last: the flag stays with the plan)
    xbig = xc.clone()
    xbig[n_in // 2, 5] = 7e4
    ctx.topdown_step(level_out, xbig, wt, xl, wl)
    with pytest.raises(gpu._lib.Fp16RangeError):
        ctx.plan_status()
    ctx.coords_set(coords, B)                              # a plan builder clears the flag
    ctx.set_exact_fp32(True)
    big = ctx.topdown_step(level_out, xbig, wt, xl, wl)
    ctx.plan_status()
    assert torch.isfinite(big).all()


# ------------------------------------------------------------------------------------ 5. the rotation sweep
def test_rotation_sweep(gpu, m3d):
    from egonn_amd import augment
    from egonn_amd.retrieval import recall_at_k
    from egonn_amd.synth import lidar_scan
    _, m, ex, _, _ = m3d
    maps = [torch.from_numpy(lidar_scan(900 + i, n_points=3000)) for i in range(4)]
    queries = [s[torch.arange(len(s)) % 10 != 3].contiguous() for s in maps]      # the same places, a tenth of the returns missing
    map_pos = np.array([[100.0 * i, 0.0] for i in range(4)])
    query_pos = map_pos + 1.0
    radius, seed = [5.0, 20.0], 5
    res = gpu.evaluate_with_rotations(ex, maps, queries, map_pos, query_pos, radius, k=4, rotations=[0.0, 90.0], seed=seed,
                                      batch_size=3)
    assert list(res.keys()) == [0.0, 90.0]
    map_emb = ex.extract(maps)["global"].clone()
    plain = ex.extract(queries)["global"].clone()
    # bound 0: the angle is exactly 0
    assert torch.equal(res[0.0]["embeddings"], plain)
    want = recall_at_k(map_emb, plain, map_pos, query_pos, radius, k=4)["recall"]
    assert res[0.0]["recall"] == want and set(want) == set(radius)
    print("recall at bound 0", want, "| at bound 90", res[90.0]["recall"])
    assert want[5.0][0] == 1.0 and want[20.0][-1] == 1.0
    # bound 90: the ROTATE stage by hand with the same keys (seed, index of the bound, query index)
    pts, off = _pack(queries)
    rot = augment.augment_points(pts, torch.tensor(off, dtype=torch.int64, device="cuda"),
                                 torch.arange(4, dtype=torch.int32, device="cuda"),
                                 augment.AugmentParams(seed=seed, stages=augment.ROTATE, max_theta=90.0), draw=1, set_id=0).points
    assert not torch.equal(rot, pts) and torch.allclose(rot.norm(dim=1), pts.norm(dim=1), rtol=1e-5, atol=1e-4)
    by_hand = ex.extract_checked(rot, off)["global"]
    assert torch.equal(res[90.0]["embeddings"], by_hand)
    assert not torch.equal(by_hand, plain)
    assert res[90.0]["recall"] == recall_at_k(map_emb, by_hand, map_pos, query_pos, radius, k=4)["recall"]
