"""GPU tests of the batched local-head loss (`egonn_local_loss`, `local_loss_packed`, `BatchedKeypointCorrLoss`) and of the full
two-phase step `EgoNNTrainStep`.  Oracles: the float64 arrays of tests/golden/local_losses.npz (real outputs of the reference's
classes) for the fixture batch, tests/local_loss_ref.py (pinned to that fixture by tests/test_local_loss_batch_host.py) for the
edge batches.  Bounds: the ones tests/test_gpu_losses.py holds the per-pair driver to — loss rel 5e-6, metrics rel 2e-4 / abs
2e-5, gradients 1e-4 of the tensor's max-abs (+1e-7), the gradients of a P-pair batch scaled by 1/P."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import local_loss_ref as R

pytestmark = pytest.mark.gpu
CASES = ("a", "b", "c")
PACK_ORDER = ("clouds1", "cloud_off1", "kp1", "sigma1", "desc1", "kp_off1", "clouds2", "cloud_off2", "kp2", "sigma2", "desc2",
              "kp_off2", "transforms")
GAMMA_ORDER = ("gamma_chamfer", "gamma_p2p", "gamma_c", "gamma_k", "beta", "dist_th")


@pytest.fixture(scope="module")
def fx():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "local_losses.npz"))


@pytest.fixture(scope="module")
def edges(fx):
    """the edge batches and their float64 oracle, computed once"""
    out = {}
    for name, (pairs, expect) in R.edge_batches(H.kernel_constant("LL_CLOUD_CHUNK")).items():
        out[name] = (pairs, expect, R.batch_f64(pairs))
    return out


def _fixture_pairs(fx, names=CASES):
    return [{k: fx[f"{n}_{k}"] for k in ("pc1", "pc2", "kp1", "kp2", "sigma1", "sigma2", "desc1", "desc2", "M")} for n in names]


def _run_packed(pairs, gammas=R.GAMMAS):
    """-> (loss, stats, pair_stats, {key: packed grad}, packed inputs)"""
    from egonn_amd import local_loss as L
    t = {k: torch.from_numpy(v).cuda() for k, v in R.pack(pairs).items()}
    for k in R.GRAD_KEYS:
        t[k].requires_grad_(True)
    loss, stats, ps = L.local_loss_packed(*[t[k] for k in PACK_ORDER], [gammas[k] for k in GAMMA_ORDER], return_pair_stats=True)
    loss.backward()
    return loss, stats, ps, {k: t[k].grad for k in R.GRAD_KEYS}, t


def _split(packed, pairs, key):
    n = np.cumsum([0] + [len(p[key]) for p in pairs])
    return [packed[n[i]:n[i + 1]] for i in range(len(pairs))]


def _close_grad(got, want, what, rel=1e-4):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "nan pattern")
    if np.isnan(want).all():
        return
    err, scale = float(np.nanmax(np.abs(got - want))), float(np.nanmax(np.abs(want)))
    print(what, "grad err / max-abs", err / max(scale, 1e-300))
    assert err <= rel * scale + 1e-7, (what, err, scale)


def _check_against(pairs, want_pair_stats, want_grads, loss, stats, ps, grads, tag):
    """want_pair_stats: [ {key: float64} ] per pair; want_grads: [ {key: array already divided by the pairs} ]"""
    P = len(pairs)
    ps = ps.cpu().numpy().astype(np.float64)
    for i in range(P):
        for c, k in enumerate(R.STAT_KEYS):
            want, got = float(want_pair_stats[i][k]), ps[i, c]
            if np.isnan(want):
                assert np.isnan(got), (tag, i, k)
            elif k == "loss":
                assert got == pytest.approx(want, rel=5e-6), (tag, i, k)
            else:
                assert got == pytest.approx(want, rel=2e-4, abs=2e-5), (tag, i, k, got, want)
    assert ps[:, 14:].tolist() == [[0.0, 0.0]] * P
    st = stats.cpu().numpy().astype(np.float64)
    for c, k in enumerate(R.STAT_KEYS):
        want = np.mean([float(s[k]) for s in want_pair_stats])
        if np.isnan(want):
            assert np.isnan(st[c]), (tag, k)
        else:
            assert st[c] == pytest.approx(want, rel=5e-6 if k == "loss" else 2e-4, abs=0 if k == "loss" else 2e-5), (tag, k)
    assert float(loss.detach()) == st[0] or (np.isnan(float(loss.detach())) and np.isnan(st[0]))
    for k in R.GRAD_KEYS:
        for i, g in enumerate(_split(grads[k], pairs, k)):
            _close_grad(g, want_grads[i][k], (tag, i, k))


def test_fixture_batch_matches_float64_reference(fx):
    """cases a, b, c of the reference fixture as ONE 3-pair batch: per-pair rows, batch means and gradients / 3"""
    pairs = _fixture_pairs(fx)
    loss, stats, ps, grads, _ = _run_packed(pairs, dict(zip(GAMMA_ORDER, fx["gammas"].tolist())))
    want_stats = []
    for n, p in zip(CASES, pairs):
        s = {k: float(fx[f"{n}_f64_metric_{k}"]) for k in R.STAT_KEYS[2:]}
        s.update(loss=float(fx[f"{n}_f64_loss_total"]), kp_per_cloud=0.5 * (len(p["kp1"]) + len(p["kp2"])))
        want_stats.append(s)
    want_grads = [{k: fx[f"{n}_f64_grad_{k}"].astype(np.float64) / 3.0 for k in R.GRAD_KEYS} for n in CASES]
    _check_against(pairs, want_stats, want_grads, loss, stats, ps, grads, "fixture")
    assert float(loss) == pytest.approx(np.mean([float(fx[f"{n}_f64_loss_total"]) for n in CASES]), rel=5e-6)


@pytest.mark.parametrize("name", ["three", "eight", "one"])
def test_edge_batches_match_float64_restatement(edges, name):
    """uneven keypoint counts around the 32 / 64-row tiles, clouds on each side of LL_CLOUD_CHUNK with the nearest point planted
    at index 0, at the last index and on both sides of every chunk boundary, exact duplicates (lowest index wins), a keypoint
    exactly on a cloud point (zero gradient), a pair without correspondences (NaN placement), shared classes; 1, 3 and 8 pairs"""
    pairs, expect, ref = edges[name]
    loss, stats, ps, grads, _ = _run_packed(pairs)
    _check_against(pairs, ref["pair_stats"], ref["grads"], loss, stats, ps, grads, name)
    if "zero_p2p" in expect:
        pi, side, k = expect["zero_p2p"]
        assert ref["pairs"][pi]["i" + side][k] >= 0
    if "nan_pair" in expect:
        i = expect["nan_pair"]
        for k in R.GRAD_KEYS:
            for j, g in enumerate(_split(grads[k], pairs, k)):
                assert bool(torch.isnan(g).all()) == (j == i and k in ("desc1", "desc2")), (k, j)
                assert bool(torch.isnan(g).any()) == (j == i and k in ("desc1", "desc2")), (k, j)


def _run_lists(loss_fn, pairs):
    ts = [{k: torch.from_numpy(v).cuda() for k, v in p.items()} for p in pairs]
    for t in ts:
        for k in R.GRAD_KEYS:
            t[k].requires_grad_(True)
    loss, metrics = loss_fn(torch.cat([t["pc1"] for t in ts]), [t["kp1"] for t in ts], [t["sigma1"] for t in ts],
                            [t["desc1"] for t in ts], torch.cat([t["pc2"] for t in ts]), [t["kp2"] for t in ts],
                            [t["sigma2"] for t in ts], [t["desc2"] for t in ts], [t["M"].cpu() for t in ts],
                            [(len(t["pc1"]), len(t["pc2"])) for t in ts])
    loss.backward()
    return loss, metrics, ts


def test_nan_placement_equals_the_per_pair_driver(edges):
    """the isnan pattern over loss, every metric and all six gradients equals KeypointCorrLoss on the same inputs"""
    from egonn_amd import local_loss as L
    pairs, expect, _ = edges["eight"]
    l0, m0, t0 = _run_lists(L.make_local_loss(), pairs)
    l1, m1, t1 = _run_lists(L.make_local_loss(batched=True), pairs)
    assert np.isnan(float(l0)) and np.isnan(float(l1))
    assert set(m0) == set(m1)
    for k in m0:
        assert np.isnan(float(m0[k])) == np.isnan(float(m1[k])), k
    for a, b in zip(t0, t1):
        for k in R.GRAD_KEYS:
            assert torch.equal(torch.isnan(a[k].grad), torch.isnan(b[k].grad)), k


def test_agrees_with_the_per_pair_driver_and_the_packed_call(fx):
    from egonn_amd import local_loss as L
    pairs = _fixture_pairs(fx)
    l0, m0, t0 = _run_lists(L.make_local_loss(), pairs)
    l1, m1, t1 = _run_lists(L.make_local_loss(batched=True), pairs)
    assert l1.is_cuda and l1.dim() == 0 and all(torch.is_tensor(v) and v.is_cuda and v.dim() == 0 for v in m1.values())
    assert set(m0) == set(m1) == set(R.STAT_KEYS)
    assert float(l1) == pytest.approx(float(l0), rel=5e-6)
    for k in m0:
        assert float(m1[k]) == pytest.approx(float(m0[k]), rel=2e-4, abs=2e-5), k
    for a, b in zip(t0, t1):
        for k in R.GRAD_KEYS:
            _close_grad(b[k].grad, a[k].grad.cpu().numpy().astype(np.float64), ("driver", k))
    loss, stats, _, grads, _ = _run_packed(pairs)
    assert torch.equal(loss, l1) and all(torch.equal(stats[i], m1[k]) for i, k in enumerate(R.STAT_KEYS))
    for k in R.GRAD_KEYS:
        assert torch.equal(grads[k], torch.cat([t[k].grad for t in t1])), k


def test_deterministic_and_batch_invariant(fx):
    pairs = _fixture_pairs(fx)
    r0, r1 = _run_packed(pairs), _run_packed(pairs)
    assert torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1]) and torch.equal(r0[2], r1[2])
    for k in R.GRAD_KEYS:
        assert torch.equal(r0[3][k], r1[3][k]), k
    a, b, c = pairs
    alone, four = _run_packed([a]), _run_packed([b, c, a, b])
    assert torch.equal(alone[2][0], four[2][2])
    for k in R.GRAD_KEYS:
        g4 = _split(four[3][k], [b, c, a, b], k)[2]
        assert torch.equal(alone[3][k], g4 * 4.0), k


def test_enqueues_on_a_side_stream_and_replays_in_a_graph(fx):
    """no host synchronisation: the whole call is captured in a torch.cuda.graph and replayed on new values in the same buffers"""
    from egonn_amd import local_loss as L
    a, b, c = _fixture_pairs(fx)
    gam = [R.GAMMAS[k] for k in GAMMA_ORDER]
    t = {k: torch.from_numpy(v).cuda() for k, v in R.pack([a]).items()}
    want_a = _run_packed([a])
    a2 = dict(a)
    a2["kp1"] = a["kp1"] + np.float32(0.01)
    a2["desc2"] = np.ascontiguousarray(a["desc2"][::-1])
    want_a2 = _run_packed([a2])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        loss, stats = L.local_loss_packed(*[t[k] for k in PACK_ORDER], gam)            # warm-up on the side stream
        assert loss.is_cuda and stats.is_cuda
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(loss, want_a[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, stats, ps = L.local_loss_packed(*[t[k] for k in PACK_ORDER], gam, return_pair_stats=True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(stats, want_a[1])
    for k, v in R.pack([a2]).items():
        t[k].copy_(torch.from_numpy(v))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(stats, want_a2[1]) and torch.equal(ps, want_a2[2]) and not torch.equal(stats, want_a[1])


# ----------------------------------------------------------------------------- the full two-phase step
def _step_inputs():
    from egonn_amd import CartesianQuantizer
    from egonn_amd.synth import planted_scan_pair
    q = CartesianQuantizer(0.4)
    prs = [planted_scan_pair(60 + i, 4000) for i in range(2)]

    def batch(clouds):
        cs = [torch.unique(q(torch.from_numpy(c))[0], dim=0) for c in clouds]
        coords = torch.cat([torch.cat([torch.full((len(c), 1), b, dtype=torch.int32), c.int()], 1) for b, c in enumerate(cs)])
        return {"coords": coords, "features": torch.ones((len(coords), 1)), "batch_size": len(cs)}
    g = batch([prs[0][0], prs[0][1], prs[1][0], prs[1][1]])
    pos = torch.zeros((4, 4), dtype=torch.bool)
    pos[0, 1] = pos[1, 0] = pos[2, 3] = pos[3, 2] = True
    neg = ~(pos | torch.eye(4, dtype=torch.bool))
    local = {"anc_batch": batch([p[0] for p in prs]), "pos_batch": batch([p[1] for p in prs]),
             "anc_pcd": torch.cat([torch.from_numpy(p[0]) for p in prs]).float(),
             "pos_pcd": torch.cat([torch.from_numpy(p[1]) for p in prs]).float(),
             "T_gt": torch.stack([torch.from_numpy(np.asarray(p[2])).float() for p in prs]),
             "len_batch": [[len(p[0]), len(p[1])] for p in prs]}
    return g, pos, neg, local


# the keypoints of a seeded, untrained model sit on a 3.2 m supervoxel grid: a wide dist_th keeps most rows in the correspondence term
LOCAL = dict(beta=2.0, dist_th=2.0)


def _model(seed=5):
    from egonn_amd import ModelParams, model_factory
    from egonn_amd.synth import seeded_state_dict
    model = model_factory(ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.4))
    sd = seeded_state_dict(seed, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to("cuda:0")


def test_full_step_accumulates_both_phases_and_steps_once(fx):
    """EgoNNTrainStep = the global phase of TrainStep + two forwards + the batched local loss + ONE optimizer step: with SGD(lr=0)
    every parameter gradient equals the one assembled by hand on the per-pair driver (1e-4 of the tensor's max-abs), two runs
    agree bitwise, and with lr > 0 the parameters move by exactly one step"""
    from egonn_amd import local_loss as L
    from egonn_amd.train import EgoNNTrainStep, TrainStep
    g, pos, neg, local = _step_inputs()

    def run(batched):
        model = _model()
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        if batched:
            gl, ll, stats = EgoNNTrainStep(model, opt, local_loss_fn=L.BatchedKeypointCorrLoss(**LOCAL))(g, pos, neg, local)
            assert gl.is_cuda and ll.is_cuda and stats["loss"].is_cuda and "correspondence_loss" in stats
        else:
            TrainStep(model, opt)(g, pos, neg, step_optimizer=False)
            y1 = model(local["anc_batch"], context_slot=1)
            y2 = model(local["pos_batch"], context_slot=2)
            ll, _ = L.KeypointCorrLoss(**LOCAL)(local["anc_pcd"].cuda(), y1["keypoints"], y1["sigma"], y1["descriptors"],
                                        local["pos_pcd"].cuda(), y2["keypoints"], y2["sigma"], y2["descriptors"],
                                        local["T_gt"], local["len_batch"])
            ll.backward()
        return float(ll), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    l_hand, g_hand = run(False)
    l_a, g_a = run(True)
    l_b, g_b = run(True)
    assert np.isfinite(l_a) and l_a == l_b and l_a == pytest.approx(l_hand, rel=5e-6)
    assert set(g_a) == set(g_hand) == set(g_b) and len(g_a) > 50
    worst = 0.0
    for n in g_a:
        assert torch.equal(g_a[n], g_b[n]), n
        err, scale = float((g_a[n] - g_hand[n]).abs().max()), float(g_hand[n].abs().max())
        worst = max(worst, err / max(scale, 1e-30))
        assert err <= 1e-4 * scale + 1e-7, (n, err, scale)
    print("full step: worst gradient error / max-abs", worst)
    # lr > 0: exactly one step, p_new = p_old - lr * (global + local gradient)
    model = _model()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    EgoNNTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.5), local_loss_fn=L.BatchedKeypointCorrLoss(**LOCAL))(g, pos, neg, local)
    for n, p in model.named_parameters():
        if n in g_a:
            assert torch.equal(p.detach(), before[n] - 0.5 * g_a[n]), n
