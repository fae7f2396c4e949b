"""GPU tests of train-mode pooling (run with -m gpu on an MI355X): NetVLAD / NetVLAD-GC forward + backward
(egonn_netvlad_train_forward / _backward under egonn_amd.train.NetVLADFn) against the reference's float64 operator fixture and,
at product channel counts, against the host-validated float64 restatement of tests/test_netvlad_train_host.py; MAC / SPoC
gradients; MinkLoc end to end against the reference graph's train-step fixtures; MinkGL with MAC / SPoC; TrainStep."""
import zlib

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_netvlad import ROWS, _batch, _scan_coords
from tests.test_netvlad_train_host import E2E_CASES, PARAM_KEYS, grad_scale, load_op_fixture, op_state, run_f64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


def _np(t):
    return t.detach().cpu().numpy()


def _module(state, c, d, gating):
    from egonn_amd.model import NetVLADLoupe
    nv = NetVLADLoupe(c, 64, d, gating=gating)
    missing = nv.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    assert all(k.endswith("num_batches_tracked") for k in missing.missing_keys) and not missing.unexpected_keys
    return nv.cuda().train()


def _step(gpu, nv, coords, feats, upstream, order=None):
    """NetVLAD train step on a level-0 plan of the given scans (scan b gets batch index order[b]).  Returns, with the scans in
    LIST order: y (B, D), grad x per input row, parameter gradients, running buffers."""
    from egonn_amd import train
    B = len(coords)
    order = list(range(B)) if order is None else [int(o) for o in order]
    ctx = gpu._lib.Context(torch.device("cuda", 0))
    c4 = np.concatenate([np.c_[np.full(len(c), order[b], np.int32), c] for b, c in enumerate(coords)])
    ctx.coords_set(torch.from_numpy(c4).cuda(), B)
    idx = ctx.input_index()                                        # plan row i holds input row idx[i]
    x = ctx.gather_input(torch.from_numpy(np.concatenate(feats)).cuda()).requires_grad_(True)
    nv.zero_grad(set_to_none=True)
    y = train.netvlad_pool(ctx, 0, x, nv)
    up = torch.empty_like(y)
    up[torch.tensor(order, device="cuda")] = torch.from_numpy(np.asarray(upstream, dtype=np.float32)).cuda()
    (y * up).sum().backward()
    gx = torch.empty_like(x)
    gx[idx] = x.grad
    grads = {k: p.grad.detach().clone() for k, p in nv.named_parameters()}
    bufs = {k: v.detach().clone() for k, v in nv.state_dict().items() if "running" in k or "num_batches" in k}
    return y.detach()[torch.tensor(order, device="cuda")], gx, grads, bufs


def _check_against(got, want, fx=None, variant=None):
    """the gates of tests/test_gpu_train.py for a differentiable operator against float64: outputs rtol 1e-4 / atol 1e-5,
    gradients rtol 1e-3 / atol 1e-4 * max|ref| (max|ref| of an analytically zero gradient: grad_scale), buffers rtol 1e-5 /
    atol 1e-6"""
    y, gx, grads, bufs = got
    wy, wgx, wg, wb = want
    np.testing.assert_allclose(_np(y), wy, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(_np(gx), wgx, rtol=1e-3, atol=1e-4 * float(np.abs(wgx).max()))
    assert set(grads) == set(wg)
    for k, ref in wg.items():
        scale = grad_scale(fx, variant, k) if fx is not None else float(np.abs(ref).max())
        assert np.isfinite(_np(grads[k])).all(), k
        np.testing.assert_allclose(_np(grads[k]).reshape(ref.shape), ref, rtol=1e-3, atol=1e-4 * scale, err_msg=k)
    for k, ref in wb.items():
        np.testing.assert_allclose(_np(bufs[k]), ref, rtol=1e-5, atol=1e-6, err_msg=k)


# ------------------------------------------------------------------ 1. operator vs the reference's float64 fixture
@pytest.mark.parametrize("variant", ["c16", "c64", "c16_alone", "c64_alone"])
def test_netvlad_train_operator_matches_reference_fixture(gpu, variant):
    fx = load_op_fixture()
    case = fx[variant]
    c, d, gating = int(case["C"]), int(case["D"]), bool(case["gating"])
    off = case["offsets"]
    rng = np.random.default_rng(5)
    coords = [_scan_coords(rng, int(n)) for n in np.diff(off)]
    if variant.endswith("_alone"):
        # the scan repeated: the same voxels under every batch index, hence the same plan row order and (batch invariance)
        # bitwise equal descriptors, as in exact arithmetic; bn2 divides their spread by sqrt(eps), so descriptors that
        # differed by fp32 rounding of another row order would show up 316-fold in the output
        coords = [coords[0]] * len(coords)
    feats = [case["x"][off[b]:off[b + 1]] for b in range(len(off) - 1)]
    nv = _module(op_state(case), c, d, gating)
    got = _step(gpu, nv, coords, feats, case["upstream"])
    keys = [k for k in PARAM_KEYS if gating or "gating" not in k]
    want = (case["out"], case["grad_x"], {k: case["grad/" + k] for k in keys},
            {k[4:]: case[k] for k in case if k.startswith("buf/")})
    _check_against(got, want, fx, variant)
    assert int(got[3]["bn1.num_batches_tracked"]) == int(got[3]["bn2.num_batches_tracked"]) == 1


# ------------------------------------------------------------------ 2. product channel counts, determinism, batch order
@pytest.mark.parametrize("c,d,gating", [(256, 256, True), (256, 128, False)])
def test_netvlad_train_operator_at_product_sizes(gpu, c, d, gating):
    case = {"C": c, "D": d, "gating": int(gating), "seed": 91}
    state = op_state(case)
    coords, feats = _batch(ROWS, 23 + d, c)
    B = len(ROWS)
    upstream = np.random.default_rng(17).standard_normal((B, d)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(ROWS)])
    want = run_f64(np.concatenate(feats), off, state, gating, upstream)
    runs = [_step(gpu, _module(state, c, d, gating), coords, feats, upstream) for _ in range(2)]
    for t in (runs[0][0], runs[0][1], *runs[0][2].values()):
        assert torch.isfinite(t).all()
    _check_against(runs[0], want)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])          # bitwise-equal reruns
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    # the same scans under other batch indices (same Nmax): per-scan grad x bitwise, parameter gradients within the gates
    perm = np.random.default_rng(2).permutation(B)
    other = _step(gpu, _module(state, c, d, gating), coords, feats, upstream, order=perm)
    assert torch.equal(other[1], runs[0][1])
    _check_against(other, want)


# ------------------------------------------------------------------ 3. MAC / SPoC operators
def test_mac_and_spoc_gradients_match_float64(gpu):
    from egonn_amd import train
    rows, c = [1, 0, 300, 65, 129], 64                      # a one-row scan and an empty scan
    rng = np.random.default_rng(8)
    coords = [_scan_coords(rng, n) for n in rows]
    ctx = gpu._lib.Context(torch.device("cuda", 0))
    c4 = np.concatenate([np.c_[np.full(len(cc), b, np.int32), cc] for b, cc in enumerate(coords)])
    ctx.coords_set(torch.from_numpy(c4).cuda(), len(rows))
    off = ctx.level_batch_offsets(0)
    assert list(np.diff(off)) == rows
    xh = rng.standard_normal((sum(rows), c)).astype(np.float32)
    b2, r2 = 2, off[2]
    xh[r2 + 7, 5] = xh[r2 + 200, 5] = 50.0                  # a tied maximum: the lowest plan row takes the gradient
    up = rng.standard_normal((len(rows), c)).astype(np.float32)
    for fn, ref in ((train.GlobalMaxFn, "amax"), (train.SegmentMeanFn, "mean")):
        x = torch.from_numpy(xh).cuda().requires_grad_(True)
        y = fn.apply(x, ctx, 0)
        (y * torch.from_numpy(up).cuda()).sum().backward()
        x64 = torch.from_numpy(xh).double().requires_grad_(True)
        if ref == "amax":
            x64b = x64.clone()
            x64b.data[r2 + 200, 5] -= 1e-9                   # float64 reference with the tie broken towards the lowest row
            x64 = x64b.detach().requires_grad_(True)
        segs = [getattr(x64[off[b]:off[b + 1]], ref)(dim=0) if rows[b] else torch.zeros(c, dtype=torch.float64)
                for b in range(len(rows))]
        y64 = torch.stack(segs)
        (y64 * torch.from_numpy(up).double()).sum().backward()
        np.testing.assert_allclose(_np(y), y64.detach().numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(_np(x.grad), x64.grad.numpy(), rtol=1e-3, atol=1e-4 * float(x64.grad.abs().max()))
        assert float(y.detach()[1].abs().max()) == 0.0               # the empty scan pools to 0 and routes no gradient
        if ref == "amax":
            assert float(x.grad[r2 + 7, 5]) == float(up[b2, 5]) and float(x.grad[r2 + 200, 5]) == 0.0
            assert torch.equal(y, ctx.global_max_pool(0, x.detach()))


# ------------------------------------------------------------------ 4. end to end vs the reference graph's train step
def _digest(name, g):
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    r = np.random.default_rng(zlib.crc32(name.encode())).standard_normal(g.size)
    return np.concatenate([[np.linalg.norm(g), float(g @ r)], g[:64] if g.size > 4096 else g])


def _minkloc(gpu, name):
    case = H.load_case(name)
    mp = gpu.ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=0.3, block=str(case["block"]),
                         pooling=str(case["pooling"]), output_dim=int(case["output_dim"]))
    m = gpu.model_factory(mp)
    w = H.seeded_weights(int(case["weight_seed"]), E2E_CASES[name])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return case, m.to("cuda").train()


@pytest.mark.parametrize("name", list(E2E_CASES))
def test_minkloc_pooling_train_step_matches_reference_fixture(gpu, name):
    """the body and the gates of tests/test_gpu_train.py::test_minkloc_train_step_matches_reference_fixture"""
    case, model = _minkloc(gpu, name)
    coords = torch.from_numpy(case["coords"]).cuda()
    g = model({"coords": coords, "features": torch.ones((len(coords), 1), device="cuda")})["global"]
    cos = H.cosine_err(_np(g), case["global"]).max()
    R = torch.from_numpy(np.random.default_rng(int(case["proj_seed"])).standard_normal(case["global"].shape)
                         .astype(np.float32)).cuda()
    loss = (g * R).sum()
    print(name, "global 1-cos", cos, "loss", loss.item(), "ref", float(case["loss"]))
    assert cos <= 1e-4
    assert abs(loss.item() - float(case["loss"])) <= 2e-3 * max(1.0, abs(float(case["loss"])))
    loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    keys = [k[5:] for k in case if k.startswith("grad/")]
    assert set(keys) == set(grads)
    bad = []
    for k in keys:
        assert grads[k] is not None, k
        mine, ref = _digest(k, _np(grads[k])), case["grad/" + k]
        norm = max(ref[0], 1e-12)
        err = max(abs(mine[0] - ref[0]) / norm, abs(mine[1] - ref[1]) / norm,
                  float(np.abs(mine[2:] - ref[2:]).max()) / max(float(np.abs(ref[2:]).max()), 1e-12))
        print(f"  {k}: digest error {err:.3e}")
        if err > 5e-3:
            bad.append((k, err))
    assert not bad, bad
    sd = model.state_dict()
    for k in [k[4:] for k in case if k.startswith("buf/")]:
        assert np.allclose(_np(sd[k]), case["buf/" + k], rtol=1e-3, atol=1e-5), k


# ------------------------------------------------------------------ 5. MinkGL with MAC / SPoC
@pytest.mark.parametrize("method", ["MAC", "SPoC"])
def test_minkgl_trains_with_mac_and_spoc(gpu, method):
    from egonn_amd import train
    from egonn_amd.model import PoolingWrapper
    case = H.load_case("egonn_train_cart03")
    model = gpu.model_factory(gpu.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.3))
    w = H.seeded_weights(int(case["weight_seed"]))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    ch = model.global_pooling.in_dim
    model.global_pool_method, model.global_pooling = method, PoolingWrapper(method, ch, ch)      # no parameters either way
    model = model.cuda().train()
    coords = torch.from_numpy(case["coords"]).cuda()
    y = model({"coords": coords, "features": torch.ones((len(coords), 1), device="cuda")}, disable_local_head=True)["global"]
    R = torch.from_numpy(np.random.default_rng(4).standard_normal(tuple(y.shape)).astype(np.float32)).cuda()
    (y * R).sum().backward()
    for k, p in model.named_parameters():
        if k.startswith("global_pooling"):
            continue
        if p.grad is None:
            assert k.startswith("local_"), k                 # only the disabled local branch is left without a gradient
        else:
            assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    assert any(p.grad is not None for k, p in model.named_parameters() if k.startswith("trunk."))
    # the train-mode features once more (batch statistics: the same values), pooled by the eval-mode kernels
    ctx = model.context()
    with torch.no_grad():
        lvl, x = train.head_forward(model.global_head, ctx, train.trunk_forward(model, ctx))
        net = model.global_descriptor_decoder.net
        x = train.LinearFn.apply(x, net[0].linear.weight, net[0].linear.bias, ctx, True)
        x = train.LinearFn.apply(x, net[2].linear.weight, net[2].linear.bias, ctx, False)
        want = ctx.global_max_pool(lvl, x) if method == "MAC" else ctx.global_avg_pool(lvl, x)
    assert torch.equal(y.detach(), want)


# ------------------------------------------------------------------ 6. TrainStep
def test_train_step_with_netvladgc_minkloc_is_bitwise_deterministic(gpu):
    from egonn_amd.train import TrainStep
    name = "minkloc_netvladgc_train_cart03"
    case = H.load_case(name)
    coords = torch.from_numpy(case["coords"]).cuda()
    batch = {"coords": coords, "features": torch.ones((len(coords), 1), device="cuda"), "batch_size": 5}
    pos = torch.zeros((5, 5), dtype=torch.bool)
    pos[0, 1] = pos[1, 0] = pos[2, 3] = pos[3, 2] = True
    neg = ~pos & ~torch.eye(5, dtype=torch.bool)
    runs = []
    for _ in range(2):
        _, model = _minkloc(gpu, name)
        step = TrainStep(model, torch.optim.SGD(model.parameters(), lr=0.0), margin=0.2)
        loss, stats = step(batch, pos, neg, step_optimizer=False)
        assert np.isfinite(float(loss))
        runs.append((float(loss), {k: p.grad.detach().clone() for k, p in model.named_parameters()}))
    assert runs[0][0] == runs[1][0]
    for k, g in runs[0][1].items():
        assert g is not None and torch.isfinite(g).all(), k
        assert torch.equal(g, runs[1][1][k]), k
