"""GPU tests of the SEBasicBlock path: the gate kernels (egonn_se_gate / egonn_se_gate_backward, egonn_amd/csrc/train.hip)
against float64 on the CPU (tests/se_ref.py), MinkLoc(block='SEBasicBlock') in eval and train mode against fixtures the
reference's own graph wrote (tests/golden/make_golden_se.py), batch invariance and run-to-run reproducibility."""
import zlib

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import se_ref as S

pytestmark = pytest.mark.gpu

EVAL, TRAIN = "minkloc_se_cart03", "minkloc_se_train_cart03"


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


def _gate(lib, arrs, hidden=True):
    """egonn_se_gate + egonn_se_gate_backward through the C ABI -> gate, hidden, {gradients} as numpy"""
    mean, w1, b1, w2, b2, gg = (torch.from_numpy(v).cuda() for v in arrs)
    B, c = mean.shape
    h = w1.shape[0]
    st = torch.cuda.current_stream().cuda_stream
    gate = torch.full_like(mean, np.nan)
    hid = torch.full((B, h), np.nan, device="cuda")
    lib.check(lib.load().egonn_se_gate(mean.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), B, c, h,
                                       gate.data_ptr(), hid.data_ptr() if hidden else None, st))
    if not hidden:
        return gate.cpu().numpy()
    out = {k: torch.full(s, np.nan, device="cuda") for k, s in (("mean", (B, c)), ("w1", (h, c)), ("b1", (h,)), ("w2", (c, h)),
                                                               ("b2", (c,)))}
    lib.check(lib.load().egonn_se_gate_backward(gg.data_ptr(), gate.data_ptr(), hid.data_ptr(), mean.data_ptr(), w1.data_ptr(),
                                                w2.data_ptr(), B, c, h, out["mean"].data_ptr(), out["w1"].data_ptr(),
                                                out["b1"].data_ptr(), out["w2"].data_ptr(), out["b2"].data_ptr(), st))
    return gate.cpu().numpy(), hid.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("dead", [None, 0], ids=["live", "dead_sample0"])
@pytest.mark.parametrize("B,c", S.SHAPES)
def test_se_gate_kernels_match_float64(gpu, B, c, dead):
    """forward and all five gradients at hidden widths 1 .. 16 and a batch that is no multiple of a wave; with `dead` every
    pre-ReLU value of sample 0 is negative: its gate is sigmoid(b2) and nothing flows back to its means.  Tolerances: the
    per-operator ones of tests/test_gpu_train.py (forward rtol 1e-4 / atol 1e-6; gradients rtol 1e-3, atol 1e-4 max|ref| + 1e-9)."""
    from egonn_amd import _lib
    arrs = S.inputs(B, c, 100 + c, dead)
    gate, hid, grads = _gate(_lib, arrs)
    wg, wh, pre = S.forward(*arrs[:5])
    want = S.backward(arrs[5], *arrs[:5])
    print(f"gate max err {np.abs(gate - wg).max():.3g}  hidden max err {np.abs(hid - wh).max():.3g}")
    assert np.allclose(gate, wg, rtol=1e-4, atol=1e-6) and np.allclose(hid, wh, rtol=1e-4, atol=1e-6)
    assert ((hid > 0) == (pre > 0)).all() or np.abs(pre).min() < 1e-5          # no ReLU decision within fp32 noise of zero
    for k, ref in want.items():
        scale = float(np.abs(ref).max())
        print(f"grad {k} max err {np.abs(grads[k] - ref).max():.3g} of {scale:.3g}")
        assert np.isfinite(grads[k]).all() and np.allclose(grads[k], ref, rtol=1e-3, atol=1e-4 * scale + 1e-9), k
    if dead is not None:
        assert (pre[dead] < 0).all() and (hid[dead] == 0).all() and (grads["mean"][dead] == 0).all()
        assert np.allclose(gate[dead], 1.0 / (1.0 + np.exp(-arrs[4].astype(np.float64))), rtol=1e-4, atol=1e-6)
    assert np.array_equal(_gate(_lib, arrs, hidden=False), gate)                # hidden_out is optional
    again = _gate(_lib, arrs)
    assert np.array_equal(again[0], gate) and all(np.array_equal(again[2][k], grads[k]) for k in grads)


def test_se_gate_is_independent_of_the_batch_around_a_sample(gpu):
    """gate and grad_mean of a sample are bitwise those of the sample alone; the parameter gradients of a batch are bitwise
    the serial sum over its samples in order"""
    from egonn_amd import _lib
    arrs = S.inputs(67, 256, 7)
    gate, hid, grads = _gate(_lib, arrs)
    acc = {k: np.zeros_like(grads[k]) for k in ("w1", "b1", "w2", "b2")}
    for b in (0, 5, 63, 64, 66):
        one = tuple(v[b:b + 1] if v.shape[0] == 67 and v.ndim == 2 and v.shape[1] == 256 else v for v in arrs)
        g1, h1, gr1 = _gate(_lib, one)
        assert np.array_equal(g1[0], gate[b]) and np.array_equal(h1[0], hid[b]) and np.array_equal(gr1["mean"][0], grads["mean"][b])
    sub = tuple(v[:9] if v.shape[0] == 67 and v.ndim == 2 and v.shape[1] == 256 else v for v in arrs)
    g9 = _gate(_lib, sub)[2]
    for b in range(9):
        one = tuple(v[b:b + 1] if v.shape[0] == 67 and v.ndim == 2 and v.shape[1] == 256 else v for v in arrs)
        gr1 = _gate(_lib, one)[2]
        for k in acc:
            acc[k] = (acc[k] + gr1[k]).astype(np.float32)
    for k in ("b1", "b2"):                       # plain sums: fp32 addition in sample order, exactly
        assert np.array_equal(acc[k], g9[k]), k
    for k in ("w1", "w2"):                       # fused multiply-adds in the kernel: one rounding fewer per sample
        assert np.allclose(acc[k], g9[k], rtol=1e-5, atol=1e-6 * np.abs(g9[k]).max()), k


def _se_model(gpu, seed):
    mp = gpu.ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=0.3, block="SEBasicBlock",
                         planes="32,64,64", layers="1,1,1")
    m = gpu.model_factory(mp)
    w = H.seeded_weights(int(seed), EVAL)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return m.to("cuda")


def test_se_eval_forward_matches_reference_and_is_batch_invariant(gpu):
    """MinkFPN(SEBasicBlock) + GeM vs the reference graph on two scans of different size (backbone rows joined by coordinate;
    the bars of test_gpu_parity.test_minkloc_forward_matches_reference_graph); each scan of the batch equals, bitwise, the
    scan run alone"""
    case = H.load_case(EVAL)
    assert str(case["block"]) == "SEBasicBlock" and int(case["n_scans"]) == 2
    m = _se_model(gpu, case["weight_seed"]).eval()
    c4 = case["coords"]
    order = np.random.default_rng(3).permutation(len(c4))
    y = m({"coords": torch.from_numpy(c4[order]), "features": torch.ones((len(c4), 1))})
    g = y["global"].cpu().numpy()
    assert g.shape == case["global"].shape and set(y.keys()) == {"global"}
    err = H.cosine_err(g, case["global"])
    print("global cosine err", err)
    assert err.max() <= 1e-4
    np.testing.assert_allclose(g, case["global"], rtol=1e-3, atol=1e-4)
    ctx = m.context()
    with torch.no_grad():
        level, x = m.backbone.run(ctx, ctx.gather_input(torch.ones((len(c4), 1), device="cuda")))
    rows = ctx.level_coords(level).cpu().numpy()
    perm = H.join_perm(rows, case["backbone_coords"])                      # asserts identical coordinate sets
    xb, want = x.cpu().numpy()[perm], case["backbone_feats"].astype(np.float32)
    berr = H.cosine_err(xb, want)
    print("backbone row cosine err max", berr.max())
    assert berr.max() <= 1e-4
    for b in range(2):
        cb = c4[c4[:, 0] == b].copy()
        cb[:, 0] = 0
        alone = m({"coords": torch.from_numpy(cb), "features": torch.ones((len(cb), 1))})["global"]
        assert torch.equal(alone[0], y["global"][b]), b
    assert H.cosine_err(g[:1], g[1:]).max() > 1e-3                         # the two scans are not interchangeable


def _digest(name, g):
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    r = np.random.default_rng(zlib.crc32(name.encode())).standard_normal(g.size)
    return np.concatenate([[np.linalg.norm(g), float(g @ r)], g[:64] if g.size > 4096 else g])


def _train_step(gpu, case):
    model = _se_model(gpu, case["weight_seed"]).train()
    coords = torch.from_numpy(case["coords"]).cuda()
    g = model({"coords": coords, "features": torch.ones((len(coords), 1), device="cuda")})["global"]
    R = torch.from_numpy(np.random.default_rng(int(case["proj_seed"])).standard_normal(case["global"].shape).astype(np.float32)).cuda()
    loss = (g * R).sum()
    loss.backward()
    return model, g, loss


def test_se_train_step_matches_reference_fixture(gpu):
    """the assertions of test_gpu_train.test_minkloc_train_step_matches_reference_fixture on the SEBasicBlock fixture: the
    parameters with a gradient are the fixture's, the four se.fc tensors of every block among them"""
    case = H.load_case(TRAIN)
    model, g, loss = _train_step(gpu, case)
    err = H.cosine_err(g.detach().cpu().numpy(), case["global"])
    print("global cosine err", err, "loss", loss.item(), "want", float(case["loss"]))
    assert err.max() <= 1e-4
    assert abs(loss.item() - float(case["loss"])) <= 2e-3 * max(1.0, abs(float(case["loss"])))
    grads = {k: p.grad for k, p in model.named_parameters()}
    keys = [k[5:] for k in case if k.startswith("grad/")]
    assert set(keys) == set(grads) and sum(".se.fc." in k for k in keys) == 12
    bad, worst = [], (None, 0.0)
    for k in keys:
        assert grads[k] is not None, k
        mine, ref = _digest(k, grads[k].detach().cpu().numpy()), case["grad/" + k]
        norm = max(ref[0], 1e-12)
        e = max(abs(mine[0] - ref[0]) / norm, abs(mine[1] - ref[1]) / norm,
                float(np.abs(mine[2:] - ref[2:]).max()) / max(float(np.abs(ref[2:]).max()), 1e-12))
        worst = max(worst, (k, e), key=lambda t: t[1])
        if e > 5e-3:
            bad.append((k, e))
    print("worst gradient digest", worst)
    assert not bad, bad
    sd = model.state_dict()
    for k in [k[4:] for k in case if k.startswith("buf/")]:
        assert np.allclose(sd[k].cpu().numpy(), case["buf/" + k], rtol=1e-3, atol=1e-5), k


def test_se_train_step_is_bitwise_repeatable(gpu):
    case = H.load_case(TRAIN)
    runs = []
    for _ in range(2):
        model, g, loss = _train_step(gpu, case)
        runs.append((float(loss), {k: p.grad.detach().clone() for k, p in model.named_parameters()}))
    assert runs[0][0] == runs[1][0]
    for k, g in runs[0][1].items():
        assert torch.equal(g, runs[1][1][k]), k
