"""CPU tests of the train-mode pooling surface: a differentiable float64 torch restatement of train-mode NetVLAD / NetVLAD-GC
that works from rows and offsets (the pad rows of the reference's zero padding enter analytically, no padded tensor is built)
against the operator fixture the reference's own NetVLADLoupe produced (tests/golden/make_golden_pooling_train.py), the
fixtures' completeness, and the guards that need no device."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as H

OP_FILES = ["netvlad_train_ref", "netvlad_train_ref_c64", "netvlad_train_ref_c64_gradh", "netvlad_train_ref_c64_alone",
            "netvlad_train_ref_c64_alone_gradh"]
OP_VARIANTS = ["c16", "c64", "c16_alone", "c64_alone"]
E2E_CASES = {"minkloc_netvlad_train_cart03": "minkloc_netvlad_cart03", "minkloc_netvladgc_train_cart03": "minkloc_netvladgc_cart03",
             "minkloc_mac_train_cart03": "minkloc_mac_cart03", "minkloc_spoc_train_cart03": "minkloc_spoc_cart03"}
PARAM_KEYS = ["cluster_weights", "cluster_weights2", "hidden1_weights", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias",
              "context_gating.gating_weights", "context_gating.bn1.weight", "context_gating.bn1.bias"]
LIMIT = 1 << 20        # committed-file size limit


def load_op_fixture():
    """the operator fixture, merged from its files: {variant: {key: array}}"""
    flat = {}
    for f in OP_FILES:
        flat.update(H.load_case(f))
    out = {v: {} for v in OP_VARIANTS}
    for k, a in flat.items():
        head, _, rest = k.partition("/")
        if head in out:
            out[head][rest] = a
    out["meta"] = {k[5:]: a for k, a in flat.items() if k.startswith("meta/")}
    return out


def op_state(case):
    """the seeded NetVLADLoupe state (float32 numpy) of a fixture variant: the generator's seeded_tensor(seed, key, shape)"""
    from egonn_amd.synth import seeded_tensor
    c, d, gating, seed = int(case["C"]), int(case["D"]), bool(case["gating"]), int(case["seed"])
    shapes = {"cluster_weights": (c, 64), "cluster_weights2": (1, c, 64), "hidden1_weights": (c * 64, d)}
    for bn, n in (("bn1", 64), ("bn2", d)) + ((("context_gating.bn1", d),) if gating else ()):
        shapes.update({f"{bn}.weight": (n,), f"{bn}.bias": (n,), f"{bn}.running_mean": (n,), f"{bn}.running_var": (n,)})
    if gating:
        shapes["context_gating.gating_weights"] = (d, d)
    return {k: seeded_tensor(seed, k, s) for k, s in shapes.items()}


def netvlad_train_f64(x, offsets, p, buf, gating, eps=1e-5, momentum=0.1, head=True):
    """Train-mode NetVLADLoupe under NetVLADWrapper's zero padding, float64 torch, differentiable, from the rows x (N, C) and
    the scan offsets (B + 1).  p: parameters, buf: running statistics (both dicts of float64 tensors, reference key names).
    The (Nmax - n_b) pad rows of scan b are never built: a pad row has the logits 0 before bn1, so
      * bn1's batch statistics over the M = B * Nmax rows are mean = (sum_real z) / M, var = (sum_real z^2) / M - mean^2;
      * every pad row has the assignment softmax(shift), shift = beta - mean * gamma * invstd, and adds it to a_sum_b;
      * pad rows add nothing to X^T A (x = 0).
    Autograd through these expressions carries the pad rows' share of the gradients of gamma, beta, mean and variance.
    head=False stops before bn2 and the gating: what NetVLADFn (egonn_netvlad_train_forward) returns.
    Returns (y (B, D), {buffer name: value after the step})."""
    off = [int(o) for o in offsets]
    B = len(off) - 1
    n = [off[b + 1] - off[b] for b in range(B)]
    nmax = max(n)
    M = float(B * nmax)
    wc, w2, hid = p["cluster_weights"], p["cluster_weights2"][0], p["hidden1_weights"]
    z = x @ wc
    mean = z.sum(0) / M
    var = (z * z).sum(0) / M - mean * mean
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = p["bn1.weight"] * invstd
    shift = p["bn1.bias"] - mean * scale
    new = {"bn1.running_mean": (1 - momentum) * buf["bn1.running_mean"] + momentum * mean.detach(),
           "bn1.running_var": (1 - momentum) * buf["bn1.running_var"] + momentum * var.detach() * M / (M - 1.0)}
    A = torch.softmax(z * scale + shift, dim=1)
    a_pad = torch.softmax(shift, dim=0)
    rows = []
    for b in range(B):
        xb, Ab = x[off[b]:off[b + 1]], A[off[b]:off[b + 1]]
        a_sum = Ab.sum(0) + float(nmax - n[b]) * a_pad
        V = xb.t() @ Ab - a_sum[None, :] * w2                         # (C, 64)
        V = F.normalize(V, dim=0, p=2)
        rows.append(F.normalize(V.reshape(1, -1), dim=1, p=2)[0])
    y = torch.stack(rows) @ hid
    if not head:
        return y, new

    def bn_rows(t, name):
        rm, rv = buf[name + ".running_mean"].clone(), buf[name + ".running_var"].clone()
        out = F.batch_norm(t, rm, rv, p[name + ".weight"], p[name + ".bias"], True, momentum, eps)
        new[name + ".running_mean"], new[name + ".running_var"] = rm, rv
        return out

    y = bn_rows(y, "bn2")
    if gating:
        g = bn_rows(y @ p["context_gating.gating_weights"], "context_gating.bn1")
        y = y * torch.sigmoid(g)
    return y, new


def run_f64(x, offsets, state, gating, upstream):
    """restatement + autograd on float32 inputs cast up: (y, grad x, {param: grad}, {buffer: value}) as float64 numpy"""
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in state.items() if "running" not in k}
    buf = {k: torch.from_numpy(v).double() for k, v in state.items() if "running" in k}
    xt = torch.from_numpy(np.asarray(x)).double().requires_grad_(True)
    y, new = netvlad_train_f64(xt, offsets, p, buf, gating)
    (y * torch.from_numpy(np.asarray(upstream)).double()).sum().backward()
    return (y.detach().numpy(), xt.grad.numpy(), {k: v.grad.numpy() for k, v in p.items()},
            {k: v.numpy() for k, v in new.items()})


NONZERO_IN_ALONE = ("bn2.bias", "context_gating.bn1.bias")


def grad_scale(fx, variant, key):
    """The magnitude an absolute tolerance on the gradient `key` of `variant` is relative to: max|ref|, except in the `alone`
    variants for every parameter but the biases of the two B-row BatchNorms.  There the B descriptors are equal, so both
    B-row BatchNorms have normalised values 0 (their weight gradients sum g * 0), bn2's backward hands scan b the gradient
    gamma * invstd * (g_b - mean g), and every gradient upstream is sum_b (g_b - mean g) J = 0 exactly (the gating matrix
    likewise): the fixture holds the float64 rounding of cancelling per-scan terms.  The scale is then that of ONE scan's term:
    the ragged case's max|ref| of the same tensor times the ratio of the two cases' max|grad x| (the amplification by bn2's
    invstd = eps^-1/2)."""
    ref = fx[variant]["grad/" + key]
    if not variant.endswith("_alone") or key in NONZERO_IN_ALONE:
        return float(np.abs(ref).max())
    base = fx[variant[:-len("_alone")]]
    amp = float(np.abs(fx[variant]["grad_x"]).max() / np.abs(base["grad_x"]).max())
    return max(float(np.abs(ref).max()), float(np.abs(base["grad/" + key]).max()) * amp)


@pytest.mark.parametrize("variant", OP_VARIANTS)
def test_restatement_matches_reference_fixture(variant):
    """the pad-row algebra (including the pad rows' share of the bn1 gradients) against the reference's own autograd on the
    zero-padded tensor, float64 both sides.  rtol 1e-9; the absolute floor 1e-12 * grad_scale is the float64 rounding of sums
    of thousands of terms of that magnitude that cancel (2^-53 each), not a tolerance on the algebra."""
    fx = load_op_fixture()
    case = fx[variant]
    y, gx, gp, bufs = run_f64(case["x"], case["offsets"], op_state(case), bool(case["gating"]), case["upstream"])

    def close(a, b, what):
        scale = grad_scale(fx, variant, what) if "grad/" + what in case else float(np.abs(b).max())
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12 * scale, err_msg=what)

    close(y, case["out"], "out")
    close(gx, case["grad_x"], "grad x")
    keys = [k for k in PARAM_KEYS if ("gating" not in k or bool(case["gating"]))]
    assert sorted(k[5:] for k in case if k.startswith("grad/")) == sorted(keys)
    for k in keys:
        close(gp[k], case["grad/" + k], k)
    for k, v in bufs.items():
        close(v, case["buf/" + k], k)
        assert int(case["buf/" + k.rsplit(".", 1)[0] + ".num_batches_tracked"]) == 1


def test_pad_term_vanishes_when_every_scan_is_the_largest():
    """alone variant: one scan repeated B times, n_b = Nmax: no pad row; the ragged batch's result for that scan differs"""
    fx = load_op_fixture()
    s = int(fx["meta"]["alone_scan"])
    for tag in ("c16", "c64"):
        case, alone = fx[tag], fx[tag + "_alone"]
        off = alone["offsets"]
        assert len(set(np.diff(off))) == 1 and np.diff(off)[0] == fx["meta"]["rows"][s]
        o = case["offsets"]
        assert np.array_equal(alone["x"][:off[1]], case["x"][o[s]:o[s + 1]])
        assert np.abs(alone["out"] - alone["out"][0]).max() < 1e-6          # B equal descriptors: bn2 maps them to beta (gated)
        assert np.abs(alone["out"][0] - case["out"][s]).max() > 1e-3


def test_train_fixtures_are_complete():
    fx = load_op_fixture()
    assert list(fx["meta"]["rows"]) == [1, 63, 64, 65, 129, 300, 17, 128]
    for v in OP_VARIANTS:
        case = fx[v]
        for k in ("x", "offsets", "out", "upstream", "grad_x", "C", "D", "gating", "seed", "grad/cluster_weights",
                  "grad/cluster_weights2", "grad/hidden1_weights", "grad/bn1.weight", "grad/bn1.bias", "grad/bn2.weight",
                  "grad/bn2.bias", "buf/bn1.running_mean", "buf/bn1.running_var", "buf/bn2.running_mean", "buf/bn2.running_var"):
            assert k in case, (v, k)
        assert case["x"].dtype == np.float32 and case["out"].dtype == np.float64
        assert case["grad_x"].shape == case["x"].shape and case["offsets"][-1] == len(case["x"])
        assert case["grad/hidden1_weights"].shape == (int(case["C"]) * 64, int(case["D"]))
    assert (int(fx["c16"]["C"]), int(fx["c16"]["D"]), int(fx["c16"]["gating"])) == (16, 16, 0)
    assert (int(fx["c64"]["C"]), int(fx["c64"]["D"]), int(fx["c64"]["gating"])) == (64, 32, 1)
    for f in OP_FILES + list(E2E_CASES):
        assert os.path.getsize(os.path.join(H.GOLDEN, f + ".npz")) <= LIMIT, f
    for name, shapes in E2E_CASES.items():
        case = H.load_case(name)
        for k in ("coords", "global", "loss", "weight_seed", "proj_seed", "block", "pooling", "output_dim"):
            assert k in case, (name, k)
        assert int(case["n_scans"]) == 5 and case["global"].shape == (5, int(case["output_dim"]))
        counts = np.bincount(case["coords"][:, 0])
        assert len(set(counts.tolist())) == 5                           # unequal sizes
        named = [k for k, s in H.state_dict_shapes(shapes).items() if "running" not in k and "num_batches" not in k]
        assert sorted(k[5:] for k in case if k.startswith("grad/")) == sorted(named), name    # no parameter without a gradient
        norms = np.array([case[k][0] for k in case if k.startswith("grad/")])
        if str(case["pooling"]).startswith("netvlad"):
            assert norms.min() >= 1e-6 * norms.max()                    # the comparison does not gate noise
    assert int(H.load_case("minkloc_mac_train_cart03")["mac_no_tie"]) == 1      # asserted by the generator on the backbone output


def test_cpu_model_in_train_mode_names_the_method():
    from egonn_amd import ModelParams, model_factory
    batch = {"coords": torch.zeros((1, 4), dtype=torch.int32), "features": torch.ones((1, 1))}
    for method in ("netvlad", "netvladgc", "MAC", "SPoC"):
        m = model_factory(ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=0.3, pooling=method,
                                      output_dim=256 if method in ("MAC", "SPoC") else 128)).train()
        with pytest.raises(NotImplementedError, match=f"pooling method '{method}' in train mode runs on the HIP device only"):
            m(batch)


def test_train_pooling_surface_exists_and_one_scan_is_refused():
    """NetVLADFn / GlobalMaxFn / pool exist; B = 1 raises ValueError (nn.BatchNorm1d's rule) before any device work; NetVLAD with
    a SyncBN group stays unimplemented"""
    from egonn_amd import train
    from egonn_amd.model import NetVLADLoupe
    assert issubclass(train.NetVLADFn, torch.autograd.Function) and issubclass(train.GlobalMaxFn, torch.autograd.Function)
    nv = NetVLADLoupe(16, 64, 16, gating=True)
    ctx = types.SimpleNamespace(batch_size=1)                # no device behind it: any device work would raise AttributeError
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        train.netvlad_pool(ctx, 0, torch.zeros((5, 16)), nv)
    wrapper = types.SimpleNamespace(net_vlad=nv)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        train.pool(ctx, 0, torch.zeros((5, 16)), wrapper, "netvladgc")
    with pytest.raises(NotImplementedError, match="process group"):
        train.pool(types.SimpleNamespace(batch_size=4), 0, torch.zeros((5, 16)), wrapper, "netvlad", group=object())
    with pytest.raises(NotImplementedError, match="Unknown pooling method"):
        train.pool(ctx, 0, torch.zeros((5, 16)), None, "GeMM")
