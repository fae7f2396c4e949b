"""CPU tests of MinkLoc's pooling surface: a float64 numpy restatement of NetVLAD / NetVLAD-GC (the contract egonn_netvlad
implements) pinned against the reference graph's fixtures, the module tree's state_dict against the reference's, the
`output_dim` model parameter, and the paths that refuse to run.

Restated contract (reference layers/pooling.py:89-109, layers/netvlad.py:18-112, eval mode), per scan b with rows X_b:
  A = softmax_k(bn1(X_b @ Wc));  a_sum_k = sum_r A[r,k] + (Nmax - n_b) * softmax_k(bn1(0))   (zero padding to Nmax)
  V[c,k] = sum_r X[r,c] A[r,k] - a_sum_k W2[c,k];  vlad = normalize(normalize_c(V) in c-major order)
  y = bn2(vlad @ H);  netvladgc: y = y * sigmoid(bn_g(y @ Wg))."""
import json
import os

import numpy as np
import pytest
import torch

from tests import helpers as H

NETVLAD_CASES = ["minkloc_netvlad_cart03", "minkloc_netvladgc_cart03"]
POOLING_CASES = NETVLAD_CASES + ["minkloc_mac_cart03", "minkloc_spoc_cart03"]
PREFIX = "pooling.pooling.net_vlad."


def _bn(w, prefix, x, eps=1e-5):
    g = lambda k: np.asarray(w[prefix + k], dtype=np.float64)          # noqa: E731
    return (x - g("running_mean")) / np.sqrt(g("running_var") + eps) * g("weight") + g("bias")


def _normalize(v, axis):
    return v / np.maximum(np.linalg.norm(v, axis=axis, keepdims=True), 1e-12)


def netvlad_f64(feats, offsets, w, gating, prefix=PREFIX):
    """float64 NetVLAD(-GC) over the scans [offsets[b], offsets[b+1]) of `feats` (rows x C); w: state_dict arrays."""
    f = lambda k: np.asarray(w[prefix + k], dtype=np.float64)           # noqa: E731
    wc, w2, hw = f("cluster_weights"), f("cluster_weights2")[0], f("hidden1_weights")
    x = np.asarray(feats, dtype=np.float64)
    n = np.diff(np.asarray(offsets))
    nmax = int(n.max())
    pad = _bn(w, prefix + "bn1.", np.zeros(wc.shape[1]))
    pad = np.exp(pad - pad.max())
    pad /= pad.sum()
    out = []
    for b in range(len(n)):
        xb = x[offsets[b]:offsets[b + 1]]
        z = _bn(w, prefix + "bn1.", xb @ wc)
        a = np.exp(z - z.max(axis=1, keepdims=True))
        a /= a.sum(axis=1, keepdims=True)
        a_sum = a.sum(axis=0) + (nmax - n[b]) * pad
        v = xb.T @ a - a_sum[None, :] * w2                    # (C, 64)
        vlad = _normalize(_normalize(v, 0).reshape(-1), 0)    # index c*64 + k
        y = _bn(w, prefix + "bn2.", vlad @ hw)
        if gating:
            g = _bn(w, prefix + "context_gating.bn1.", y @ f("context_gating.gating_weights"))
            y = y / (1.0 + np.exp(-g))
        out.append(y)
    return np.stack(out)


def _case(name):
    case = H.load_case(name)
    return case, H.seeded_weights(case["weight_seed"], name)


@pytest.mark.parametrize("name", NETVLAD_CASES)
def test_restatement_reproduces_reference_graph(name):
    case, w = _case(name)
    gating = str(case["pooling"]) == "netvladgc"
    off = case["backbone_offsets"]
    got = netvlad_f64(case["backbone_feats"], off, w, gating)
    assert got.shape == case["global"].shape == (2, int(case["output_dim"]))
    np.testing.assert_allclose(got, case["global"], rtol=1e-5, atol=1e-5)
    if "global_alone" in case:
        s = int(case["alone_scan"])
        alone = netvlad_f64(case["backbone_feats"][off[s]:off[s + 1]], [0, off[s + 1] - off[s]], w, gating)
        np.testing.assert_allclose(alone, case["global_alone"], rtol=1e-5, atol=1e-5)
        # the pad rule is visible: the same scan alone and in a batch with a larger one differ well above 1e-4
        assert np.abs(case["global_alone"][0] - case["global"][s]).max() > 1e-4
        assert np.abs(alone[0] - got[s]).max() > 1e-4


@pytest.mark.parametrize("name", ["minkloc_mac_cart03", "minkloc_spoc_cart03"])
def test_mac_spoc_fixtures_are_plain_max_and_mean(name):
    case = H.load_case(name)
    off, x = case["backbone_offsets"], case["backbone_feats"].astype(np.float64)
    red = np.max if str(case["pooling"]) == "MAC" else np.mean
    want = np.stack([red(x[off[b]:off[b + 1]], axis=0) for b in range(len(off) - 1)])
    np.testing.assert_allclose(want, case["global"], rtol=1e-5, atol=1e-6)


def _minkloc(name):
    from egonn_amd import ModelParams, model_factory
    case = H.load_case(name)
    mp = ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=0.3, block=str(case["block"]),
                     pooling=str(case["pooling"]), output_dim=int(case["output_dim"]))
    return model_factory(mp)


@pytest.mark.parametrize("name", POOLING_CASES)
def test_minkloc_state_dict_matches_reference(name):
    m = _minkloc(name)
    sd = m.state_dict()
    ref = H.state_dict_shapes(name)
    assert list(sd.keys()) == list(ref.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == ref[k], k
    if str(H.load_case(name)["pooling"]) == "netvladgc":
        assert sum(k.startswith(PREFIX) for k in sd) == 19
    m.load_state_dict({k: torch.from_numpy(v) for k, v in H.seeded_weights(H.load_case(name)["weight_seed"], name).items()},
                      strict=True)
    assert m.pooled_feature_size == m.output_dim == int(H.load_case(name)["output_dim"])


def test_model_params_output_dim():
    from egonn_amd import ModelParams
    assert ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=0.3).output_dim == 256
    mp = ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=0.3, pooling="netvladgc", output_dim=128)
    assert mp.output_dim == 128 and mp.pooling == "netvladgc"


def test_seeded_netvlad_weights_follow_reference_init_scale():
    from egonn_amd.synth import seeded_tensor
    c, d = 256, 128
    for key, shape, fan in (("cluster_weights", (c, 64), c), ("cluster_weights2", (1, c, 64), c),
                            ("hidden1_weights", (c * 64, d), c), ("context_gating.gating_weights", (d, d), d)):
        t = seeded_tensor(1, PREFIX + key, shape)
        assert t.shape == shape and t.dtype == np.float32
        assert abs(t.std() * np.sqrt(fan) - 1.0) < 0.1, key


def test_minkloc_refuses_what_it_does_not_implement():
    from egonn_amd import ModelParams, model_factory
    from egonn_amd.model import MinkGL, MinkHead, MinkTrunk
    from egonn_amd.quantization import CartesianQuantizer
    batch = {"coords": torch.zeros((1, 4), dtype=torch.int32), "features": torch.ones((1, 1))}
    for method in ("netvlad", "netvladgc", "MAC", "SPoC"):
        m = model_factory(ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=0.3, pooling=method,
                                      output_dim=256 if method in ("MAC", "SPoC") else 128)).train()
        with pytest.raises(NotImplementedError, match=method):        # before any device work (the model is on the CPU)
            m(batch)
    with pytest.raises(NotImplementedError, match="Unknown pooling method"):
        model_factory(ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=0.3, pooling="GeMM"))
    for method in ("netvlad", "netvladgc"):
        with pytest.raises(NotImplementedError, match=method):
            MinkGL(MinkTrunk(1, [32, 64]), local_head=MinkHead([1], [32], 16), local_descriptor_size=8,
                   global_head=MinkHead([2], [64], 32), global_descriptor_size=16, global_pool_method=method,
                   quantizer=CartesianQuantizer(0.1))


def test_pooling_fixtures_are_complete():
    for name in POOLING_CASES:
        case = H.load_case(name)
        for k in ("coords", "global", "backbone_coords", "backbone_feats", "backbone_offsets", "weight_seed", "block",
                  "pooling", "output_dim"):
            assert k in case, (name, k)
        off = case["backbone_offsets"]
        assert off[0] == 0 and off[-1] == len(case["backbone_feats"]) == len(case["backbone_coords"])
        assert np.array_equal(case["backbone_coords"][:, 0], np.repeat(np.arange(len(off) - 1), np.diff(off)))
        with open(os.path.join(H.GOLDEN, f"{name}_state_dict_shapes.json")) as f:
            assert json.load(f)
