"""Host-side tests of the SEBasicBlock surface (no GPU): the module tree of MinkLoc(block='SEBasicBlock') against the
reference's state_dict (fixture written by tests/golden/make_golden_se.py), the Bottleneck refusal, the seeded weights, the
argument checks of the two C entry points and the float64 restatement the GPU test compares the gate kernels with."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import se_ref as S

NAME = "minkloc_se_cart03"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    return egonn_amd


def _model(mod, block="SEBasicBlock"):
    return mod.model_factory(mod.ModelParams(model="MinkLoc", coordinates="cartesian", quantization_step=0.3, block=block,
                                             planes="32,64,64", layers="1,1,1", num_top_down=1, conv0_kernel_size=5,
                                             feature_size=256, pooling="GeM"))


def test_se_state_dict_matches_reference_keys_shapes_and_order(built):
    want = H.state_dict_shapes(NAME)
    sd = _model(built).state_dict()
    assert list(sd.keys()) == list(want.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == want[k], k
    se = [k for k in want if ".se.fc." in k]
    assert len(se) == 12 and all(k.endswith(("se.fc.0.linear.weight", "se.fc.0.linear.bias", "se.fc.2.linear.weight",
                                             "se.fc.2.linear.bias")) for k in se)
    assert want["backbone.blocks.0.0.se.fc.0.linear.weight"] == (2, 32) and want["backbone.blocks.2.0.se.fc.2.linear.weight"] == (64, 4)


def test_se_reference_checkpoint_loads(built):
    m = _model(built)
    w = H.seeded_weights(int(H.load_case(NAME)["weight_seed"]), NAME)
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    assert not res.missing_keys and not res.unexpected_keys
    assert np.array_equal(m.backbone.blocks[1][0].se.fc[2].linear.bias.detach().numpy(), w["backbone.blocks.1.0.se.fc.2.linear.bias"])


def test_bottleneck_still_raises_and_says_why(built):
    with pytest.raises(NotImplementedError) as ei:
        _model(built, "Bottleneck")
    msg = str(ei.value)
    assert "models/resnet.py:107" in msg and "models/minkfpn.py:49" in msg and "planes[-1] * 4" in msg
    with pytest.raises(NotImplementedError):
        _model(built, "SEBottleneck")
    for block in ("BasicBlock", "ECABasicBlock"):                      # the other blocks keep their trees: no se keys
        assert not any(".se." in k for k in _model(built, block).state_dict())


def test_seeded_weights_keep_every_existing_key(built):
    """the se.fc rule of egonn_amd.synth.seeded_tensor touches no key the older fixtures use: their rules restated"""
    from egonn_amd.synth import seeded_tensor, _key_seed
    for key, shape in (("global_descriptor_decoder.net.0.linear.weight", (128, 64)), ("x.net.2.linear.bias", (7,))):
        rng = np.random.default_rng(_key_seed(22, key))
        want = rng.standard_normal(shape) * (np.sqrt(2.0 / shape[1]) if key.endswith("weight") else 0.05)
        assert np.array_equal(seeded_tensor(22, key, shape), want.astype(np.float32)), key
    shapes = H.state_dict_shapes("minkloc_eca_cart03")
    assert not any(".se.fc." in k for k in shapes)
    w = seeded_tensor(5, "backbone.blocks.0.0.se.fc.0.linear.weight", (2, 32))
    assert w.std() > 2.0 * np.sqrt(2.0 / 32)                          # the wider SE rule is in force for the new keys


def test_se_gate_argument_checks_need_no_gpu(built):
    """unsupported sizes and null arguments return the invalid status before anything is launched"""
    from egonn_amd import _lib
    lib = _lib.load()
    one = 256                     # non-null, never dereferenced: every call below fails its argument check first
    for c, h in ((8, 1), (24, 1), (272, 17), (32, 1), (32, 4), (0, 0), (64, 8)):
        assert lib.egonn_se_gate(one, one, one, one, one, 2, c, h, one, None, None) == 1, (c, h)
        assert lib.egonn_se_gate_backward(one, one, one, one, one, one, 2, c, h, one, one, one, one, one, None) == 1, (c, h)
    assert "se_gate" in _lib._err(lib)
    assert lib.egonn_se_gate(None, one, one, one, one, 2, 32, 2, one, None, None) == 1
    assert lib.egonn_se_gate_backward(one, one, None, one, one, one, 2, 32, 2, one, one, one, one, one, None) == 1
    assert lib.egonn_se_gate(one, one, one, one, one, -1, 32, 2, one, None, None) == 1
    assert lib.egonn_se_gate(one, one, one, one, one, 0, 32, 2, one, None, None) == 0          # empty batch: nothing to do


@pytest.mark.parametrize("B,c", S.SHAPES)
def test_se_restatement_matches_torch_autograd(B, c):
    for dead in (None, 0):
        mean, w1, b1, w2, b2, gg = S.inputs(B, c, 100 + c, dead)
        t = [torch.from_numpy(v).double().requires_grad_(True) for v in (mean, w1, b1, w2, b2)]
        hid = torch.relu(torch.nn.functional.linear(t[0], t[1], t[2]))
        gate = torch.sigmoid(torch.nn.functional.linear(hid, t[3], t[4]))
        (gate * torch.from_numpy(gg).double()).sum().backward()
        g, h, pre = S.forward(mean, w1, b1, w2, b2)
        assert np.allclose(g, gate.detach().numpy(), rtol=1e-12, atol=1e-14)
        got = S.backward(gg, mean, w1, b1, w2, b2)
        for k, tt in zip(("mean", "w1", "b1", "w2", "b2"), t):
            assert np.allclose(got[k], tt.grad.numpy(), rtol=1e-10, atol=1e-13), k
        if dead is not None:
            assert (pre[dead] < 0).all() and np.allclose(g[dead], 1 / (1 + np.exp(-b2.astype(np.float64))), rtol=1e-14)
            assert (got["mean"][dead] == 0).all()
        else:
            assert 0.1 < (pre > 0).mean() < 0.9 or pre.size < 4             # both sides of the ReLU are exercised
