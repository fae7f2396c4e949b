"""CPU tests of the one-call MinkFPN path (csrc/minkfpn.hip, csrc/topdown.hip, egonn_amd/minkloc.py, GlobalExtractor, the
rotation sweep): the symbols, the argument checks that come before any launch, the model specification and the keys the
finalize asks for, the sequence of library calls, and what the new entry points refuse.

The new call sequences are stored in tests/golden/minkfpn_calls.json; a pull request that changes them on purpose regenerates
the file and shows the diff:

    python -m tests.test_minkfpn_host --write
"""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import test_graph_calls_host as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["egonn_minkfpn_finalize", "egonn_minkfpn_forward", "egonn_minkfpn_out_level", "egonn_topdown_step"]
GOLDEN_CALLS = os.path.join(REPO, "tests", "golden", "minkfpn_calls.json")
PER_OPERATOR = ("egonn_conv", "egonn_conv_transpose", "egonn_bn_fold", "egonn_block_tail", "egonn_add", "egonn_gem",
                "egonn_gather_input", "egonn_global_max_pool", "egonn_global_avg_pool", "egonn_coords_set")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


@pytest.fixture(scope="module")
def lib(built):
    from egonn_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.egonn_last_error().decode()


def _ints(v):
    return (C.c_int * len(v))(*v)


def _mp(**kw):
    from egonn_amd import ModelParams
    return ModelParams(coordinates="cartesian", quantization_step=0.3, **kw)


def test_new_symbols_are_declared_listed_and_exported(lib):
    from egonn_amd import _lib
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    declared = set(re.findall(r"\b(egonn_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "EGONN_MINKFPN_SPLIT_TOPDOWN = 1" in header and _lib.MINKFPN_SPLIT_TOPDOWN == 1


@pytest.mark.parametrize("kw,word", [
    (dict(n_levels=0), "n_levels"),
    (dict(n_levels=8), "n_levels"),
    (dict(planes=[32, 48, 64]), "planes[1] = 48"),
    (dict(num_top_down=4), "num_top_down"),
    (dict(block=2), "block 2"),
    (dict(pooling=4), "pooling 4"),
    (dict(feature_size=48), "feature_size 48"),
    (dict(layers=[1, 0, 1]), "layers[1] = 0"),
    (dict(planes=[64, 64, 64]), "planes[0] = 64"),
])
def test_finalize_rejects_bad_arguments_before_any_device_work(lib, kw, word):
    """no tensor is registered: a status other than 1 would mean the finalize went past its argument checks"""
    a = dict(n_levels=3, planes=[32, 64, 64], layers=[1, 1, 1], num_top_down=1, feature_size=256, block=0, pooling=1)
    a.update(kw)
    planes = (a["planes"] + [32] * 8)[:max(a["n_levels"], 8)]
    layers = (a["layers"] + [1] * 8)[:max(a["n_levels"], 8)]
    m = C.c_void_p()
    assert lib.egonn_model_create(C.byref(m)) == 0
    try:
        rc = lib.egonn_minkfpn_finalize(m, a["n_levels"], _ints(planes), _ints(layers), a["num_top_down"], a["feature_size"],
                                        a["block"], a["pooling"], None)
        assert rc == 1 and word in _err(lib), (rc, _err(lib))
    finally:
        lib.egonn_model_destroy(m)


def test_out_level(lib):
    lv = C.c_int(-1)
    assert lib.egonn_minkfpn_out_level(3, 1, C.byref(lv)) == 0 and lv.value == 2
    assert lib.egonn_minkfpn_out_level(4, 4, C.byref(lv)) == 0 and lv.value == 0
    assert lib.egonn_minkfpn_out_level(3, 4, C.byref(lv)) == 1 and "num_top_down" in _err(lib)
    assert lib.egonn_minkfpn_out_level(3, 1, None) == 1


def test_forward_and_topdown_step_check_their_arguments_before_any_launch(lib):
    """a null context is what is left when every argument check has passed: status 4; the listed mistakes are status 1"""
    m = C.c_void_p()
    assert lib.egonn_model_create(C.byref(m)) == 0
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)            # 16-byte aligned, as the feature maps must be
    try:
        assert lib.egonn_minkfpn_forward(None, m, 0, None, None, None) == 1 and "both null" in _err(lib)
        assert lib.egonn_minkfpn_forward(None, m, 0, p, None, None) == 1 and "not finalized" in _err(lib)
        assert lib.egonn_minkfpn_forward(None, None, 0, p, None, None) == 1 and "not finalized" in _err(lib)
        assert lib.egonn_minkfpn_forward(None, m, 6, p, None, None) == 1 and "flags" in _err(lib)
    finally:
        lib.egonn_model_destroy(m)
    step = lib.egonn_topdown_step
    assert step(None, 7, p, p, p, p, 256, 64, p, None) == 1 and "level_out 7" in _err(lib)
    assert step(None, -1, p, p, p, p, 256, 64, p, None) == 1
    assert step(None, 2, p, p, p, p, 96, 64, p, None) == 1 and "C=96" in _err(lib)
    assert step(None, 2, p, p, p, p, 128, 256, p, None) == 1 and "Cl=256" in _err(lib)
    assert step(None, 2, p, p, p, p, 256, 48, p, None) == 1
    assert step(None, 2, p, p, p, None, 256, 64, p, None) == 1 and "w_lateral" in _err(lib)
    assert step(None, 2, None, p, None, None, 256, 0, p, None) == 1 and "null" in _err(lib)
    assert step(None, 2, p, p, None, None, 256, 0, None, None) == 1
    assert step(None, 2, p, p, p, p, 256, 64, p, None) == 4          # every argument is fine: there is no plan
    assert step(None, 2, p, p, None, None, 64, 0, p, None) == 4


SPECS = [("minkloc3d_cart03_b2", dict(model="MinkLoc3D"), ((32, 64, 64), (1, 1, 1), 1, 256, 0, 1)),
         ("minkloc_eca_cart03", dict(model="MinkLoc", block="ECABasicBlock"), ((32, 64, 64), (1, 1, 1), 1, 256, 1, 1)),
         ("minkloc_mac_cart03", dict(model="MinkLoc", pooling="MAC"), ((32, 64, 64), (1, 1, 1), 1, 256, 0, 2)),
         ("minkloc_spoc_cart03", dict(model="MinkLoc", block="ECABasicBlock", pooling="SPoC"), ((32, 64, 64), (1, 1, 1), 1, 256, 1, 3))]


@pytest.mark.parametrize("name,kw,spec", SPECS)
def test_spec_and_the_keys_the_finalize_asks_for(lib, name, kw, spec):
    """The specification derived from the model is the expected tuple, and the finalize finds every tensor it asks for under
    the reference's state_dict keys with the reference's shapes: with all of them registered it gets past its checks (status 0
    on a HIP device, 2 = the first allocation fails without one); with one missing or misshapen it names the key."""
    from egonn_amd import model_factory
    model = model_factory(_mp(**kw))
    assert model.minkfpn_spec() == spec and model.out_level == 2 and model.quantizer is not None
    shapes = H.state_dict_shapes(name)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == shapes
    on_gpu = torch.cuda.is_available()
    keep = {k: torch.zeros(s, dtype=torch.float32, device="cuda" if on_gpu else "cpu") + (1.0 if k.endswith("running_var") else 0.0)
            for k, s in shapes.items() if not k.endswith("num_batches_tracked")}
    planes, layers, ntd, fs, block, pooling = spec

    def finalize(drop=None, reshape=None):
        m = C.c_void_p()
        assert lib.egonn_model_create(C.byref(m)) == 0
        try:
            for k, t in keep.items():
                if k == drop:
                    continue
                shape = list(t.shape) if k != reshape else list(t.shape)[:-1] + [t.shape[-1] + 1]
                assert lib.egonn_model_set_tensor(m, k.encode(), C.c_void_p(t.data_ptr()), len(shape), (C.c_int64 * len(shape))(*shape)) == 0
            if on_gpu:
                torch.cuda.synchronize()
            rc = lib.egonn_minkfpn_finalize(m, len(planes), _ints(planes), _ints(layers), ntd, fs, block, pooling, None)
            if on_gpu:
                torch.cuda.synchronize()
            return rc, _err(lib)
        finally:
            lib.egonn_model_destroy(m)

    rc, msg = finalize()
    assert rc == (0 if on_gpu else 2), (rc, msg)
    asked = ["backbone.conv0.kernel", "backbone.bn0.bn.running_var", "backbone.convs.2.kernel", "backbone.bn.1.bn.weight",
             "backbone.blocks.1.0.conv1.kernel", "backbone.blocks.1.0.downsample.0.kernel", "backbone.blocks.1.0.downsample.1.bn.bias",
             "backbone.blocks.2.0.norm2.bn.running_mean", "backbone.conv1x1.0.kernel", "backbone.conv1x1.1.kernel",
             "backbone.tconvs.0.kernel"]
    if block == 1:
        asked.append("backbone.blocks.0.0.eca.conv.weight")
    if pooling == 1:
        asked.append("pooling.p" if kw["model"] == "MinkLoc3D" else "pooling.pooling.p")
    for key in asked:
        assert key in shapes, key
        rc, msg = finalize(drop=key)
        named = "pooling.p'" if key.endswith("pooling.p") else f"'{key}'"      # (a missing GeM exponent is named by its short key)
        assert rc == 4 and named in msg, (key, rc, msg)
    for key in ("backbone.tconvs.0.kernel", "backbone.conv1x1.1.kernel", "backbone.blocks.0.0.conv2.kernel"):
        rc, msg = finalize(reshape=key)
        assert rc == 1 and f"'{key}'" in msg and "expected" in msg, (key, rc, msg)


def _record(run):
    from egonn_amd import _lib
    fake = G.FakeLib()
    stream = _lib._stream
    _lib._stream = lambda: 0
    try:
        torch.manual_seed(0)
        run(fake)
    finally:
        _lib._stream = stream
    return fake.calls


def _global_extractor_calls(fake, **kw):
    from egonn_amd import GlobalExtractor, model_factory
    m = G._stand(model_factory(_mp(**kw)), fake, False)
    m._handle, m._sync_weights = types.SimpleNamespace(h=2), lambda: None         # the weights are not registered
    ex = GlobalExtractor(m)
    ctx = m.context()
    ctx.voxelize = lambda points, offsets, mode, step: type(ctx).voxelize(ctx, G._AsDevice(points), offsets, mode, step)
    out = ex.extract_packed(torch.zeros((G.ROWS[0], 3)), [0, G.ROWS[0] // 2, G.ROWS[0]])
    assert set(out) == {"global"} and out["global"].shape == (G.B, 256)


CALL_CASES = (("minkloc3d/extract_packed", dict(model="MinkLoc3D")),
              ("minkloc/ECABasicBlock/SPoC/extract_packed", dict(model="MinkLoc", block="ECABasicBlock", pooling="SPoC")))


def test_extract_packed_is_voxelize_plus_one_forward_call():
    """GlobalExtractor.extract_packed on MinkLoc3D: egonn_voxelize, then exactly one egonn_minkfpn_forward and no per-operator
    call; model(batch) still issues the per-operator sequence tests/golden/graph_calls.json pins."""
    with open(GOLDEN_CALLS) as f:
        golden = json.load(f)
    for case, kw in CALL_CASES:
        calls = _record(lambda fake: _global_extractor_calls(fake, **kw))
        names = [c.split("(")[0] for c in calls]
        assert names == ["egonn_voxelize", "egonn_minkfpn_forward"], names
        assert not set(names) & set(PER_OPERATOR)
        assert calls == golden[case], (calls, golden[case])
    old = _record(lambda fake: G._minkloc(fake, False, model="MinkLoc3D"))
    with open(G.GOLDEN) as f:
        assert old == json.load(f)["minkloc3d/eval"]
    assert "egonn_minkfpn_forward" not in [c.split("(")[0] for c in old] and len(old) > 20


def test_split_topdown_switch_reaches_the_flags():
    from egonn_amd import GlobalExtractor, model_factory

    def run(fake):
        m = G._stand(model_factory(_mp(model="MinkLoc3D")), fake, False)
        m._handle, m._sync_weights = types.SimpleNamespace(h=2), lambda: None
        ctx = m.context()
        ctx.batch_size = G.B
        m.split_topdown = True
        m.forward_on_plan(ctx, outputs=(torch.empty((G.B, 256)), torch.empty((G.ROWS[2], 256))))
    assert _record(run) == ["egonn_minkfpn_forward(p,p,1,p,p,-)"]


@pytest.mark.parametrize("kw", [dict(block="SEBasicBlock"), dict(pooling="netvlad", output_dim=128),
                                dict(pooling="netvladgc", output_dim=128)])
def test_models_outside_the_one_call_path_construct_and_are_refused_by_the_new_entry_points_only(kw):
    from egonn_amd import GlobalExtractor, model_factory
    m = model_factory(_mp(model="MinkLoc", **kw))
    assert len(m.state_dict()) > 0
    with pytest.raises(NotImplementedError, match="one-call"):
        GlobalExtractor(m)
    with pytest.raises(NotImplementedError, match="one-call"):
        m.minkfpn_spec()
    with pytest.raises(NotImplementedError, match="one-call"):
        m.forward_on_plan(None)
    fake_calls = _record(lambda fake: G._minkloc(fake, False, **kw))          # the eager forward still runs them
    assert len(fake_calls) > 20


def test_global_extractor_needs_a_quantizer_and_a_known_model():
    from egonn_amd import GlobalExtractor, MinkLoc3D, CartesianQuantizer
    with pytest.raises(ValueError, match="quantizer"):
        GlobalExtractor(MinkLoc3D())
    assert GlobalExtractor(MinkLoc3D(), quantizer=CartesianQuantizer(0.3)).dim == 256
    with pytest.raises(NotImplementedError):
        GlobalExtractor(torch.nn.Linear(2, 2), quantizer=CartesianQuantizer(0.3))


def test_rotation_sweep_rejects_mismatched_counts():
    from egonn_amd import evaluate_with_rotations
    scans = [np.zeros((4, 3), np.float32)] * 3
    pos = np.zeros((3, 2))
    with pytest.raises(ValueError, match="3 map scans but 2 map positions"):
        evaluate_with_rotations(None, scans, scans, pos[:2], pos, [5.0])
    with pytest.raises(ValueError, match="3 query scans but 4 query positions"):
        evaluate_with_rotations(None, scans, scans, pos, np.zeros((4, 2)), [5.0])
    with pytest.raises(ValueError, match="empty"):
        evaluate_with_rotations(None, [], scans, pos[:0], pos, [5.0])


if __name__ == "__main__":
    import sys
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    with open(GOLDEN_CALLS, "w") as f:
        json.dump({case: _record(lambda fake, kw=kw: _global_extractor_calls(fake, **kw)) for case, kw in CALL_CASES}, f, indent=0,
                  sort_keys=True)
        f.write("\n")
