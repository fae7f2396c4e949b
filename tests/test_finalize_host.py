"""CPU test of egonn_model_finalize's resolve pass: the finalize looks every tensor up before its first device call, so a
state_dict with one tensor missing or misshapen is refused with that key's name on a machine without a GPU (status 4 / 1), and
the complete one gets as far as the first allocation (status 2 without a HIP device, 0 with one)."""
import ctypes as C

import pytest
import torch

from tests import helpers as H

# one key of each kind the finalize asks for: conv0, a trunk BatchNorm, a strided kernel, the seven entries of a block with a
# downsample branch, a head kernel, an MLP weight
DROP, RESHAPE = "drop", "reshape"
CASES = [("trunk.convs.0.kernel", DROP),
         ("trunk.bn.3.bn.running_var", DROP),
         ("trunk.convs.4.kernel", RESHAPE),
         ("trunk.blocks.2.0.conv1.kernel", DROP),
         ("trunk.blocks.2.0.norm1.bn.weight", DROP),
         ("trunk.blocks.2.0.conv2.kernel", RESHAPE),
         ("trunk.blocks.2.0.norm2.bn.bias", DROP),
         ("trunk.blocks.2.0.downsample.0.kernel", DROP),
         ("trunk.blocks.2.0.downsample.1.bn.running_mean", RESHAPE),
         ("trunk.blocks.2.0.eca.conv.weight", DROP),
         ("global_head.tconv.6.kernel", DROP),
         ("local_descriptor_decoder.net.2.linear.weight", RESHAPE)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def tensors():
    shapes = H.state_dict_shapes()
    assert len(shapes) == 176
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    return {k: torch.zeros(s, dtype=torch.float32, device=dev) + (1.0 if k.endswith("running_var") else 0.0)
            for k, s in shapes.items() if not k.endswith("num_batches_tracked")}


def _finalize(lib, tensors, key=None, how=None):
    m = C.c_void_p()
    assert lib.egonn_model_create(C.byref(m)) == 0
    try:
        for k, t in tensors.items():
            if k == key and how == DROP:
                continue
            shape = list(t.shape)
            if k == key and how == RESHAPE:
                shape[-1] += 1
            assert lib.egonn_model_set_tensor(m, k.encode(), C.c_void_p(t.data_ptr()), len(shape), (C.c_int64 * len(shape))(*shape)) == 0
        rc = lib.egonn_model_finalize(m, None)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        return rc, lib.egonn_last_error().decode()
    finally:
        lib.egonn_model_destroy(m)


def test_complete_state_dict_passes_every_lookup(lib, tensors):
    rc, msg = _finalize(lib, tensors)
    assert rc == (0 if torch.cuda.is_available() else 2), (rc, msg)


@pytest.mark.parametrize("key,how", CASES, ids=[f"{h}-{k}" for k, h in CASES])
def test_finalize_names_the_offending_key_before_any_device_call(lib, tensors, key, how):
    assert key in tensors
    rc, msg = _finalize(lib, tensors, key, how)
    if how == DROP:
        assert rc == 4 and f"missing state_dict tensor '{key}'" in msg, (rc, msg)
    else:
        assert rc == 1 and f"tensor '{key}'" in msg and "expected" in msg, (rc, msg)
