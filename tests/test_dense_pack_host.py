"""Host test of the 1x1-kernel packer (egonn_dense_pack_fragments_host, egonn_amd/csrc/dense.hip): the packed buffer must equal a
numpy restatement of the fragment order the dense kernels stage into LDS (frag_of in dense_lds_kernel),
    packed[((nt * cin/16 + t) * 64 + lane) * 4 + u] = Wmat[16 t + 4 (lane >> 4) + u][16 nt + (lane & 15)],
bit for bit, for (in, out) and (out, in) kernels.  The device packer runs the same index function
(tests/test_gpu_dense_stream.py compares the two)."""
import numpy as np
import pytest


def _restate(wmat):
    """wmat (cin, cout) -> the fragment order, by the formula of the docstring"""
    cin, cout = wmat.shape
    ks = cin // 16
    out = np.empty((cout // 16, ks, 64, 4), dtype=np.float32)
    for nt in range(cout // 16):
        for t in range(ks):
            for lane in range(64):
                for u in range(4):
                    out[nt, t, lane, u] = wmat[16 * t + 4 * (lane >> 4) + u, 16 * nt + (lane & 15)]
    return out.reshape(-1)


@pytest.mark.parametrize("cin", [32, 64, 128])
@pytest.mark.parametrize("cout", [64, 128])
def test_packed_fragments_equal_the_restatement(cin, cout):
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    rng = np.random.default_rng(cin * 1000 + cout)
    wmat = (rng.permutation(cin * cout).reshape(cin, cout) - 0.5 * cin * cout).astype(np.float32)     # distinct values
    want = _restate(wmat).view(np.int32)
    assert np.array_equal(_lib.dense_pack_fragments(wmat, False).view(np.int32), want)
    assert np.array_equal(_lib.dense_pack_fragments(np.ascontiguousarray(wmat.T), True).view(np.int32), want)
    assert np.unique(want).size == cin * cout          # every element of the kernel exactly once


def test_packer_rejects_ragged_channels():
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    with pytest.raises(Exception):
        _lib.dense_pack_fragments(np.zeros((24, 64), np.float32), False)
