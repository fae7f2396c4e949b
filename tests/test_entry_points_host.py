"""Argument checks of the context-free operator entry points, without a GPU: every case is one valid-looking argument set broken
in one place, and the library must answer with the recorded status and message before it touches a device.

EXPECTED was recorded from the library as it stood before the entry points moved out of model.hip into the files that hold their
kernels (`python tests/test_entry_points_host.py [path/to/libegonn_hip.so]` prints the table of the library it is given); a change
of an entry point keeps it unless it means to change the C ABI's behaviour.  A case whose broken argument is not caught by a
check reaches a HIP call (status 2 on a machine without a device) and has no row here.  The rows of egonn_debug_radix_sort were
recorded when that hook was added.  Its check of the segmented pass count (8 at most) has no row: nbits <= 64 is checked first and
64 bits are 8 passes of 9, so no argument set reaches it.

The borrowed (non-owning) Arena that the ICP entry points sort on is a host-side object: tests/arena_view_main.cpp is a program
of its own that this file compiles for the host and runs."""
import ctypes as C
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 256                      # non-null, 256-byte aligned, never dereferenced: every call below fails a check first
PARAMS = (C.c_float * 6)(1.0, 1.0, 1.0, 1.0, 1.0, 0.5)


def _base(lib):
    """entry point -> one valid-looking argument list (in the order of include/egonn_hip.h)"""
    return {
        "egonn_triplet_loss": [P, 8, 16, P, P, 0.2, P, P, None, P, None],
        "egonn_contrastive_loss": [P, 8, 16, P, P, 0.2, 0.5, P, P, None, P, None],
        "egonn_nn_search": [P, 10, None, P, 10, P, P, None],
        "egonn_matrix_min": [P, 4, 4, P, P, P, P, None],
        "egonn_softmax_cross_entropy": [P, 4, 4, P, P, P, None, None],
        # pairs, n_cloud1, n_cloud2, n_kp1, n_kp2, dim | 13 inputs | params | out_pair, out_batch, 6 gradients, scratch | bytes
        "egonn_local_loss": [2, 100, 100, 10, 10, 128] + [P] * 13 + [PARAMS] + [P, P] + [None] * 6 + [P] +
                            [lib.egonn_local_loss_scratch_bytes(2, 10, 10, 128), None],
        "egonn_dense_backward_weight": [P, 32, P, 32, 10, P, P, 1 << 20, None],
        "egonn_col_stats": [0, P, None, None, None, 100, 32, P, P, 1 << 20, None],
        "egonn_bn_train_finalize": [P, P, 10.0, 32, P, P, 1e-5, 0.1, P, P, P, None],
        "egonn_bn_backward_finalize": [P, P, 10.0, 32, P, P, P, P, None],
        "egonn_affine_act": [P, P, P, 10, 32, 1, P, None],
        "egonn_affine3": [P, None, P, P, P, P, 10, 32, P, None],
        "egonn_relu_backward": [P, P, 10, 32, P, None],
        "egonn_eca_gate": [P, P, 3, 2, 32, P, None],
        "egonn_eca_gate_backward": [P, P, P, P, 3, 2, 32, P, P, None],
        "egonn_se_gate": [P] * 5 + [2, 32, 2, P, None, None],
        "egonn_se_gate_backward": [P] * 6 + [2, 32, 2] + [P] * 5 + [None],
        "egonn_act_backward": [1, P, P, 10, 32, P, None],
        "egonn_l2_normalize": [P, None, 10, 32, P, None],
        "egonn_sigmoid_gate": [P, P, None, 10, P, None, None, None],
        "egonn_knn": [P, 4, P, 10, 256, 2, P, P, P, 40, None],
        "egonn_recall_counts": [P, P, P, 4, 2, 2, P, 3, P, None],
        "egonn_filter_points": [P, 5000, 4, P, 2, 1, 1, -1.0, P, P, P, lib.egonn_filter_points_scratch_ints(5000), None],
        "egonn_voxel_downsample": [P, 10, P, 1, 0.1, None, P, P, P, P, P, lib.egonn_voxel_downsample_scratch_bytes(10, 1), None],
        "egonn_icp_pairs": [P, 10, P, P, 10, P, 1, None, 1.2, 200, 1e-6, 1e-6] + [P] * 5 + [None] * 3 +
                           [P, lib.egonn_icp_scratch_bytes(10, 10, 1), None],
        # keys_in, vals_in, keys_out, vals_out, n, nbits, n_dev, seg_offsets, n_segments, idx_bits, either_pair, result_pair | scratch
        "egonn_debug_radix_sort": [P, P, P, P, 100, 16, None, None, 0, 0, 0, C.pointer(C.c_int32(-1)), P,
                                   lib.egonn_debug_radix_sort_scratch_bytes(100, 0), None],
    }


# (entry point, what is broken, {argument index: value}); LESS as the value of a size argument = one less than the base's.
# The last two: the ICP entry points sort on a borrowed span of the caller's scratch, so one byte less than
# egonn_*_scratch_bytes reports must be refused up front (tests/test_icp_host.py covers a scratch of 8 bytes).
LESS = "one less"
SEG = {7: P, 8: 2, 13: 1 << 20}
CASES = [
    ("egonn_triplet_loss", "null embeddings", {0: None}),
    ("egonn_triplet_loss", "null scratch", {9: None}),
    ("egonn_triplet_loss", "n = 0", {1: 0}),
    ("egonn_triplet_loss", "d = 0", {2: 0}),
    ("egonn_contrastive_loss", "null embeddings", {0: None}),
    ("egonn_contrastive_loss", "null scratch", {10: None}),
    ("egonn_contrastive_loss", "d = 0", {2: 0}),
    ("egonn_nn_search", "null a", {0: None}),
    ("egonn_nn_search", "m = 0", {4: 0}),
    ("egonn_nn_search", "n = 2^31", {1: 1 << 31}),
    ("egonn_matrix_min", "null d", {0: None}),
    ("egonn_matrix_min", "n = 0", {1: 0}),
    ("egonn_softmax_cross_entropy", "null target", {3: None}),
    ("egonn_softmax_cross_entropy", "m = 0", {2: 0}),
    ("egonn_local_loss", "pairs = 0", {0: 0}),
    ("egonn_local_loss", "dim = 64", {5: 64}),
    ("egonn_local_loss", "n_kp1 = 2^31 / 128", {3: (1 << 31) // 128}),
    ("egonn_local_loss", "null clouds1", {6: None}),
    ("egonn_local_loss", "one gradient of six", {22: P}),
    ("egonn_local_loss", "misaligned scratch", {28: P + 8}),
    ("egonn_local_loss", "scratch too small", {29: LESS}),
    ("egonn_dense_backward_weight", "null a", {0: None}),
    ("egonn_dense_backward_weight", "ca = 0", {1: 0}),
    ("egonn_dense_backward_weight", "scratch too small", {7: 8}),
    ("egonn_col_stats", "null a", {1: None}),
    ("egonn_col_stats", "mode = 4", {0: 4}),
    ("egonn_col_stats", "c = 0", {6: 0}),
    ("egonn_col_stats", "c = 257", {6: 257}),
    ("egonn_col_stats", "misaligned scratch", {8: P + 4}),
    ("egonn_col_stats", "scratch too small", {9: 8}),
    ("egonn_bn_train_finalize", "null sums", {0: None}),
    ("egonn_bn_train_finalize", "c = 0", {3: 0}),
    ("egonn_bn_train_finalize", "count = 0", {2: 0.0}),
    ("egonn_bn_backward_finalize", "null local sums", {0: None}),
    ("egonn_bn_backward_finalize", "count = 0.5", {2: 0.5}),
    ("egonn_affine_act", "null x", {0: None}),
    ("egonn_affine3", "null g", {0: None}),
    ("egonn_relu_backward", "null grad_out", {0: None}),
    ("egonn_eca_gate", "null mean", {0: None}),
    ("egonn_eca_gate", "channels = 0", {4: 0}),
    ("egonn_eca_gate", "even kernel size", {2: 4}),
    ("egonn_eca_gate_backward", "null grad_gate", {0: None}),
    ("egonn_eca_gate_backward", "channels = 0", {6: 0}),
    ("egonn_se_gate", "null mean", {0: None}),
    ("egonn_se_gate", "channels = 0", {6: 0}),
    ("egonn_se_gate", "hidden = 3", {7: 3}),
    ("egonn_se_gate_backward", "null grad_gate", {0: None}),
    ("egonn_se_gate_backward", "channels = 0", {7: 0}),
    ("egonn_act_backward", "act = 5", {0: 5}),
    ("egonn_act_backward", "null grad_out", {1: None}),
    ("egonn_l2_normalize", "null x", {0: None}),
    ("egonn_l2_normalize", "c = 0", {3: 0}),
    ("egonn_sigmoid_gate", "null y", {0: None}),
    ("egonn_sigmoid_gate", "null out", {4: None}),
    ("egonn_sigmoid_gate", "n = -1", {3: -1}),
    ("egonn_knn", "null query", {0: None}),
    ("egonn_knn", "n_query = 2^31", {1: 1 << 31}),
    ("egonn_knn", "dim = 0", {4: 0}),
    ("egonn_knn", "null scratch", {8: None}),
    ("egonn_knn", "scratch too small", {9: LESS}),
    ("egonn_recall_counts", "null radius", {6: None}),
    ("egonn_recall_counts", "null nn_index", {0: None}),
    ("egonn_recall_counts", "k = 0", {4: 0}),
    ("egonn_filter_points", "null raw", {0: None}),
    ("egonn_filter_points", "floats_per_point = 5", {2: 5}),
    ("egonn_filter_points", "n = 2^31", {1: 1 << 31}),
    ("egonn_filter_points", "null scratch", {10: None}),
    ("egonn_filter_points", "scratch too small", {11: LESS}),
    ("egonn_voxel_downsample", "scratch one byte short", {11: LESS}),
    ("egonn_icp_pairs", "scratch one byte short", {21: LESS}),
    # the sort hook: flat without seg_offsets; SEG turns the base into a segmented call of two segments with scratch to spare
    ("egonn_debug_radix_sort", "null keys_in", {0: None}),
    ("egonn_debug_radix_sort", "null vals_out", {3: None}),
    ("egonn_debug_radix_sort", "null result_pair", {11: None}),
    ("egonn_debug_radix_sort", "null scratch", {12: None}),
    ("egonn_debug_radix_sort", "n = -1", {4: -1}),
    ("egonn_debug_radix_sort", "n = 2^31", {4: 1 << 31}),
    ("egonn_debug_radix_sort", "nbits = 0", {5: 0}),
    ("egonn_debug_radix_sort", "nbits = 65", {5: 65}),
    ("egonn_debug_radix_sort", "idx_bits without offsets", {9: 16}),
    ("egonn_debug_radix_sort", "segments without offsets", {8: 2}),
    ("egonn_debug_radix_sort", "nbits + idx_bits = 65", {**SEG, 5: 37, 9: 28}),
    ("egonn_debug_radix_sort", "idx_bits = -1", {**SEG, 9: -1}),
    ("egonn_debug_radix_sort", "n_segments = 0", {**SEG, 8: 0}),
    ("egonn_debug_radix_sort", "n_segments = 4097", {**SEG, 8: 4097}),
    ("egonn_debug_radix_sort", "n_dev with segments", {**SEG, 6: P}),
    ("egonn_debug_radix_sort", "misaligned scratch", {12: P + 8}),
    ("egonn_debug_radix_sort", "scratch one byte short", {13: LESS}),
    ("egonn_debug_radix_sort", "segmented scratch one byte short", {**SEG, 13: 40447}),
]

# (status, egonn_last_error()) of every case above
EXPECTED = {
    ('egonn_triplet_loss', 'null embeddings'): (1, 'triplet_loss: null argument'),
    ('egonn_triplet_loss', 'null scratch'): (1, 'triplet_loss: null argument'),
    ('egonn_triplet_loss', 'n = 0'): (1, 'triplet loss: n=0 d=16 out of range'),
    ('egonn_triplet_loss', 'd = 0'): (1, 'triplet loss: n=8 d=0 out of range'),
    ('egonn_contrastive_loss', 'null embeddings'): (1, 'contrastive_loss: null argument'),
    ('egonn_contrastive_loss', 'null scratch'): (1, 'contrastive_loss: null argument'),
    ('egonn_contrastive_loss', 'd = 0'): (1, 'contrastive loss: n=8 d=0 out of range'),
    ('egonn_nn_search', 'null a'): (1, 'nn_search: null argument'),
    ('egonn_nn_search', 'm = 0'): (1, 'nn_search: bad sizes'),
    ('egonn_nn_search', 'n = 2^31'): (1, 'nn_search: bad sizes'),
    ('egonn_matrix_min', 'null d'): (1, 'matrix_min: null argument'),
    ('egonn_matrix_min', 'n = 0'): (1, 'matrix_min: bad sizes'),
    ('egonn_softmax_cross_entropy', 'null target'): (1, 'softmax_cross_entropy: null argument'),
    ('egonn_softmax_cross_entropy', 'm = 0'): (1, 'softmax_ce: bad sizes'),
    ('egonn_local_loss', 'pairs = 0'): (1, 'local_loss: pairs=0 outside [1, 4096]'),
    ('egonn_local_loss', 'dim = 64'): (1, 'local_loss: descriptor width 64 not supported (128)'),
    ('egonn_local_loss', 'n_kp1 = 2^31 / 128'): (1, 'local_loss: totals out of range (clouds 100 100, keypoints 16777216 10)'),
    ('egonn_local_loss', 'null clouds1'): (1, 'local_loss: null argument'),
    ('egonn_local_loss', 'one gradient of six'): (1, 'local_loss: the six gradient outputs are given together or not at all'),
    ('egonn_local_loss', 'misaligned scratch'): (1, 'local_loss: descriptors must be 16-byte aligned, scratch 256-byte aligned'),
    ('egonn_local_loss', 'scratch too small'): (1, 'local_loss: scratch of 3583 bytes, 3584 needed'),
    ('egonn_dense_backward_weight', 'null a'): (1, 'dense_backward_weight: bad arguments'),
    ('egonn_dense_backward_weight', 'ca = 0'): (1, 'dense_backward_weight: bad arguments'),
    ('egonn_dense_backward_weight', 'scratch too small'): (1, 'wgrad: scratch of 8 floats is smaller than one kernel (1024)'),
    ('egonn_col_stats', 'null a'): (1, 'col_stats: bad arguments'),
    ('egonn_col_stats', 'mode = 4'): (1, 'col_stats: bad arguments'),
    ('egonn_col_stats', 'c = 0'): (1, 'col_stats: 0 channels unsupported (1..256)'),
    ('egonn_col_stats', 'c = 257'): (1, 'col_stats: 257 channels unsupported (1..256)'),
    ('egonn_col_stats', 'misaligned scratch'): (1, 'col_stats: out and scratch hold doubles (8-byte alignment)'),
    ('egonn_col_stats', 'scratch too small'): (1, 'col_stats: scratch too small (8 < 128 floats)'),
    ('egonn_bn_train_finalize', 'null sums'): (1, 'bn_train_finalize: bad arguments'),
    ('egonn_bn_train_finalize', 'c = 0'): (1, 'bn_train_finalize: bad arguments'),
    ('egonn_bn_train_finalize', 'count = 0'): (1, 'bn_train_finalize: bad arguments'),
    ('egonn_bn_backward_finalize', 'null local sums'): (1, 'bn_backward_finalize: bad arguments'),
    ('egonn_bn_backward_finalize', 'count = 0.5'): (1, 'bn_backward_finalize: bad arguments'),
    ('egonn_affine_act', 'null x'): (1, 'affine_act: null argument'),
    ('egonn_affine3', 'null g'): (1, 'affine3: null argument'),
    ('egonn_relu_backward', 'null grad_out'): (1, 'relu_backward: null argument'),
    ('egonn_eca_gate', 'null mean'): (1, 'eca_gate: null argument'),
    ('egonn_eca_gate', 'channels = 0'): (1, 'eca_gate: bad shape'),
    ('egonn_eca_gate', 'even kernel size'): (1, 'eca_gate: bad shape'),
    ('egonn_eca_gate_backward', 'null grad_gate'): (1, 'eca_gate_backward: null argument'),
    ('egonn_eca_gate_backward', 'channels = 0'): (1, 'eca_gate: bad shape'),
    ('egonn_se_gate', 'null mean'): (1, 'se_gate: null argument'),
    ('egonn_se_gate', 'channels = 0'): (1, 'se_gate: B=2 channels=0 hidden=2 unsupported (channels a multiple of 16 in 16..256, hidden = channels/16)'),
    ('egonn_se_gate', 'hidden = 3'): (1, 'se_gate: B=2 channels=32 hidden=3 unsupported (channels a multiple of 16 in 16..256, hidden = channels/16)'),
    ('egonn_se_gate_backward', 'null grad_gate'): (1, 'se_gate_backward: null argument'),
    ('egonn_se_gate_backward', 'channels = 0'): (1, 'se_gate: B=2 channels=0 hidden=2 unsupported (channels a multiple of 16 in 16..256, hidden = channels/16)'),
    ('egonn_act_backward', 'act = 5'): (1, 'act_backward: bad arguments'),
    ('egonn_act_backward', 'null grad_out'): (1, 'act_backward: bad arguments'),
    ('egonn_l2_normalize', 'null x'): (1, 'l2_normalize: bad arguments'),
    ('egonn_l2_normalize', 'c = 0'): (1, 'l2_normalize: bad arguments'),
    ('egonn_sigmoid_gate', 'null y'): (1, 'sigmoid_gate: bad argument'),
    ('egonn_sigmoid_gate', 'null out'): (1, 'sigmoid_gate: bad argument'),
    ('egonn_sigmoid_gate', 'n = -1'): (1, 'sigmoid_gate: bad argument'),
    ('egonn_knn', 'null query'): (1, 'knn: bad arguments (nq=4 m=10 d=256 k=2)'),
    ('egonn_knn', 'n_query = 2^31'): (1, 'knn: too many rows'),
    ('egonn_knn', 'dim = 0'): (1, 'knn: bad arguments (nq=4 m=10 d=0 k=2)'),
    ('egonn_knn', 'null scratch'): (1, 'knn: scratch needs 40 floats'),
    ('egonn_knn', 'scratch too small'): (1, 'knn: scratch needs 40 floats'),
    ('egonn_recall_counts', 'null radius'): (1, 'recall: bad arguments'),
    ('egonn_recall_counts', 'null nn_index'): (1, 'recall: bad arguments'),
    ('egonn_recall_counts', 'k = 0'): (1, 'recall: bad arguments'),
    ('egonn_filter_points', 'null raw'): (1, 'ingest: bad arguments (n=5000 stride=4)'),
    ('egonn_filter_points', 'floats_per_point = 5'): (1, 'ingest: bad arguments (n=5000 stride=5)'),
    ('egonn_filter_points', 'n = 2^31'): (1, 'ingest: bad arguments (n=2147483648 stride=4)'),
    ('egonn_filter_points', 'null scratch'): (1, 'ingest: bad arguments (n=5000 stride=4)'),
    ('egonn_filter_points', 'scratch too small'): (1, 'ingest: scratch too small'),
    ('egonn_voxel_downsample', 'scratch one byte short'): (1, 'voxel_downsample: scratch needs 23552 bytes, 256-byte aligned'),
    ('egonn_icp_pairs', 'scratch one byte short'): (1, 'icp_pairs: scratch needs 25344 bytes, 256-byte aligned'),
    ('egonn_debug_radix_sort', 'null keys_in'): (1, 'debug_radix_sort: null pointer'),
    ('egonn_debug_radix_sort', 'null vals_out'): (1, 'debug_radix_sort: null pointer'),
    ('egonn_debug_radix_sort', 'null result_pair'): (1, 'debug_radix_sort: null pointer'),
    ('egonn_debug_radix_sort', 'null scratch'): (1, 'debug_radix_sort: null pointer'),
    ('egonn_debug_radix_sort', 'n = -1'): (1, 'debug_radix_sort: n=-1 outside [0, 2^31)'),
    ('egonn_debug_radix_sort', 'n = 2^31'): (1, 'debug_radix_sort: n=2147483648 outside [0, 2^31)'),
    ('egonn_debug_radix_sort', 'nbits = 0'): (1, 'debug_radix_sort: nbits=0 outside [1, 64]'),
    ('egonn_debug_radix_sort', 'nbits = 65'): (1, 'debug_radix_sort: nbits=65 outside [1, 64]'),
    ('egonn_debug_radix_sort', 'idx_bits without offsets'): (1, 'debug_radix_sort: n_segments=0 idx_bits=16 without seg_offsets (the flat sort takes neither)'),
    ('egonn_debug_radix_sort', 'segments without offsets'): (1, 'debug_radix_sort: n_segments=2 idx_bits=0 without seg_offsets (the flat sort takes neither)'),
    ('egonn_debug_radix_sort', 'nbits + idx_bits = 65'): (1, 'debug_radix_sort: nbits=37 + idx_bits=28 outside [nbits, 64]'),
    ('egonn_debug_radix_sort', 'idx_bits = -1'): (1, 'debug_radix_sort: nbits=16 + idx_bits=-1 outside [nbits, 64]'),
    ('egonn_debug_radix_sort', 'n_segments = 0'): (1, 'debug_radix_sort: n_segments=0 outside [1, 4096]'),
    ('egonn_debug_radix_sort', 'n_segments = 4097'): (1, 'debug_radix_sort: n_segments=4097 outside [1, 4096]'),
    ('egonn_debug_radix_sort', 'n_dev with segments'): (1, 'debug_radix_sort: the segmented sort takes no n_dev'),
    ('egonn_debug_radix_sort', 'misaligned scratch'): (1, 'debug_radix_sort: scratch needs 18944 bytes, 256-byte aligned'),
    ('egonn_debug_radix_sort', 'scratch one byte short'): (1, 'debug_radix_sort: scratch needs 18944 bytes, 256-byte aligned'),
    ('egonn_debug_radix_sort', 'segmented scratch one byte short'): (1, 'debug_radix_sort: scratch needs 40448 bytes, 256-byte aligned'),
}


def _lib_at(path=None):
    from egonn_amd import _lib
    if path is None:
        return _lib.load()
    lib = C.CDLL(path)
    for name, res, args in _lib._SIGS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def _call(lib, base, name, patch):
    args = list(base[name])
    for i, v in patch.items():
        args[i] = args[i] - 1 if v is LESS else v
    rc = getattr(lib, name)(*args)
    return rc, (lib.egonn_last_error() or b"").decode()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib_at()


def test_every_case_has_a_recorded_answer():
    assert sorted(EXPECTED) == sorted((n, w) for n, w, _ in CASES) and len(EXPECTED) == len(CASES)
    assert all(rc != 0 and rc != 2 and msg for rc, msg in EXPECTED.values())


@pytest.mark.parametrize("name,what,patch", CASES, ids=[f"{n[6:]}-{w.replace(' ', '_')}" for n, w, _ in CASES])
def test_bad_argument_answer_is_unchanged(lib, name, what, patch):
    rc, msg = _call(lib, _base(lib), name, patch)
    want_rc, want_msg = EXPECTED[(name, what)]
    assert rc == want_rc, (rc, msg)
    assert want_msg in msg, msg


def test_borrowed_arena(tmp_path):
    """Arena::view: ensure() inside the span succeeds, beyond it is EGONN_ERR_INVALID; nothing is freed, allocated or moved"""
    import __graft_entry__ as g
    exe = str(tmp_path / "arena_view")
    subprocess.check_call([g._hipcc(), "--offload-arch=gfx950", "-O1", "-std=c++20", "-o", exe,
                           os.path.join(REPO, "tests", "arena_view_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "borrowed arena: ok" in r.stdout


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    lib_ = _lib_at(sys.argv[1] if len(sys.argv) > 1 else None)
    base_ = _base(lib_)
    for name_, what_, patch_ in CASES:
        rc_, msg_ = _call(lib_, base_, name_, patch_)
        print(f"    ({name_!r}, {what_!r}): ({rc_}, {msg_!r}),")
