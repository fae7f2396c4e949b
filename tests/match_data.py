"""The operand sets of the mutual-matching tests, shared by tests/test_gpu_relocalize.py, tests/test_gpu_registration.py,
tests/test_registration_host.py and tests/golden/make_golden_match.py (not a test module itself).

One operator, two addressings: egonn_match_candidates reads pair p = q * k + c as (query q, map entry nn[q][c]),
egonn_match_mutual reads pair p as block p of both sides.  `index_sets()` are the sets in the indexed form, `gather_host`
turns one into the dense form, `dense_sets()` are the padded batches of the registration tests.  The results the parent of
the one-kernel refactor (commit a2c5576: reg_match_kernel, one workgroup per pair, both directions computed) gave on an
MI355X for every set are recorded in tests/golden/match_parent.npz; `check_matching` is the float64 restatement's side."""
import hashlib
import os

import numpy as np

from tests.test_registration_host import PLANTED_CASES, edge_pairs, match_band, match_f64, pad_batch, planted_case, planted_pair
from tests.test_relocalize_host import planted_case as reloc_planted_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_parent.npz")
EXCUSED_ROW_CAP = 0.01        # share of matching rows per set


def gather_host(qf, qk, qn, bf, bk, bn, nn):
    """the operands of register_pairs / match_mutual for pairs p = q * k + c, gathered on the host (invalid index: zeros, n2 = 0)"""
    Q, k = nn.shape
    M = len(bf)
    F1, K1, n1 = np.repeat(qf, k, axis=0), np.repeat(qk, k, axis=0), np.repeat(qn, k).astype(np.int32)
    F2, K2, n2 = np.zeros_like(F1), np.zeros_like(K1), np.zeros_like(n1)
    for p, idx in enumerate(nn.reshape(-1)):
        if 0 <= idx < M:
            F2[p], K2[p], n2[p] = bf[idx], bk[idx], bn[idx]
    return F1, F2, K1, K2, n1, n2


def _pad(rows, n_max):
    out = np.zeros((n_max, rows.shape[1]), np.float32)
    out[: len(rows)] = rows
    return out


def index_sets():
    """name -> (q_feat (Q, n_max, D) f32, q_n (Q,) i32, bank_feat (M, n_max, D) f32, bank_n (M,) i32, nn (Q, k) i32)"""
    full = np.full
    s = {}
    c = reloc_planted_case()
    s["planted"] = (c["q_feat"], full(6, 64), c["map_feat"], full(7, 64), c["nn"])
    # one map entry used by several queries and twice in one row
    s["planted_shared_entries"] = (c["q_feat"][:2], full(2, 64), c["map_feat"], full(7, 64), [[0, 0, 1], [0, 2, 0]])
    s["planted_q1_k1"] = (c["q_feat"][3:4], full(1, 64), c["map_feat"], full(7, 64), [[3]])
    s["planted_q5_k3"] = (c["q_feat"][:5], full(5, 64), c["map_feat"], full(7, 64),
                          [[(q + c3) % 7 for c3 in range(3)] for q in range(5)])
    # n_max = 256, D = 256 (the largest LDS tile), counts 256 / 200 (no multiple of the 64-row or the 32-column tile), both ways
    f1, f2, _, _, _ = planted_pair(256, 300, 0.5, 0.08, D=256, n2=200)
    s["largest_tile"] = (np.stack([f1, _pad(f2, 256)]), [256, 200], np.stack([_pad(f2, 256), f1]), [200, 256], [[0, 1], [1, 0]])
    rng = np.random.default_rng(5)
    qf, bf = rng.standard_normal((2, 8, 4)).astype(np.float32), rng.standard_normal((3, 8, 4)).astype(np.float32)
    s["n_max_8_dim_4"] = (qf, [8, 5], bf, [8, 3, 7], [[0, 1], [2, 1]])
    # counts 0, 1, 2, 3 on either side against everything: the "fewer than 3 mutual" branch and the empty pair
    f1, f2, _, _, _ = planted_pair(64, 900, 0.0, noise=0.0)
    qf, bf = np.stack([f1] * 5), np.stack([f2] * 5)
    s["counts_0_to_3"] = (qf, [1, 2, 3, 0, 64], bf, [64, 1, 2, 3, 0], [list(range(5))] * 5)
    s["clipped_counts"] = (qf[:2], [1000, -4], bf[:2], [64, 900], [[0, 1], [1, 0]])      # counts outside [0, n_max] are clipped
    # edge_pairs()['duplicate_descriptors'] (query rows 4..8 equal, candidate rows 19..22 equal), moved so that ties span the
    # tiles: a row tile holds 64 query rows, so copies of query row 4 are appended as rows 64..69 (row tile 1); a column tile
    # holds 32 candidate rows, so candidate rows 22 and 40 are swapped (column tiles 0 and 1)
    g1, g2, _, _, _ = edge_pairs()["duplicate_descriptors"]
    q = np.concatenate([g1, np.repeat(g1[4:5], 6, axis=0)])
    b = g2.copy()
    b[[22, 40]] = b[[40, 22]]
    assert np.array_equal(q[66], q[4]) and np.array_equal(b[40], b[19])
    s["ties_across_row_tiles"] = (_pad(q, 128)[None], [70], _pad(b, 128)[None], [64], [[0]])
    s["ties_across_column_tiles"] = (_pad(b, 128)[None], [64], _pad(q, 128)[None], [70], [[0]])   # copies in column tiles 0 and 2
    return {k: (np.ascontiguousarray(v[0], np.float32), np.asarray(v[1], np.int32), np.ascontiguousarray(v[2], np.float32),
                np.asarray(v[3], np.int32), np.asarray(v[4], np.int32)) for k, v in s.items()}


def dense_of(qf, qn, bf, bn, nn):
    """an indexed set in the dense form: (F1, F2, n1, n2)"""
    z = lambda f: np.zeros((len(f), f.shape[1], 3), np.float32)       # noqa: E731
    F1, F2, _, _, n1, n2 = gather_host(qf, z(qf), qn, bf, z(bf), bn, nn)
    return F1, F2, n1, n2


def dense_sets():
    """name -> (F1, F2, n1, n2): the padded batches of PLANTED_CASES and of edge_pairs()"""
    s = {}
    for name in PLANTED_CASES:
        F1, F2, _, _, n1, n2 = pad_batch(planted_case(name))
        s[name] = (F1, F2, n1, n2)
    F1, F2, _, _, n1, n2 = pad_batch(list(edge_pairs().values()), 128)
    s["edge_pairs"] = (F1, F2, n1, n2)
    return s


def rows_of(F1, F2, n1, n2):
    """the (f1, f2) row sets of a dense batch, counts clipped to [0, n_max] as the kernels clip them"""
    n_max = F1.shape[1]
    return [(F1[p, : np.clip(n1[p], 0, n_max)], F2[p, : np.clip(n2[p], 0, n_max)]) for p in range(len(F1))]


def input_sha256(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


_GOLDEN = {}


def recorded(name, arrays):
    """(corr, n_corr) the parent commit's egonn_match_mutual gave for set `name`; `arrays`: the regenerated inputs, which must
    hash to the recorded value"""
    if not _GOLDEN:
        with np.load(GOLDEN) as z:
            _GOLDEN.update({k: z[k] for k in z.files})
    assert input_sha256(arrays) == str(_GOLDEN[name + ".sha256"]), f"{name}: the regenerated inputs are not the recorded ones"
    corr, n_corr = _GOLDEN[name + ".corr"], _GOLDEN[name + ".n_corr"]
    assert corr.dtype == np.int32 and n_corr.dtype == np.int32
    return corr, n_corr


def check_matching(pairs, corr, n_corr):
    """-> excused rows, rows, unchecked pairs.  Rows whose best and second-best float64 squared distances lie within match_band
    may pick either; a pair is unchecked when such a row put the device and the restatement on different sides of the
    fewer-than-3 fallback (the sets then differ wholesale).  Callers assert or print the last figure: it must not hide."""
    excused = total = unchecked = 0
    for i, p in enumerate(pairs):
        want, g1, g2 = match_f64(p[0], p[1])
        band = match_band(p[0], p[1])
        # a gap of exactly 0 is a tie of duplicated descriptors: identical bits on both sides, the lowest-index rule decides
        e1, e2 = np.nonzero((g1 > 0) & (g1 < band))[0], np.nonzero((g2 > 0) & (g2 < band))[0]
        excused += len(e1) + len(e2)
        total += len(g1) + len(g2)
        got = corr[i, :n_corr[i]]
        assert (corr[i, n_corr[i]:] == -1).all()
        if len(e1) + len(e2) == 0:
            assert n_corr[i] == len(want) and np.array_equal(got, want), i
        else:       # entries that touch no excused row must agree (the < 3 fallback may flip with an excused row)
            skip = lambda c: np.isin(c[:, 0], e1) | np.isin(c[:, 1], e2)       # noqa: E731
            a, b = got[~skip(got)], want[~skip(want)]
            # all-rows output = the fewer-than-3 fallback (or every row mutual); on different sides nothing can be compared
            if (n_corr[i] == len(p[0])) != (len(want) == len(p[0])):
                unchecked += 1
            else:
                assert np.array_equal(a, b), i
                # an excused row changes at most its own entry and the entry of the row it displaces
                assert abs(int(n_corr[i]) - len(want)) <= 2 * (len(e1) + len(e2)), i
    return excused, total, unchecked
