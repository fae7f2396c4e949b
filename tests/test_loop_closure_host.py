"""CPU tests of the loop-closure layer: the new symbols, the argument checks of every entry point (refused on the host before
any launch, so none of this needs a device), the restatement tests/loop_closure_ref.py on hand-made curves whose counts and
scalars are written out here, and the host-side checks of LoopDetector.push and evaluate_loop_closure."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import loop_closure_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["egonn_time_windows", "egonn_knn_window_scratch_bytes", "egonn_knn_window", "egonn_window_radius",
               "egonn_pr_curve_scratch_bytes", "egonn_pr_curve"]
INVALID = 1


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_new_symbols_declared_and_exported(built):
    import egonn_amd
    from egonn_amd import _lib, loop_closure
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    declared = set(re.findall(r"\b(egonn_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for name in ("knn_window", "time_windows", "detect_loops", "LoopDetector", "evaluate_loop_closure"):
        assert getattr(egonn_amd, name) is getattr(loop_closure, name) and name in egonn_amd.__all__


def test_scratch_sizes_do_not_depend_on_the_database(built):
    """the one hard property: the windowed search's scratch is a function of (n_query, k) alone, and never a Q x M matrix"""
    from egonn_amd import _lib
    lib = _lib.load()
    f = lib.egonn_knn_window_scratch_bytes
    assert f(-1, 20) == -1 and f(1 << 31, 20) == -1 and f(16, 0) == -1 and f(16, 65) == -1 and f(16, -3) == -1
    assert f(0, 20) == 0
    for nq in (1, 16, 100, 511, 512, 20000, 1 << 20):
        for k in (1, 20, 64):
            assert 0 <= f(nq, k) <= 16 * nq * k * 8, (nq, k)         # at most 16 partial lists of (index, distance) per query
    assert f(20000, 20) < 20000 * 20000 * 4 // 1000
    g = lib.egonn_pr_curve_scratch_bytes
    assert g(-1) == -1 and g(1 << 31) == -1 and g(0) > 0 and g(4097) >= 4097 * 24 and g(4097) % 256 == 0


def test_argument_checks_need_no_gpu(built):
    """every up-front refusal returns the library's invalid status before anything is launched"""
    from egonn_amd import _lib
    lib = _lib.load()
    one, big = 256, 1 << 40      # non-null, aligned, never dereferenced: every call below fails its argument check first
    inf = math.inf

    def knn(query=one, nq=16, db=one, m=100, d=256, k=20, lo=one, hi=one, idx=one, dist=one, scratch=one, nbytes=big):
        return lib.egonn_knn_window(query, nq, db, m, d, k, lo, hi, idx, dist, scratch, nbytes, None)
    need = lib.egonn_knn_window_scratch_bytes(16, 20)
    assert need > 0
    for kw, word in ((dict(query=None), b"null"), (dict(db=None), b"null"), (dict(hi=None), b"null"), (dict(idx=None), b"null"),
                     (dict(dist=None), b"null"), (dict(k=0), b"k=0"), (dict(k=65), b"k=65"), (dict(d=0), b"d=0"),
                     (dict(d=4097), b"d=4097"), (dict(nq=-1), b"n_query=-1"), (dict(m=-1), b"n_database=-1"),
                     (dict(m=1 << 31), b"n_database"), (dict(scratch=None), b"scratch needs"),
                     (dict(nbytes=need - 1), b"scratch needs"), (dict(scratch=one + 4), b"8-byte aligned")):
        assert knn(**kw) == INVALID, kw
        assert word in lib.egonn_last_error(), (kw, lib.egonn_last_error())

    def tw(t_db=one, m=10, t_q=one, nq=4, min_gap=30.0, max_gap=inf, lo=one, hi=one, status=one):
        return lib.egonn_time_windows(t_db, m, t_q, nq, min_gap, max_gap, lo, hi, status, None)
    for kw, word in ((dict(t_db=None), b"null"), (dict(t_q=None), b"null"), (dict(lo=None), b"null"), (dict(hi=None), b"null"),
                     (dict(status=None), b"null"), (dict(m=-1), b"m=-1"), (dict(nq=-1), b"n_query=-1"),
                     (dict(min_gap=math.nan), b"NaN"), (dict(max_gap=math.nan), b"NaN")):
        assert tw(**kw) == INVALID, kw
        assert word in lib.egonn_last_error(), (kw, lib.egonn_last_error())

    def wr(qpos=one, nq=4, dbpos=one, m=10, pd=2, hi=one, pred=None, count=one, pred_dist=None):
        return lib.egonn_window_radius(qpos, nq, dbpos, m, pd, None, hi, 5.0, pred, count, pred_dist, None)
    for kw, word in ((dict(qpos=None), b"null"), (dict(dbpos=None), b"null"), (dict(hi=None), b"null"), (dict(count=None), b"null"),
                     (dict(pred=one), b"null"), (dict(pd=4), b"pd=4"), (dict(pd=1), b"pd=1"), (dict(nq=-1), b"n_query=-1"),
                     (dict(m=-1), b"m=-1")):
        assert wr(**kw) == INVALID, kw
        assert word in lib.egonn_last_error(), (kw, lib.egonn_last_error())

    def pr(score=one, correct=one, revisit=one, n=100, order=one, cum=one, end=one, totals=one, scratch=one, nbytes=big):
        return lib.egonn_pr_curve(score, correct, revisit, n, order, cum, cum, cum, end, totals, scratch, nbytes, None)
    need = lib.egonn_pr_curve_scratch_bytes(100)
    for kw, word in ((dict(score=None), b"null"), (dict(correct=None), b"null"), (dict(revisit=None), b"null"),
                     (dict(order=None), b"null"), (dict(cum=None), b"null"), (dict(end=None), b"null"), (dict(totals=None), b"null"),
                     (dict(n=-1), b"n=-1"), (dict(scratch=None), b"scratch needs"), (dict(nbytes=need - 1), b"scratch needs"),
                     (dict(scratch=one + 8), b"256-byte aligned")):
        assert pr(**kw) == INVALID, kw
        assert word in lib.egonn_last_error(), (kw, lib.egonn_last_error())


# ------------------------------------------------------------------ the restatement on hand-made curves
def _scalars(c):
    return tuple(c[name] for name in ref.SCALARS)


def test_restated_curve_all_correct():
    # four predictions, all correct, every scan a revisit: precision 1 throughout, recall 1/4 .. 1
    c = ref.curve([0.1, 0.4, 0.2, 0.3], [1, 1, 1, 1], [1, 1, 1, 1])
    assert c["thresholds"].tolist() == [np.float32(v) for v in (0.1, 0.2, 0.3, 0.4)]
    assert c["tp"].tolist() == [1, 2, 3, 4] and c["fp"].tolist() == [0, 0, 0, 0] and c["fn"].tolist() == [3, 2, 1, 0]
    assert c["precision"].tolist() == [1, 1, 1, 1] and c["recall"].tolist() == [0.25, 0.5, 0.75, 1.0]
    assert _scalars(c) == (1.0, float(np.float32(0.4)), 1.0, 1.0, 1.0)
    p = ref.pr_curve([0.1, 0.4, 0.2, 0.3], [1, 1, 1, 1], [1, 1, 1, 1])
    assert p["order"].tolist() == [0, 2, 3, 1] and p["cum_tp"].tolist() == [1, 2, 3, 4] and p["group_end"].tolist() == [1, 1, 1, 1]
    assert (p["n_predicted"], p["n_revisit"]) == (4, 4)


def test_restated_curve_none_predicted():
    c = ref.curve([np.inf, np.nan, np.inf], [0, 0, 0], [1, 0, 1])
    assert len(c["thresholds"]) == 0 and len(c["tp"]) == 0
    assert _scalars(c) == (0.0, -np.inf, 0.0, 0.0, 0.0)
    p = ref.pr_curve([np.inf, np.nan, np.inf], [0, 0, 0], [1, 0, 1])
    assert p["order"].tolist() == [0, 1, 2] and p["group_end"].tolist() == [0, 0, 0] and p["cum_tp"].tolist() == [0, 0, 0]
    assert (p["n_predicted"], p["n_revisit"]) == (0, 2)


def test_restated_curve_no_revisit():
    # three predictions, none correct, no scan is a revisit: precision 0, recall 0 by definition
    c = ref.curve([1.0, 2.0, 3.0], [0, 0, 0], [0, 0, 0])
    assert c["tp"].tolist() == [0, 0, 0] and c["fp"].tolist() == [1, 2, 3] and c["fn"].tolist() == [0, 0, 0]
    assert c["precision"].tolist() == [0, 0, 0] and c["recall"].tolist() == [0, 0, 0]
    assert _scalars(c) == (0.0, 1.0, 0.0, 0.0, 0.0)


def test_restated_curve_tie_group_straddles_correct_and_wrong():
    # scores  -2 (correct)  | 0.5, 0.5 tie: one correct, one wrong | 0.5 is written once as -0.0 + 0.5 |  9 (wrong) | inf (a missed revisit)
    score = [0.5, -2.0, 9.0, 0.5, np.inf, -0.0, 0.0]
    correct = [1, 1, 0, 0, 0, 1, 0]
    revisit = [1, 1, 0, 1, 1, 1, 0]
    c = ref.curve(score, correct, revisit)
    # thresholds -2 | 0 (the -0.0 / +0.0 group: one correct, one wrong) | 0.5 (the straddling group) | 9
    assert c["thresholds"].tolist() == [-2.0, 0.0, 0.5, 9.0]
    assert c["tp"].tolist() == [1, 2, 3, 3] and c["fp"].tolist() == [0, 1, 2, 3]
    # revisits: scans 0, 1, 3, 4, 5 (5 of them); not yet predicted ones: {0,3,4,5} | {0,3,4} | {4} | {4}
    assert c["fn"].tolist() == [4, 3, 1, 1]
    assert np.allclose(c["precision"], [1.0, 2 / 3, 3 / 5, 3 / 6], rtol=0, atol=1e-15)
    assert np.allclose(c["recall"], [1 / 5, 2 / 5, 3 / 4, 3 / 4], rtol=0, atol=1e-15)
    f1 = [2 / 6, 4 / 8, 6 / 9, 6 / 10]
    assert c["f1_max"] == pytest.approx(max(f1), abs=1e-15) and c["f1_threshold"] == 0.5
    ap = 1 / 5 * 1.0 + (2 / 5 - 1 / 5) * (2 / 3) + (3 / 4 - 2 / 5) * (3 / 5) + 0.0
    assert c["average_precision"] == pytest.approx(ap, abs=1e-15)
    assert c["recall_at_full_precision"] == pytest.approx(0.2, abs=1e-15)
    assert c["extended_precision"] == pytest.approx(0.5 * (1.0 + 0.2), abs=1e-15)
    p = ref.pr_curve(score, correct, revisit)
    assert p["order"].tolist() == [1, 5, 6, 0, 3, 2, 4]                      # equal scores in index order, no prediction last
    assert p["group_end"].tolist() == [1, 0, 1, 0, 1, 1, 0]
    assert p["cum_tp"].tolist() == [1, 2, 2, 3, 3, 3, 3] and p["cum_fp"].tolist() == [0, 0, 1, 1, 2, 3, 3]
    assert p["cum_rev"].tolist() == [1, 2, 2, 3, 4, 4, 4] and (p["n_predicted"], p["n_revisit"]) == (6, 5)


def test_restated_windows_and_knn():
    t = np.array([0.0, 1.0, 1.0, 2.0, 5.0])
    lo, hi = ref.windows(t, [1.0, 3.0, 5.0, 10.0], 1.0, 3.0)
    assert hi.tolist() == [1, 4, 4, 5] and lo.tolist() == [0, 0, 3, 5]       # t_q - min_gap itself is admissible
    assert ref.windows(t, [5.0], 1.0)[0].tolist() == [0]
    assert ref.is_sorted(t) and not ref.is_sorted([0.0, 2.0, 1.0]) and not ref.is_sorted([0.0, np.nan, 1.0])
    db = np.array([[0.0], [3.0], [3.0], [np.inf], [np.nan], [1.0]])
    idx, dist = ref.knn_window(np.array([[0.0]]), db, 6, [0], [6])
    assert idx[0].tolist() == [0, 5, 1, 2, 3, -1] and dist[0].tolist() == [0.0, 1.0, 3.0, 3.0, np.inf, np.inf]
    idx, _ = ref.knn_window(np.array([[0.0]]), db, 2, [-4], [99])
    assert idx[0].tolist() == [0, 5]
    idx, dist = ref.knn_window(np.array([[0.0]]), db, 2, [3], [2])
    assert idx[0].tolist() == [-1, -1] and np.isinf(dist).all()


def test_host_metrics_from_restated_arrays_equal_the_protocol():
    """the float64 host half of evaluate_loop_closure, fed the restated integer arrays, against the protocol stated per threshold"""
    from egonn_amd.loop_closure import curve_metrics
    rng = np.random.default_rng(2)
    for n in (0, 1, 7, 300):
        score = np.round(rng.random(n) * 16).astype(np.float32) / 4 - 1.0
        score[rng.random(n) < 0.2] = np.inf
        correct, revisit = rng.integers(0, 2, n), rng.integers(0, 2, n)
        p, want = ref.pr_curve(score, correct, revisit), ref.curve(score, correct, revisit)
        got = curve_metrics(p["cum_tp"], p["cum_fp"], p["cum_rev"], p["group_end"], p["n_revisit"])
        for name in ("tp", "fp", "fn"):
            assert np.array_equal(got[name], want[name]), (n, name)
        for name in ("precision", "recall"):
            assert np.abs(got[name] - want[name]).max(initial=0.0) <= 1e-12
        for name in ref.SCALARS:
            if name != "f1_threshold":
                assert abs(got[name] - want[name]) <= 1e-12, (n, name)
        if len(want["tp"]):
            assert want["thresholds"][got["_f1_at"]] == want["f1_threshold"]


# ------------------------------------------------------------------ the host side of the public layer
class _StubMap:
    """what LoopDetector needs of a KeypointMap, on the CPU, counting the calls that would change it"""
    n_k, dim, global_dim = 4, 4, 4

    def __init__(self):
        self.device = torch.device("cpu")
        self.adds = 0
        self._n = 0

    def __len__(self):
        return self._n

    def add(self, out, poses):
        self.adds += 1
        self._n += out["global"].shape[0]


def test_push_with_decreasing_times_raises_before_touching_the_map():
    from egonn_amd import LoopDetector
    km = _StubMap()
    det = LoopDetector(kmap=km, k=3, min_time_gap=1.0, verify=False)
    out = {"global": torch.zeros(2, 4)}
    for bad in ([5.0, 4.0], [math.nan, 1.0], [math.inf, math.inf]):
        with pytest.raises(ValueError, match="non-decreasing"):
            det.push(out, bad)
    assert km.adds == 0 and len(det) == 0
    with pytest.raises(ValueError, match="empty batch"):
        det.push({"global": torch.zeros(0, 4)}, [])
    # a detector that has seen t = 10 refuses t = 9 later on, again before the map is touched
    det2 = LoopDetector(kmap=km, k=3, min_time_gap=1.0, verify=False)
    det2._last = 10.0
    with pytest.raises(ValueError, match="non-decreasing"):
        det2.push(out, [9.0, 11.0])
    assert km.adds == 0
    for kw in (dict(k=0), dict(k=65), dict(min_time_gap=0.0), dict(min_time_gap=5.0, max_time_gap=4.0), dict(min_time_gap=math.nan)):
        with pytest.raises(ValueError):
            LoopDetector(kmap=_StubMap(), **kw)
    km3 = _StubMap()
    km3._n = 3
    with pytest.raises(ValueError, match="times"):
        LoopDetector(kmap=km3)                                   # an adopted map with entries needs their stamps


def test_evaluate_loop_closure_rejects_mismatched_lengths():
    from egonn_amd import evaluate_loop_closure
    n = 6
    nn = torch.zeros((n, 3), dtype=torch.int32)
    score, pos, w = torch.zeros(n), np.zeros((n, 2)), torch.zeros(n, dtype=torch.int32)
    for kw in (dict(score=torch.zeros(n + 1)), dict(positions=np.zeros((n - 1, 2))), dict(positions=np.zeros((n, 4))),
               dict(win_lo=w[:-1]), dict(win_hi=torch.zeros(n + 2, dtype=torch.int32)), dict(nn_index=nn[:-1]),
               dict(predicted=torch.zeros(n - 1, dtype=torch.int32)), dict(score=torch.zeros((n, 1)))):
        a = dict(nn_index=nn, score=score, positions=pos, win_lo=w, win_hi=w, revisit_radius=5.0)
        a.update(kw)
        with pytest.raises(ValueError, match="must agree in n"):
            evaluate_loop_closure(**a)
    with pytest.raises(ValueError, match="revisit_radius"):
        evaluate_loop_closure(nn, score, pos, w, w, -1.0)
