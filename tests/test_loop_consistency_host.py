"""CPU tests of the loop-consistency filter: the new symbols and status bits, every refusal of the entry points (made on the host
before any launch, so none of this needs a device), the scratch size, the float64 restatement tests/loop_consistency_ref.py on
hand-made cases whose answers are written out here, and the argument checks of the Python surface."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import loop_consistency_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["egonn_loop_consistency_scratch_bytes", "egonn_loop_consistency", "egonn_loop_cycle_errors"]
INVALID = 1


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_new_symbols_declared_and_exported(built):
    import egonn_amd
    from egonn_amd import _lib, loop_consistency, pose_graph
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    declared = set(re.findall(r"\b(egonn_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for name in ("filter_loops", "loop_cycle_errors"):
        assert getattr(egonn_amd, name) is getattr(loop_consistency, name) and name in egonn_amd.__all__
    bits = dict(re.findall(r"EGONN_LC_STATUS_([A-Z_]+) = (\d+)", header))
    assert set(bits) == {"TRUNCATED", "ROUNDS"} and len(set(bits.values())) == 2
    for name in bits:
        assert int(bits[name]) == getattr(loop_consistency, name) == getattr(ref, name), name
    for name in ("BAD_INDEX", "SELF_LOOP", "NONFINITE", "NEGATIVE_WEIGHT"):          # the edge bits are the pose graph's
        assert getattr(ref, name) == getattr(pose_graph, name), name


def test_scratch_bytes(built):
    """a function of (E, max_partners) and of nothing else: the signature has no other argument"""
    from egonn_amd import _lib
    f = _lib.load().egonn_loop_consistency_scratch_bytes
    assert len(f.argtypes) == 2
    for bad in ((-1, 256), (1 << 30, 256), (10, 0), (10, -64), (10, 100), (10, 32), (10, 65600)):
        assert f(*bad) == -1, bad
    assert f(0, 64) > 0 and f(0, 64) % 256 == 0 and f(0, 64) == f(1, 64)
    assert f(141, 256) == f(141, 256) and f(141, 256) % 256 == 0
    for a, b in (((10, 64), (1000, 64)), ((1000, 64), (1000, 256)), ((64, 64), (65, 64)), ((20000, 256), (20001, 256))):
        assert f(*a) <= f(*b), (a, b)
    assert f(20000, 256) > f(2000, 256) and f(20000, 512) > f(20000, 256)
    # linear in E and in max_partners: rows of max_partners + 64 bits, no E x E buffer
    assert f(20000, 256) < 20000 * (5 * 8 + 24) + (1 << 20)


def test_argument_checks_need_no_gpu(built):
    """every up-front refusal returns the library's invalid status before anything is launched"""
    from egonn_amd import _lib
    lib = _lib.load()
    one, big = 256, 1 << 40      # non-null, aligned, never dereferenced: every call below fails its argument check first
    nan, inf = math.nan, math.inf
    need = lib.egonn_loop_consistency_scratch_bytes(12, 128)

    def filt(poses=one, n=10, ei=one, Z=one, w=one, E=12, window=16, tt=1.0, rt=0.1, td=0.0, rd=0.0, ms=2, mr=16, mp=128, keep=one,
             s0=one, s1=one, wo=one, rounds=one, est=one, gst=one, scratch=one, nbytes=big):
        return lib.egonn_loop_consistency(poses, n, ei, Z, w, E, window, tt, rt, td, rd, ms, mr, mp, keep, s0, s1, wo, rounds, est, gst,
                                          scratch, nbytes, None)
    cases = [(dict(**{k: None}), b"null") for k in ("poses", "ei", "Z", "w", "keep", "s0", "s1", "wo", "rounds", "est", "gst")]
    cases += [(dict(**{k: one + 4}), b"misaligned") for k in ("poses", "Z", "w", "wo")]
    cases += [(dict(**{k: one + 2}), b"misaligned") for k in ("ei", "s0", "s1", "rounds", "est", "gst")]
    cases += [(dict(n=0), b"n=0"), (dict(n=-3), b"n=-3"), (dict(n=(1 << 31) - 1), b"n="), (dict(E=-1), b"E=-1"), (dict(E=1 << 30), b"E="),
              (dict(window=-1), b"window=-1"),
              (dict(tt=-1.0), b"threshold"), (dict(tt=nan), b"threshold"), (dict(tt=inf), b"threshold"),
              (dict(rt=-1e-3), b"threshold"), (dict(rt=nan), b"threshold"), (dict(rt=inf), b"threshold"),
              (dict(td=-1.0), b"threshold"), (dict(td=nan), b"threshold"), (dict(td=inf), b"threshold"),
              (dict(rd=-1.0), b"threshold"), (dict(rd=nan), b"threshold"), (dict(rd=inf), b"threshold"),
              (dict(ms=0), b"min_support=0"), (dict(ms=-2), b"min_support=-2"), (dict(mr=0), b"max_rounds=0"), (dict(mr=-1), b"max_rounds=-1"),
              (dict(mp=0), b"max_partners=0"), (dict(mp=-64), b"max_partners=-64"), (dict(mp=100), b"max_partners=100"),
              (dict(mp=32), b"max_partners=32"),
              (dict(scratch=None), b"scratch needs"), (dict(nbytes=need - 1), b"scratch needs"), (dict(scratch=one + 8), b"256-byte aligned"),
              (dict(E=4000, nbytes=need), b"scratch needs"), (dict(E=200, mp=1024, nbytes=lib.egonn_loop_consistency_scratch_bytes(200, 128)), b"scratch needs")]
    for kw, word in cases:
        assert filt(**kw) == INVALID, kw
        assert word in lib.egonn_last_error(), (kw, lib.egonn_last_error())

    def cyc(poses=one, n=10, ei=one, Z=one, E=12, pairs=one, P=3, out=one):
        return lib.egonn_loop_cycle_errors(poses, n, ei, Z, E, pairs, P, out, None)
    for kw, word in ((dict(poses=None), b"null"), (dict(ei=None), b"null"), (dict(Z=None), b"null"), (dict(pairs=None), b"null"),
                     (dict(out=None), b"null"), (dict(n=0), b"n=0"), (dict(E=-1), b"E=-1"), (dict(P=-1), b"P=-1"), (dict(P=1 << 30), b"P="),
                     (dict(poses=one + 4), b"misaligned"), (dict(Z=one + 4), b"misaligned"), (dict(out=one + 4), b"misaligned"),
                     (dict(ei=one + 2), b"misaligned"), (dict(pairs=one + 2), b"misaligned")):
        assert cyc(**kw) == INVALID, kw
        assert word in lib.egonn_last_error(), (kw, lib.egonn_last_error())


# ------------------------------------------------------------------ the restatement on hand-made cases
def _rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _line(n=10):
    """poses that turn by 0.3 rad about z and advance 2 m along their own x per step"""
    step = np.eye(4)
    step[:3, :3], step[:3, 3] = _rot_z(0.3), [2.0, 0.0, 0.0]
    X = [np.eye(4)]
    for _ in range(n - 1):
        X.append(X[-1] @ step)
    return np.stack(X)


def _exact(X, a, b):
    return np.linalg.inv(X[a]) @ X[b]


def test_restated_exact_loops_and_a_known_offset():
    """Two exact loops one step apart: the cycle is the identity and each is the other's only support.  A third edge whose Z is
    the exact one times a pure translation by (1, 2, 2): conjugating a translation keeps its length, so c_trans = 3 against each
    of the two, in either role, and c_rot = 0."""
    X = _line()
    ei = np.array([[0, 5], [1, 6], [2, 7]], np.int32)
    D = np.eye(4)
    D[:3, 3] = [1.0, 2.0, 2.0]
    Z = np.stack([_exact(X, 0, 5), _exact(X, 1, 6), _exact(X, 2, 7) @ D])
    w = np.ones((3, 2))
    t, r = ref.cycle(X, ei, Z, 0, 1)
    assert t <= 1e-13 and r <= 1e-13
    for e, f in ((0, 2), (1, 2), (2, 0), (2, 1)):
        t, r = ref.cycle(X, ei, Z, e, f)
        assert abs(t - 3.0) <= 1e-12 and r <= 1e-13, (e, f, t, r)
    assert ref.first_of(ei, 2, 0) == (0, 2) and ref.first_of(ei, 1, 2) == (1, 2)
    errs = ref.cycle_errors(X, ei, Z, [[0, 1], [1, 0], [2, 1], [0, 3], [-1, 0]])
    assert np.array_equal(errs[0], errs[1]) and abs(errs[2, 0] - 3.0) <= 1e-12 and np.isnan(errs[3:]).all()
    got = ref.filter_loops(X, ei, Z, w, window=2, trans_thr=1.0, rot_thr=0.1, min_support=1)
    assert got["adj"].tolist() == [[False, True, False], [True, False, False], [False, False, False]]
    assert got["comparable"].sum() == 6 and got["support0"].tolist() == [1, 1, 0]
    assert got["keep"].tolist() == [True, True, False] and got["support"].tolist() == [1, 1, 0] and got["rounds"] == 1
    assert got["weights"].tolist() == [[1.0, 1.0], [1.0, 1.0], [0.0, 0.0]] and got["flags"] == 0
    assert abs(got["margin"] - 1.0) <= 1e-12          # the exact pair sits at 0, a whole threshold away; the others at 3 against 1
    # window 1: edges 0 and 2 are two steps apart and no longer comparable
    assert ref.relation(X, ei, Z, w, window=1)["comparable"].sum() == 4
    # a dead edge does not vote: with edge 1 switched off, edge 0 has nobody
    w0 = w.copy()
    w0[1] = 0.0
    dead = ref.filter_loops(X, ei, Z, w0, window=2, min_support=1)
    assert dead["support0"].tolist() == [0, 0, 0] and not dead["keep"].any() and dead["live"].tolist() == [True, False, True]
    # duplicates count each other: the offset edge reported twice survives min_support = 1 and falls at 2
    ei2, Z2 = np.concatenate([ei, ei[2:]]), np.concatenate([Z, Z[2:]])
    dup = ref.filter_loops(X, ei2, Z2, np.ones((4, 2)), window=2, min_support=1)
    assert dup["keep"].tolist() == [True, True, True, True] and dup["support0"].tolist() == [1, 1, 1, 1]
    dup2 = ref.filter_loops(X, ei2, Z2, np.ones((4, 2)), window=2, min_support=2)
    assert not dup2["keep"].any() and dup2["rounds"] == 1


def test_restated_status_bits_and_the_position_cap():
    X = _line()
    X[9, 0, 3] = np.nan
    ei = np.array([[0, 5], [-1, 5], [3, 3], [1, 6], [2, 9], [1, 7], [2, 8]], np.int32)
    Z = np.stack([np.eye(4)] * 7)
    Z[3, 1, 1] = np.inf
    w = np.ones((7, 2))
    w[5] = [1.0, -1.0]
    w[6] = 0.0
    st, live = ref.edge_status(X, ei, Z, w)
    assert st.tolist() == [0, ref.BAD_INDEX, ref.SELF_LOOP, ref.NONFINITE, ref.NONFINITE, ref.NEGATIVE_WEIGHT, 0]
    assert live.tolist() == [True] + [False] * 6
    # five live edges on consecutive b with a cap of one place either side (max_partners = 2 is below the library's 64: the
    # restatement takes any even number)
    X = _line()
    ei = np.array([[k, k + 4] for k in range(5)], np.int32)
    Z = np.stack([_exact(X, a, b) for a, b in ei])
    full = ref.relation(X, ei, Z, np.ones((5, 2)), window=2)
    assert not full["truncated"] and full["adj"].sum(axis=1).tolist() == [2, 3, 4, 3, 2]
    capped = ref.relation(X, ei, Z, np.ones((5, 2)), window=2, max_partners=2)
    assert capped["truncated"] and capped["adj"].sum(axis=1).tolist() == [1, 2, 2, 2, 1]
    assert np.array_equal(capped["adj"], capped["adj"].T)


def test_restated_synchronous_rounds_on_a_path():
    """The path 0 - 1 - 2 - 3 - 4 with min_support = 2.  Round 1: the ends have one partner and leave.  Round 2: 1 and 3 have
    lost a partner each and leave.  Round 3: 2 has nobody.  Removing one at a time in index order would give the same empty
    end, but after two rounds the synchronous rule holds exactly {2}."""
    adj = np.zeros((5, 5), bool)
    for k in range(4):
        adj[k, k + 1] = adj[k + 1, k] = True
    live = np.ones(5, bool)
    full = ref.select(adj, live, min_support=2, max_rounds=16)
    assert full["support0"].tolist() == [1, 2, 2, 2, 1] and not full["keep"].any() and full["rounds"] == 3 and not full["hit_limit"]
    assert full["support"].tolist() == [0] * 5
    three = ref.select(adj, live, min_support=2, max_rounds=3)
    assert not three["keep"].any() and three["rounds"] == 3 and three["hit_limit"]       # the last round still removed something
    two = ref.select(adj, live, min_support=2, max_rounds=2)
    assert two["keep"].tolist() == [False, False, True, False, False] and two["rounds"] == 2 and two["hit_limit"]
    assert two["support"].tolist() == [0] * 5
    one = ref.select(adj, live, min_support=2, max_rounds=1)
    assert one["keep"].tolist() == [False, True, True, True, False] and one["support"].tolist() == [0, 1, 2, 1, 0]
    easy = ref.select(adj, live, min_support=1)
    assert easy["keep"].all() and easy["rounds"] == 0 and not easy["hit_limit"] and easy["support"].tolist() == [1, 2, 2, 2, 1]
    # a dead edge in the middle cuts the path: it never votes
    cut = ref.select(adj, np.array([True, True, False, True, True]), min_support=1)
    assert cut["support0"].tolist() == [1, 1, 0, 1, 1] and cut["keep"].tolist() == [True, True, False, True, True]


def test_filter_loops_checks_its_arguments():
    """shape and value checks come before anything that needs a device"""
    import egonn_amd
    X = torch.from_numpy(_line())
    loops = {"edge_index": torch.tensor([[0, 5], [1, 6]], dtype=torch.int32), "Z": torch.eye(4, dtype=torch.float64).repeat(2, 1, 1),
             "weights": torch.ones((2, 2), dtype=torch.float64)}
    f = egonn_amd.filter_loops
    for kw, word in ((dict(window=-1), "window"), (dict(trans_thr=-1.0), "trans_thr"), (dict(trans_thr=math.nan), "trans_thr"),
                     (dict(rot_thr=math.inf), "rot_thr"), (dict(trans_drift=-0.1), "trans_drift"), (dict(rot_drift=math.nan), "rot_drift"),
                     (dict(min_support=0), "min_support"), (dict(max_rounds=0), "max_rounds"), (dict(max_partners=0), "max_partners"),
                     (dict(max_partners=96), "max_partners"), (dict(max_partners=-64), "max_partners")):
        with pytest.raises(ValueError, match=word):
            f(X, loops, **kw)
    with pytest.raises(ValueError, match="poses"):
        f(X[:, :3], loops)
    with pytest.raises(ValueError, match="weights"):
        f(X, dict(loops, weights=torch.ones(2)))
    with pytest.raises(ValueError, match="Z"):
        f(X, dict(loops, Z=loops["Z"][:1]))
    with pytest.raises(ValueError, match="loop_edges"):
        f(X, {"edge_index": loops["edge_index"], "Z": loops["Z"]})
    with pytest.raises(ValueError, match="pairs"):
        egonn_amd.loop_cycle_errors(X, loops, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="edge_index"):
        egonn_amd.loop_cycle_errors(X, dict(loops, edge_index=torch.zeros(2, dtype=torch.int32)), torch.zeros((1, 2), dtype=torch.int32))
