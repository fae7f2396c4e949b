"""CPU tests of the ScanContext baseline (egonn_amd/scan_context.py, csrc/scan_context.hip): the fixture and its shared inputs,
the argument checks that come before any device work, and the absence of a CPU path."""
import os
import re

import numpy as np
import pytest
import torch

from tests import scan_context_data as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["egonn_scan_context", "egonn_scan_context_ringkey", "egonn_scan_context_distance", "egonn_scan_context_rerank"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "scan_context.npz"))


def test_fixture_is_complete(fx):
    n = D.N_MAP + D.N_QUERY
    for R, S in D.SHAPES:
        assert fx[f"sc_{R}x{S}"].shape == (n, R, S) and fx[f"sc_{R}x{S}"].dtype == np.float32
        assert fx[f"rk_{R}x{S}"].shape == (n, R) and fx[f"rk_{R}x{S}"].dtype == np.float64
        assert fx[f"edge_sc_{R}x{S}"].shape == (3, R, S) and not fx[f"edge_sc_{R}x{S}"][1].any()
        assert fx[f"edge_dist_{R}x{S}"].shape == (3, 3) and fx[f"edge_yaw_{R}x{S}"].shape == (3, 3)
        # every distance that involves the empty scan is NaN with yaw 1
        assert np.isnan(fx[f"edge_dist_{R}x{S}"][1]).all() and np.isnan(fx[f"edge_dist_{R}x{S}"][:, 1]).all()
        assert (fx[f"edge_yaw_{R}x{S}"][1] == 1).all() and (fx[f"edge_yaw_{R}x{S}"][:, 1] == 1).all()
        assert (fx[f"sc_{R}x{S}"] >= 0).all() and not np.signbit(fx[f"sc_{R}x{S}"]).any()
    nq = len(D.manager_queries())
    for R, S in D.DIST_SHAPES:
        for key in ("dist", "yaw", "simgap"):
            assert fx[f"{key}_{R}x{S}"].shape == (D.N_QUERY, D.N_MAP)
        assert np.isfinite(fx[f"dist_{R}x{S}"]).all() and (fx[f"simgap_{R}x{S}"] > 4e-5).all()    # no pair is left out of the yaw check
        for k in D.MANAGER_K:
            for key in ("nn", "dist", "yaw", "nn_norerank"):
                assert fx[f"mgr_{R}x{S}_k{k}_{key}"].shape == (nq, k)
            # the node added last is never returned, not even for the query that is a copy of it
            assert (fx[f"mgr_{R}x{S}_k{k}_nn"] != D.N_MAP - 1).all() and (fx[f"mgr_{R}x{S}_k{k}_nn_norerank"] != D.N_MAP - 1).all()
            assert (np.diff(fx[f"mgr_{R}x{S}_k{k}_dist"], axis=1) >= 0).all()
    for key in ("recall_rerank", "recall_norerank"):
        assert fx[key].shape == (len(D.RADII), D.EVAL_K) and (np.diff(fx[key], axis=1) >= 0).all()
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "scan_context.npz")) < (1 << 20)


def test_shared_inputs_are_deterministic_and_filtered():
    a = [c.copy() for c in D.all_clouds()]
    D._CACHE.clear()
    b = D.all_clouds()
    assert len(a) == len(b) == D.N_MAP + D.N_QUERY
    for x, y in zip(a, b):
        assert x.dtype == np.float32 and x.shape[1] == 3 and np.array_equal(x, y)
        assert not D.near_edge(x).any()
    print("removed shares", D.removed_shares())
    assert max(D.removed_shares()) <= 0.01
    # the margins are more than 20 times the fp32 error of theta (4e-7 rad at 2 pi) and of the range (8e-6 m at 80 m)
    assert D.SECTOR_MARGIN >= 20 * 4e-7 and D.RING_MARGIN >= 20 * 8e-6
    pts, off = D.edge_batch()
    assert off[1] == off[2] == len(D.edge_cloud()) and off[-1] == len(pts)
    e = D.edge_cloud()
    assert np.signbit(e[3, 1]) and not np.signbit(e[2, 1]) and e[2, 1] == e[3, 1] == 0
    assert len(D.manager_queries()) == D.N_QUERY + 1 and np.array_equal(D.manager_queries()[-1], D.map_clouds()[-1])


def test_new_symbols_declared_and_exported(built):
    from egonn_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "egonn_hip.h")).read()
    declared = set(re.findall(r"\b(egonn_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_library_argument_checks_need_no_gpu(built):
    """the up-front checks return the library's invalid status before anything is launched"""
    from egonn_amd import _lib
    lib = _lib.load()
    one = 256       # non-null, aligned, never dereferenced: every call below fails its argument check first
    assert lib.egonn_scan_context(one, 10, one, 1, 60, 41, 80.0, 2.0, one, one, None) == 1
    assert b"num_ring" in lib.egonn_last_error()
    assert lib.egonn_scan_context(one, 10, one, 1, 129, 20, 80.0, 2.0, one, one, None) == 1
    assert lib.egonn_scan_context(one, 10, one, 1, 1, 20, 80.0, 2.0, one, one, None) == 1
    assert lib.egonn_scan_context(one, 10, one, 0, 60, 20, 80.0, 2.0, one, one, None) == 1
    assert lib.egonn_scan_context(one, 10, one, 1, 60, 20, 0.0, 2.0, one, one, None) == 1
    assert b"max_length" in lib.egonn_last_error()
    assert lib.egonn_scan_context(one, 10, None, 1, 60, 20, 80.0, 2.0, one, one, None) == 1
    assert lib.egonn_scan_context_ringkey(one, 4, 0, 60, one, None) == 1
    assert lib.egonn_scan_context_distance(one, 4, one, 7, 20, 130, one, 5, one, one, None) == 1
    assert lib.egonn_scan_context_distance(one, 4, one, 7, 20, 60, None, 5, one, one, None) == 1      # no list: k = n_map
    assert b"k = n_map" in lib.egonn_last_error()
    assert lib.egonn_scan_context_rerank(one, one, one, 4, 0, one + 256, one + 512, one + 768, None) == 1
    assert lib.egonn_scan_context_rerank(one, one, one, 4, 129, one + 256, one + 512, one + 768, None) == 1
    assert lib.egonn_scan_context_rerank(one, one, one, 4, 5, one + 256, one, one + 768, None) == 1    # aliasing
    # nothing to do is not an error
    assert lib.egonn_scan_context_rerank(None, None, None, 0, 5, None, None, None, None) == 0
    assert lib.egonn_scan_context_distance(None, 0, None, 7, 20, 60, None, 7, None, None, None) == 0


def test_binding_rejects_bad_arguments_before_any_device_work():
    """these pass (by raising ValueError) without a GPU"""
    import egonn_amd
    from egonn_amd import scan_context as sc
    for name in ("ScanContext", "ScanContextManager", "sc2rk", "distance_sc", "evaluate_scan_context"):
        assert callable(getattr(egonn_amd, name)), name
    assert egonn_amd.evaluate_scan_context is sc.evaluate
    z = np.zeros
    for bad in (dict(num_ring=0), dict(num_ring=41), dict(num_sector=1), dict(num_sector=129), dict(max_length=0)):
        with pytest.raises(ValueError):
            sc.ScanContext(**bad)
        with pytest.raises(ValueError):
            sc.ScanContextManager(**bad)
    s = sc.ScanContext()
    assert (s.num_sector, s.num_ring, s.max_length, s.lidar_height) == (60, 20, 80.0, 2.0)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        s(z((10, 2), np.float32))
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        s.batch(z((10,), np.float32), [0, 10])
    with pytest.raises(ValueError, match="offsets"):
        s.batch(z((10, 3), np.float32), [10])
    with pytest.raises(ValueError, match="offsets"):
        s.batch(z((10, 3), np.float32), z((2, 2), np.int64))
    with pytest.raises(ValueError, match="descriptor"):
        sc.sc2rk(z((60,), np.float32))
    with pytest.raises(ValueError, match="num_ring"):
        sc.sc2rk(z((41, 60), np.float32))
    with pytest.raises(ValueError, match="different shapes"):
        sc.distance_sc(z((20, 60), np.float32), z((20, 30), np.float32))
    with pytest.raises(ValueError, match="num_sector"):
        sc.distance_sc(z((20, 130), np.float32), z((20, 130), np.float32))
    with pytest.raises(ValueError, match="candidates"):
        sc.distance_pairs(z((2, 20, 60), np.float32), z((3, 20, 60), np.float32), z((3, 5), np.int32))
    with pytest.raises(ValueError, match="k must be"):
        sc.rerank(z((2, 129), np.float32), z((2, 129), np.int32), z((2, 129), np.int32))
    with pytest.raises(ValueError, match="one .* shape"):
        sc.rerank(z((2, 5), np.float32), z((2, 4), np.int32), z((2, 5), np.int32))
    man = sc.ScanContextManager(max_capacity=3)
    with pytest.raises(ValueError, match="capacity exceeded: 3"):
        man.add_nodes(z((30, 3), np.float32), [0, 10, 20, 30])               # 3 nodes: curr_node_idx would reach max_capacity
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        man.add_node(z((30, 4), np.float32))
    assert man.curr_node_idx == 0
    for k in (0, 129):
        with pytest.raises(ValueError, match="k must be"):
            man.query(z((10, 3), np.float32), k=k)
        with pytest.raises(ValueError, match="k must be"):
            sc.evaluate([], [], z((0, 2)), z((0, 2)), D.RADII, k=k)
    with pytest.raises(ValueError, match="Empty database"):
        man.query(z((10, 3), np.float32), k=1)
    with pytest.raises(ValueError, match="one position per cloud"):
        sc.evaluate([z((5, 3), np.float32)], [], z((2, 2)), z((0, 2)), D.RADII, k=1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_scan_context_has_no_cpu_path(built):
    from egonn_amd import scan_context as sc
    pc = D.map_clouds()[0]
    d = np.zeros((20, 60), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.ScanContext()(pc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.sc2rk(d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.distance_sc(d, d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.rerank(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.int32), np.zeros((1, 3), np.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.ScanContextManager().add_node(pc)
    mp, qp = D.positions()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sc.evaluate(D.map_clouds(), D.manager_queries(), mp, qp, D.RADII, k=D.EVAL_K)
