"""GPU tests of the ScanContext baseline against outputs of the reference's own code (tests/golden/scan_context.npz, written by
tests/golden/make_golden_scan_context.py from the inputs of tests/scan_context_data.py).

Bounds:
  descriptors  bit-equal.  Cell values are fp32 heights; bins agree because the shared inputs keep more than 20 times the fp32
               error away from every bin edge, and the edge cloud's special points are computed exactly by both sides.
  ring keys    rtol 1e-5 against the float64 means: a fixed-order fp32 sum of <= 128 non-negative terms has relative error
               <= 128 * 2^-24 ~ 8e-6.
  distances    |dist - ref| <= 1e-5: each column cosine carries about (R + 3) * 2^-24 relative error and the mean of <= 128
               values in [0, 1] adds <= 8e-6.
  yaw          equal wherever the reference's best and second-best shift similarities differ by more than 4e-5 (4 x the
               distance bound); at most 5 % of the pairs may be left out on that ground.
  rerank       order equal wherever consecutive sorted reference distances differ by more than 2e-5 (2 x the bound).
  candidates   k = 11: equal as sets; k = 5: equal where the 5th and 6th ring-key distances differ by more than 1e-5 relative.
"""
import os

import numpy as np
import pytest
import torch

from tests import scan_context_data as D

pytestmark = pytest.mark.gpu

DIST_TOL, YAW_GAP, ORDER_GAP, RK_RTOL, RK_GAP = 1e-5, 4e-5, 2e-5, 1e-5, 1e-5


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "scan_context.npz"))


@pytest.fixture(scope="module")
def sc_mod(built):
    from egonn_amd import scan_context
    return scan_context


def _cuda(x, dtype=None):
    return torch.as_tensor(x).to(device="cuda", dtype=dtype)


@pytest.fixture(scope="module")
def device_sc(sc_mod):
    """descriptors and ring keys of the 18 clouds, one batched call per shape: {(R, S): (sc, rk)} on the device"""
    pts, off = D.concat(D.all_clouds())
    pts, off = _cuda(pts), _cuda(off)
    out = {}
    for R, S in D.SHAPES:
        out[(R, S)] = sc_mod.ScanContext(S, R, D.MAX_LENGTH, D.LIDAR_HEIGHT).batch(pts, off)
    return out


@pytest.mark.parametrize("shape", D.SHAPES)
def test_descriptors_bit_equal_and_ring_keys(sc_mod, fx, device_sc, shape):
    R, S = shape
    sc, rk = device_sc[shape]
    got = sc.cpu().numpy()
    want = fx[f"sc_{R}x{S}"]
    assert got.dtype == np.float32 and got.shape == want.shape
    bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    print("clouds that differ:", bad, "cells:", int((got != want).sum()))
    assert not bad
    assert not np.signbit(got).any()                          # never -0.0
    err = np.abs(rk.cpu().numpy().astype(np.float64) - fx[f"rk_{R}x{S}"]) / np.maximum(fx[f"rk_{R}x{S}"], 1e-300)
    print("ring key max relative error", err.max())
    assert np.allclose(rk.cpu().numpy(), fx[f"rk_{R}x{S}"], rtol=RK_RTOL, atol=0)
    # sc2rk on its own gives the same bits as the ring keys of the batched call
    assert torch.equal(sc_mod.sc2rk(sc), rk) and torch.equal(sc_mod.sc2rk(sc[3]), rk[3])


@pytest.mark.parametrize("shape", D.SHAPES)
def test_edge_cloud_batch_and_single_scan_forms(sc_mod, fx, device_sc, shape):
    R, S = shape
    s = sc_mod.ScanContext(S, R, D.MAX_LENGTH, D.LIDAR_HEIGHT)
    pts, off = D.edge_batch()
    sc, rk = s.batch(_cuda(pts), _cuda(off))                  # edge cloud, empty scan, map scan 0
    want = fx[f"edge_sc_{R}x{S}"]
    assert np.array_equal(sc.cpu().numpy(), want) and not sc[1].any() and not np.signbit(sc.cpu().numpy()).any()
    assert np.allclose(rk.cpu().numpy(), fx[f"edge_rk_{R}x{S}"], rtol=RK_RTOL, atol=0)
    e = D.edge_cloud()
    one = want[0]
    assert one[0, S - 1] == np.float32(2.5) and one[0, 0] == np.float32(2.75) and one[0, S // 2] == np.float32(2.0)
    # the batched form equals the per-scan form bitwise (host arrays and unaligned device slices included)
    assert torch.equal(s(e), sc[0]) and torch.equal(s(pts[off[2]:off[3]]), sc[2]) and torch.equal(s(pts[:0]), sc[1])
    assert torch.equal(s(_cuda(pts)[off[2]:off[3]]), sc[2])
    assert torch.equal(sc[2], device_sc[shape][0][0])
    # two runs agree bitwise
    sc2, rk2 = s.batch(_cuda(pts), _cuda(off))
    assert torch.equal(sc, sc2) and torch.equal(rk, rk2)
    # distances of the batch's pairs: NaN / yaw 1 with the empty scan; NaN counts as the maximum in a partly defined row
    dist, yaw = sc_mod.distance_pairs(sc, sc)
    dist, yaw = dist.cpu().numpy(), yaw.cpu().numpy()
    wd, wy = fx[f"edge_dist_{R}x{S}"], fx[f"edge_yaw_{R}x{S}"]
    assert np.array_equal(np.isnan(dist), np.isnan(wd))
    assert np.isnan(dist[1]).all() and np.isnan(dist[:, 1]).all() and (yaw[1] == 1).all() and (yaw[:, 1] == 1).all()
    assert np.array_equal(yaw[np.isnan(wd)], wy[np.isnan(wd)])
    fin = ~np.isnan(wd)
    assert (np.abs(dist[fin] - wd[fin]) <= DIST_TOL).all() and np.array_equal(yaw[fin], wy[fin])


def test_large_scan_is_independent_of_point_order(sc_mod):
    from egonn_amd.synth import lidar_scan
    pc = lidar_scan(1, n_points=120_000)                      # several workgroups
    s = sc_mod.ScanContext()
    base = s(_cuda(pc))
    assert base.any()
    rng = np.random.default_rng(5)
    for _ in range(4):
        assert torch.equal(s(_cuda(np.ascontiguousarray(pc[rng.permutation(len(pc))]))), base)
    # inside a batch, at an offset that is not a multiple of four rows
    pts = np.concatenate([pc[:3], pc, pc[:5]])
    sc, _ = s.batch(_cuda(pts), _cuda(np.array([0, 3, 3 + len(pc), len(pts)], dtype=np.int64)))
    assert torch.equal(sc[1], base)


@pytest.mark.parametrize("shape", D.DIST_SHAPES)
def test_distance_and_yaw_match_reference(sc_mod, fx, device_sc, shape):
    R, S = shape
    sc = device_sc[shape][0]
    maps, qs = sc[:D.N_MAP].contiguous(), sc[D.N_MAP:].contiguous()
    dist, yaw = sc_mod.distance_pairs(qs, maps)               # candidates = None: all pairs
    d, y = dist.cpu().numpy().astype(np.float64), yaw.cpu().numpy()
    err = np.abs(d - fx[f"dist_{R}x{S}"])
    print("max |dist - ref|", err.max())
    assert (err <= DIST_TOL).all()
    decided = fx[f"simgap_{R}x{S}"] > YAW_GAP
    print("pairs left out of the yaw check:", int((~decided).sum()), "of", decided.size)
    assert (~decided).mean() <= 0.05
    assert np.array_equal(y[decided], fx[f"yaw_{R}x{S}"][decided])
    # the listed form equals the all-pairs form bitwise, whatever the list's order; -1 and out-of-range give (+inf, -1)
    rng = np.random.default_rng(3)
    cand = np.stack([rng.permutation(D.N_MAP) for _ in range(D.N_QUERY)]).astype(np.int32)
    cand[1, 2] = -1
    cand[4, 0] = -1
    cand[5, 7] = D.N_MAP
    dl, yl = sc_mod.distance_pairs(qs, maps, _cuda(cand))
    dl, yl = dl.cpu().numpy(), yl.cpu().numpy()
    miss = (cand < 0) | (cand >= D.N_MAP)
    assert np.isposinf(dl[miss]).all() and (yl[miss] == -1).all()
    rows = np.arange(D.N_QUERY)[:, None].repeat(D.N_MAP, 1)
    safe = np.where(miss, 0, cand)
    assert np.array_equal(dl[~miss], dist.cpu().numpy()[rows, safe][~miss]) and np.array_equal(yl[~miss], y[rows, safe][~miss])
    # one pair through the reference's signature: the candidate is the descriptor that is shifted
    d00, y00 = sc_mod.distance_sc(maps[4], qs[2])
    assert d00 == float(dist[2, 4]) and y00 == int(yaw[2, 4])
    # a descriptor against itself: distance 0 at the identity shift, which wins only by being the strict maximum
    ds, ys = sc_mod.distance_sc(maps[0], maps[0])
    assert abs(ds) <= DIST_TOL and ys == 0


def test_all_zero_descriptors_and_many_sectors(sc_mod):
    z = torch.zeros((2, 20, 60), device="cuda")
    z[1, 3, 7] = 1.5
    dist, yaw = sc_mod.distance_pairs(z, z)
    assert torch.isnan(dist[0]).all() and torch.isnan(dist[:, 0]).all() and (yaw[0] == 1).all() and (yaw[:, 0] == 1).all()
    # one occupied column against itself: only the identity shift has a common column, every other shift is 0 / 0 = NaN,
    # which np.max / np.argmax treat as the maximum: (NaN, first NaN shift 1 -> yaw 1)
    assert torch.isnan(dist[1, 1]) and int(yaw[1, 1]) == 1
    # S > 64 (two shifts per lane) and the largest shape against a float64 evaluation of the same formula
    rng = np.random.default_rng(11)
    for R, S in ((40, 128), (3, 65), (1, 2)):
        a = rng.uniform(0, 5, (3, R, S)).astype(np.float32)
        if R > 1:
            a[rng.random((3, R, S)) < 0.3] = 0
            a[0, :, : S // 3] = 0                               # empty columns: masks differ between shifts
        dist, yaw = sc_mod.distance_pairs(_cuda(a), _cuda(a))
        dist, yaw = dist.cpu().numpy(), yaw.cpu().numpy()
        for i in range(3):
            for j in range(3):
                q, c = a[i].astype(np.float64), a[j].astype(np.float64)
                nq = np.linalg.norm(q, axis=0)
                sims = np.full(S, np.nan)
                for sh in range(1, S + 1):
                    r = np.roll(c, sh, axis=1)
                    nr = np.linalg.norm(r, axis=0)
                    m = (nr > 1e-8) & (nq > 1e-8)
                    if m.any():
                        sims[sh - 1] = ((r[:, m] * q[:, m]).sum(0) / (nr[m] * nq[m])).sum() / m.sum()
                assert not np.isnan(sims).any()
                assert abs(dist[i, j] - (1.0 - sims.max())) <= DIST_TOL, (R, S, i, j)
                top = np.sort(sims)[::-1]
                if top[0] - top[1] > YAW_GAP:
                    assert yaw[i, j] == (np.argmax(sims) + 1) % S, (R, S, i, j)


def test_rerank_orders_like_argsort(sc_mod):
    inf, nan = np.inf, np.nan
    dist = np.array([[0.5, nan, 0.25, inf, 0.25, 0.0, nan], [3.0, 2.0, 1.0, 0.5, 0.25, 0.125, 0.0]], dtype=np.float32)
    cand = np.array([[4, 9, 7, -1, 2, 11, 3], [0, 1, 2, 3, 4, 5, 6]], dtype=np.int32)
    yaw = np.array([[10, 1, 12, -1, 14, 15, 1], [1, 2, 3, 4, 5, 6, 7]], dtype=np.int32)
    oi, od, oy = (t.cpu().numpy() for t in sc_mod.rerank(_cuda(dist), _cuda(yaw), _cuda(cand)))
    assert oi.tolist() == [[11, 2, 7, 4, -1, 3, 9], [6, 5, 4, 3, 2, 1, 0]]       # ties: lower candidate index; NaN last
    assert oy.tolist() == [[15, 14, 12, 10, -1, 1, 1], [7, 6, 5, 4, 3, 2, 1]]
    assert np.array_equal(od[0, :5], np.array([0.0, 0.25, 0.25, 0.5, inf], np.float32)) and np.isnan(od[0, 5:]).all()
    # k = 128, random with repeats: a stable argsort over (distance, candidate index)
    rng = np.random.default_rng(2)
    d = rng.integers(0, 40, (5, 128)).astype(np.float32)
    c = np.stack([rng.permutation(128) for _ in range(5)]).astype(np.int32)
    oi, od, _ = (t.cpu().numpy() for t in sc_mod.rerank(_cuda(d), _cuda(np.zeros_like(c)), _cuda(c)))
    for q in range(5):
        order = np.lexsort((c[q], d[q]))
        assert np.array_equal(oi[q], c[q][order]) and np.array_equal(od[q], d[q][order])


@pytest.fixture(scope="module")
def managers(sc_mod):
    pts, off = D.concat(D.map_clouds())
    out = {}
    for R, S in D.DIST_SHAPES:
        for last in (False, True):
            m = sc_mod.ScanContextManager(S, R, D.MAX_LENGTH, D.LIDAR_HEIGHT, include_last_node=last)
            m.add_nodes(pts[:off[5]], off[:6])                  # batched, then one by one
            for c in D.map_clouds()[5:]:
                m.add_node(c)
            out[(R, S, last)] = m
    return out


@pytest.mark.parametrize("shape", D.DIST_SHAPES)
def test_manager_candidates_and_rerank_match_reference(sc_mod, fx, managers, shape):
    R, S = shape
    man = managers[(R, S, False)]
    assert man.curr_node_idx == D.N_MAP and man.scancontexts.shape == (D.N_MAP, R, S)
    assert np.array_equal(man.scancontexts.cpu().numpy(), fx[f"sc_{R}x{S}"][:D.N_MAP])
    qpts, qoff = D.concat(D.manager_queries())
    rk = fx[f"rk_{R}x{S}"]
    qrk = np.concatenate([rk[D.N_MAP:], rk[D.N_MAP - 1:D.N_MAP]])
    rkd = np.sort(np.linalg.norm(qrk[:, None] - rk[None, :D.N_MAP - 1], axis=2), axis=1)
    for k in D.MANAGER_K:
        nn, dist, yaw = man.query_batch(_cuda(qpts), _cuda(qoff), k=k, reranking=True)
        nn, dist, yaw = nn.cpu().numpy(), dist.cpu().numpy(), yaw.cpu().numpy()
        raw, none_d, none_y = man.query_batch(_cuda(qpts), _cuda(qoff), k=k, reranking=False)
        assert none_d is None and none_y is None
        raw = raw.cpu().numpy()
        want_nn, want_d, want_y = (fx[f"mgr_{R}x{S}_k{k}_{key}"] for key in ("nn", "dist", "yaw"))
        assert (nn != D.N_MAP - 1).all() and (raw != D.N_MAP - 1).all()        # the last node is absent by default
        for q in range(len(qrk)):
            settled = k == D.N_MAP - 1 or (rkd[q, k] - rkd[q, k - 1]) > RK_GAP * rkd[q, k]
            assert settled, "the fixture's candidate sets are all decided by more than rounding"
            assert set(raw[q].tolist()) == set(fx[f"mgr_{R}x{S}_k{k}_nn_norerank"][q].tolist()) == set(nn[q].tolist())
            assert np.isfinite(dist[q]).all() and (np.diff(dist[q]) >= 0).all()
            assert (np.abs(dist[q] - want_d[q]) <= DIST_TOL).all()
            gaps = np.diff(want_d[q])
            firm = np.concatenate([[True], gaps > ORDER_GAP]) & np.concatenate([gaps > ORDER_GAP, [True]])
            assert np.array_equal(nn[q][firm], want_nn[q][firm])
            if q < D.N_QUERY:                                   # the stored similarity gaps cover the rotated queries
                firm &= fx[f"simgap_{R}x{S}"][q, want_nn[q]] > YAW_GAP
                assert np.array_equal(yaw[q][firm], want_y[q][firm])
        # one query through the reference's signature
        n1, d1, y1 = man.query(D.manager_queries()[2], k=k, reranking=True)
        assert isinstance(n1, np.ndarray) and np.array_equal(n1, nn[2]) and np.array_equal(d1, dist[2]) and np.array_equal(y1, yaw[2])
        n2, d2, y2 = man.query(D.manager_queries()[2], k=k, reranking=False)
        assert np.array_equal(n2, raw[2]) and d2 is None and y2 is None
    # include_last_node=True: the copy of the last node finds it, at distance 0
    full = managers[(R, S, True)]
    nn, dist, yaw = full.query(D.manager_queries()[-1], k=D.N_MAP, reranking=True)
    assert nn[0] == D.N_MAP - 1 and abs(dist[0]) <= DIST_TOL and yaw[0] == 0 and sorted(nn.tolist()) == list(range(D.N_MAP))
    with pytest.raises(ValueError, match="exceeds"):
        man.query(D.manager_queries()[0], k=D.N_MAP)            # 11 searchable nodes by default


def test_evaluate_recall_table(sc_mod, fx):
    mpos, qpos = D.positions()
    for rerank, key in ((True, "recall_rerank"), (False, "recall_norerank")):
        got = sc_mod.evaluate(D.map_clouds(), D.manager_queries(), mpos, qpos, D.RADII, k=D.EVAL_K, reranking=rerank)
        table = np.array([got["recall1"][r] for r in D.RADII])
        print(key, table.tolist())
        assert np.array_equal(table, fx[key])
    # a sample of the queries, and every node searchable: the copy of the last node is then found
    sub = sc_mod.evaluate(D.map_clouds(), D.manager_queries(), mpos, qpos, D.RADII, k=D.EVAL_K, query_indexes=[6, 0],
                          include_last_node=True)
    assert sub["recall1"][5][0] == 1.0 and sub["nn_index"].shape == (2, D.EVAL_K)


def test_graph_capture_replays_the_eager_bits(sc_mod):
    R, S = D.DIST_SHAPES[0]
    s = sc_mod.ScanContext(S, R, D.MAX_LENGTH, D.LIDAR_HEIGHT)
    mp, mo = D.concat(D.map_clouds())
    qp, qo = D.concat(D.query_clouds())
    mp, mo, qp, qo = _cuda(mp), _cuda(mo), _cuda(qp), _cuda(qo)
    rng = np.random.default_rng(9)
    cand = _cuda(np.stack([rng.permutation(D.N_MAP)[:7] for _ in range(D.N_QUERY)]).astype(np.int32))

    def run():
        msc, _ = s.batch(mp, mo)
        qsc, _ = s.batch(qp, qo)
        dist, yaw = sc_mod.distance_pairs(qsc, msc, cand)
        return (msc, qsc) + sc_mod.rerank(dist, yaw, cand)

    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run()
    for t in outs:
        t.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert torch.equal(a, b)
