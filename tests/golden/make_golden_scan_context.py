"""Writes tests/golden/scan_context.npz: outputs of the REFERENCE's third_party/scan_context/scan_context.py on the inputs of
tests/scan_context_data.py.  Runs only where the reference tree is present:

    python tests/golden/make_golden_scan_context.py --reference /path/to/reference

The reference imports `numpy_indexed` for one call, `group_by(keys).max(values)`; a stand-in with that one method is placed
in sys.modules (the pattern of the MinkowskiEngine stand-in in make_golden.py).  No reference source text is stored, only
arrays its code computed, plus one quantity of our own: `simgap_*`, the float64 gap between the best and the second-best
shift similarity of a pair, which tells the yaw test where the argmax is decided by more than rounding (this script asserts
that its similarities reproduce the reference's distance).
"""
import argparse
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests import scan_context_data as D  # noqa: E402


def install_numpy_indexed():
    class _GroupBy:
        def __init__(self, keys):
            self.keys = np.asarray(keys)

        def max(self, values):
            values = np.asarray(values)
            if len(self.keys) == 0:
                return self.keys[:0], values[:0]
            order = np.argsort(self.keys, kind="stable")
            k, v = self.keys[order], values[order]
            uniq, first = np.unique(k, return_index=True)
            return uniq, np.maximum.reduceat(v, first)

    m = types.ModuleType("numpy_indexed")
    m.group_by = _GroupBy
    sys.modules["numpy_indexed"] = m


def shift_similarities(cand, query):
    """float64 similarity of every shift 1..S (our own restatement, used for `simgap` only)"""
    S = cand.shape[1]
    nq = np.linalg.norm(query, axis=0)
    out = np.full(S, np.nan)
    for i in range(1, S + 1):
        a = np.roll(cand, i, axis=1)
        na = np.linalg.norm(a, axis=0)
        m = (na > 1e-8) & (nq > 1e-8)
        if m.any():
            out[i - 1] = ((a[:, m] * query[:, m]).sum(0) / (na[m] * nq[m])).sum() / m.sum()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree")
    ap.add_argument("--out", default=os.path.join(HERE, "scan_context.npz"))
    args = ap.parse_args()
    install_numpy_indexed()
    sys.path.insert(0, args.reference)
    from third_party.scan_context import scan_context as ref          # REFERENCE module

    out = {}
    clouds = D.all_clouds()
    assert max(D.removed_shares()) <= 0.01, D.removed_shares()
    e_pts, e_off = D.edge_batch()
    e_clouds = [e_pts[e_off[i]:e_off[i + 1]] for i in range(len(e_off) - 1)]
    generic = D.edge_cloud()[[4, 5, 6, 8, 9, 10]]
    assert not D.near_edge(generic).any(), "an ordinary point of the edge cloud sits near an edge"
    for R, S in D.SHAPES:
        sc = ref.ScanContext(num_sector=S, num_ring=R, max_length=D.MAX_LENGTH, lidar_height=D.LIDAR_HEIGHT)   # REFERENCE
        d = np.stack([sc(c) for c in clouds])
        assert np.array_equal(d.astype(np.float32).astype(np.float64), d), "descriptor values are not float32 heights"
        out[f"sc_{R}x{S}"] = d.astype(np.float32)
        out[f"rk_{R}x{S}"] = np.stack([ref.sc2rk(x) for x in d])                                                # REFERENCE
        e = np.stack([sc(c) for c in e_clouds])
        assert np.array_equal(e.astype(np.float32).astype(np.float64), e) and not e[1].any()
        out[f"edge_sc_{R}x{S}"] = e.astype(np.float32)
        out[f"edge_rk_{R}x{S}"] = np.stack([ref.sc2rk(x) for x in e])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                              # 0 / 0 of the empty scan
            pairs = [[ref.distance_sc(e[j], e[i]) for j in range(3)] for i in range(3)]                        # REFERENCE
        out[f"edge_dist_{R}x{S}"] = np.array([[p[0] for p in row] for row in pairs], dtype=np.float64)
        out[f"edge_yaw_{R}x{S}"] = np.array([[p[1] for p in row] for row in pairs], dtype=np.int64)

    mq = D.manager_queries()
    for R, S in D.DIST_SHAPES:
        maps, qs = out[f"sc_{R}x{S}"][:D.N_MAP].astype(np.float64), out[f"sc_{R}x{S}"][D.N_MAP:].astype(np.float64)
        dist, yaw, gap = np.zeros((D.N_QUERY, D.N_MAP)), np.zeros((D.N_QUERY, D.N_MAP), np.int64), np.zeros((D.N_QUERY, D.N_MAP))
        for i in range(D.N_QUERY):
            for j in range(D.N_MAP):
                dist[i, j], yaw[i, j] = ref.distance_sc(maps[j], qs[i])                                        # REFERENCE
                sims = shift_similarities(maps[j], qs[i])
                assert abs((1.0 - sims.max()) - dist[i, j]) < 1e-12 and (np.argmax(sims) + 1) % S == yaw[i, j]
                top = np.sort(sims)[::-1]
                gap[i, j] = top[0] - top[1]
        out[f"dist_{R}x{S}"], out[f"yaw_{R}x{S}"], out[f"simgap_{R}x{S}"] = dist, yaw, gap

        man = ref.ScanContextManager(num_sector=S, num_ring=R, max_length=D.MAX_LENGTH, lidar_height=D.LIDAR_HEIGHT)  # REFERENCE
        for c in D.map_clouds():
            man.add_node(c)
        for k in D.MANAGER_K:
            res = [man.query(q, k=k, reranking=True) for q in mq]
            out[f"mgr_{R}x{S}_k{k}_nn"] = np.stack([r[0] for r in res]).astype(np.int64)
            out[f"mgr_{R}x{S}_k{k}_dist"] = np.stack([r[1] for r in res])
            out[f"mgr_{R}x{S}_k{k}_yaw"] = np.stack([r[2] for r in res]).astype(np.int64)
            out[f"mgr_{R}x{S}_k{k}_nn_norerank"] = np.stack([man.query(q, k=k, reranking=False)[0] for q in mq]).astype(np.int64)

    # the recall table: the counting of evaluate_scan_context.py:53-84 around the REFERENCE manager with its defaults
    mpos, qpos = D.positions()
    man = ref.ScanContextManager()
    for c in D.map_clouds():
        man.add_node(c)
    for rerank in (True, False):
        hits = np.zeros((len(D.RADII), D.EVAL_K))
        for q, pos in zip(mq, qpos):
            nn = man.query(q, D.EVAL_K, reranking=rerank)[0]
            best = np.minimum.accumulate(np.linalg.norm(pos - mpos[nn], axis=1))
            hits += np.array([best <= r for r in D.RADII])
        out["recall_rerank" if rerank else "recall_norerank"] = hits / len(mq)
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes;", "removed shares max", max(D.removed_shares()))
    for R, S in D.DIST_SHAPES:
        print(R, S, "min sim gap", out[f"simgap_{R}x{S}"].min(), "recall", out["recall_rerank"].tolist())


if __name__ == "__main__":
    main()
