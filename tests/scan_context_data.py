"""Seeded inputs shared by the ScanContext fixture generator (tests/golden/make_golden_scan_context.py) and the tests
(test_scan_context_host.py, test_gpu_scan_context.py): the fixture stores the reference's outputs only, the inputs are rebuilt
here.

Edge filter: the reference bins with numpy's float32 arctan2 and floor-division, which a device cannot promise to match in
the last bit of theta.  Before either side sees a cloud, every point within SECTOR_MARGIN rad of a sector edge or
RING_MARGIN m of a ring edge of ANY of the three fixture shapes is dropped, judged in float64.  fp32 error is about 4e-7 rad
at theta ~ 2 pi and 8e-6 m at 80 m, so the margins are more than 20 times the error.  The hand-placed edge cloud is NOT
filtered: its special points sit exactly on edges where both sides compute exact values."""
import numpy as np

from egonn_amd.synth import lidar_scan

SHAPES = [(20, 60), (24, 90), (8, 16)]            # (num_ring, num_sector) of the stored descriptors
DIST_SHAPES = [(20, 60), (24, 90)]                # shapes of the stored distances and manager queries
MAX_LENGTH, LIDAR_HEIGHT = 80, 2.0
SECTOR_MARGIN, RING_MARGIN = 2e-5, 2e-4
N_MAP, N_QUERY, N_POINTS = 12, 6, 6000
MANAGER_K = (5, 11)
RADII = (5, 20)
EVAL_K = 5

_CACHE = {}


def near_edge(pc):
    """float64 judgement of every point of an (n, 3) cloud: True within the margins of an edge of any fixture shape"""
    p = np.asarray(pc, dtype=np.float64)
    theta = np.arctan2(p[:, 1], p[:, 0]) + np.pi
    r = np.hypot(p[:, 0], p[:, 1])
    bad = np.zeros(len(p), dtype=bool)
    for R, S in SHAPES:
        gs, gr = 2.0 * np.pi / S, MAX_LENGTH / R
        bad |= np.abs(theta / gs - np.round(theta / gs)) * gs < SECTOR_MARGIN
        bad |= np.abs(r / gr - np.round(r / gr)) * gr < RING_MARGIN
    return bad


def edge_filter(pc):
    """-> (filtered cloud, share of points removed)"""
    bad = near_edge(pc)
    return np.ascontiguousarray(pc[~bad]), float(bad.mean()) if len(pc) else 0.0


def _build():
    if "map" not in _CACHE:
        maps, removed = [], []
        for seed in range(N_MAP):
            pc, share = edge_filter(lidar_scan(seed, n_points=N_POINTS))
            maps.append(pc)
            removed.append(share)
        queries = []
        for i in range(N_QUERY):
            a = np.deg2rad(37.0 * (i + 1))
            rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
            pc = (lidar_scan(i, n_points=N_POINTS).astype(np.float64) @ rot.T).astype(np.float32)
            pc, share = edge_filter(pc)
            queries.append(pc)
            removed.append(share)
        _CACHE.update(map=maps, query=queries, removed=removed)
    return _CACHE


def map_clouds():
    return _build()["map"]


def query_clouds():
    return _build()["query"]


def removed_shares():
    return _build()["removed"]


def manager_queries():
    """the rotated queries plus a copy of the node added last, which the reference's KD-tree leaves out (:127)"""
    return query_clouds() + [map_clouds()[N_MAP - 1]]


def all_clouds():
    """the 18 clouds of the descriptor check: 12 map scans, then 6 queries"""
    return map_clouds() + query_clouds()


def edge_cloud():
    """hand-placed float32 points, not filtered.  Rows: 0-1 at and beyond max_length (dropped); 2 on the negative x axis with
    y = +0.0 (theta clips to 2 pi - 1e-6: sector S - 1); 3 the same with y = -0.0 (theta = 0: sector 0); 4 below the ground
    (z + lidar_height < 0: its cell is 0); 5-6 two points of one cell (the higher wins); 7 the origin; 8-10 ordinary points,
    the last with z + lidar_height = +0.5 in the outermost ring of every shape."""
    f = np.float32
    return np.array([[0.0, -80.0, 5.0], [85.0, 3.0, 1.0], [-1.0, 0.0, 0.5], [-1.0, -0.0, 0.75], [10.5, 7.3, -3.0],
                     [20.3, 1.0, 1.0], [20.6, 1.1, 2.5], [0.0, 0.0, 0.0], [-30.2, 12.7, 4.0], [5.5, -41.3, 0.25],
                     [55.1, -55.2, -1.5]], dtype=f)


def edge_batch():
    """(points, offsets) of a batch of three scans: the edge cloud, an empty scan, map scan 0"""
    e, m = edge_cloud(), map_clouds()[0]
    pts = np.ascontiguousarray(np.concatenate([e, m]))
    return pts, np.array([0, len(e), len(e), len(e) + len(m)], dtype=np.int64)


def positions():
    """synthetic float64 (map (12, 2), query (7, 2)) positions at UTM scale: the map along a line, 7 m apart; query i a
    couple of metres off map pose i, the copy of the last node right on it"""
    base = np.array([4.05e6, 3.96e6])
    mpos = base + np.stack([7.0 * np.arange(N_MAP), 0.5 * np.arange(N_MAP)], axis=1)
    off = np.array([[1.0, -0.5], [-2.0, 1.0], [0.5, 2.5], [3.0, 0.0], [-1.0, -1.0], [2.0, 2.0], [0.0, 0.0]])
    qpos = mpos[[0, 1, 2, 3, 4, 5, N_MAP - 1]] + off
    return mpos, qpos


def concat(clouds):
    """list of clouds -> (points (sum n, 3) float32, offsets (len + 1,) int64)"""
    off = np.zeros(len(clouds) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    return np.ascontiguousarray(np.concatenate(clouds).astype(np.float32)), off
