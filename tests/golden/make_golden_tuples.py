"""Golden vectors of the training-tuple path.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference tree and sklearn).

The reference's own functions are imported from their files and run as they are:
    MulranSequences.find_neighbours_ndx   (datasets/mulran/mulran_raw.py:152-159; KDTree.query_radius on a tree built as :139-140)
    filter_query_elements, in_sorted_array (datasets/dataset_utils.py:210-232, 270-275)
    relative_pose                          (datasets/mulran/utils.py:110-124 and misc/poses.py:80-89)
Their modules import packages that are not installed (open3d, MinkowskiEngine, torchvision, third_party.pypcd); empty
stand-in modules are registered first, and the reference's package directories are put on stand-in packages' __path__ (an
installed package named `datasets` would shadow them otherwise).  None of the stand-ins is called.  No reference source
text is stored: the fixture holds inputs and outputs only.

Before writing, the script asserts that the numpy restatement of the fp64 neighbour rule (tests/tuples_data.py) reproduces
EVERY reference row exactly: the reference alone has no excused rows, so the tests demand equality.

    python tests/golden/make_golden_tuples.py
"""
from __future__ import annotations

import importlib.machinery
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("EGONN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import tuples_data as D  # noqa: E402


def load_reference():
    def stub(name, **kw):
        m = types.ModuleType(name)
        m.__spec__ = importlib.machinery.ModuleSpec(name, None)
        m.__dict__.update(kw)
        sys.modules[name] = m
        return m
    stub("open3d")
    stub("MinkowskiEngine")
    stub("torchvision", transforms=stub("torchvision.transforms", Compose=object))
    stub("third_party", pypcd=stub("third_party.pypcd"))
    for pkg in ("datasets", "datasets/mulran", "datasets/kitti", "datasets/southbay", "misc"):
        stub(pkg.replace("/", ".")).__path__ = [os.path.join(REF, pkg)]
    import datasets.base_datasets as bd
    import datasets.dataset_utils as du
    import datasets.mulran.mulran_raw as mr
    import datasets.mulran.utils as mu
    import misc.poses as mp
    return bd, du, mr, mu, mp


def sequence_of(mr, xy):
    """a MulranSequences that holds positions only: the attributes its find_neighbours_ndx reads, built as its __init__ does"""
    from sklearn.neighbors import KDTree
    ds = object.__new__(mr.MulranSequences)
    ds.poses = np.tile(np.eye(4), (len(xy), 1, 1))
    ds.poses[:, :2, 3] = xy
    ds.kdtree = KDTree(ds.get_xy())
    return ds


def reference_rows(mr, xy, radius, drop_anchor=False):
    """generate_training_tuples.py:50-57 per anchor: find_neighbours_ndx, optionally minus the anchor, np.sort"""
    ds = sequence_of(mr, xy)
    off, rows = np.zeros(len(xy) + 1, dtype=np.int64), []
    for anchor in range(len(xy)):
        nb = ds.find_neighbours_ndx(ds.get_xy()[anchor], radius)
        if drop_anchor:
            nb = nb[nb != anchor]
        rows.append(np.sort(nb).astype(np.int32))
        off[anchor + 1] = off[anchor] + len(rows[-1])
    return off, np.concatenate(rows)


def store_rows(out, key, off, idx, xy, radius, exclude_self=False):
    my_off, my_idx = D.radius_rows(xy, xy, radius, exclude_self)
    assert np.array_equal(off, my_off) and np.array_equal(idx, my_idx), f"{key}: the fp64 rule misses a reference row"
    assert idx.max(initial=0) < 32768
    out[key + "_off"], out[key + "_didx"] = off, D.delta_encode(idx)


def main():
    bd, du, mr, mu, mp = load_reference()
    from sklearn.neighbors import KDTree
    out = {}
    for rows in D.TRAJECTORY_ROWS:
        xy = D.trajectory(rows, 1)
        assert xy.shape == (rows, 2)
        out[f"traj{rows}_xy"] = xy
        for r in D.TRAJECTORY_RADII:
            store_rows(out, f"traj{rows}_r{int(r)}", *reference_rows(mr, xy, r), xy, r)
    xy = D.lattice()
    out["lattice_xy"] = xy
    off, idx = reference_rows(mr, xy, D.LATTICE_RADIUS)
    d2 = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)
    out["lattice_boundary_pairs"] = np.int64((d2 == 25.0).sum())
    assert out["lattice_boundary_pairs"] == 1136
    store_rows(out, "lattice_r5", off, idx, xy, D.LATTICE_RADIUS)
    xy = D.stationary()
    out["stationary_xy"] = xy
    store_rows(out, "stationary_r1", *reference_rows(mr, xy, D.STATIONARY_RADIUS), xy, D.STATIONARY_RADIUS)
    off, idx = reference_rows(mr, xy, D.STATIONARY_RADIUS, drop_anchor=True)
    assert (np.diff(off) == 39).all()
    store_rows(out, "stationary_r1_noself", off, idx, xy, D.STATIONARY_RADIUS, exclude_self=True)

    # the float32-map filter case: filter_query_elements itself, and the rows of its tree (query set != reference set)
    map_xy, query_xy = D.filter_case()
    map_set = [bd.EvaluationTuple(i, f"m{i}", map_xy[i]) for i in range(len(map_xy))]
    query_set = [bd.EvaluationTuple(i, f"q{i}", query_xy[i]) for i in range(len(query_xy))]
    kept = du.filter_query_elements(query_set, map_set, D.FILTER_RADIUS)
    kept_mask = np.zeros(len(query_set), dtype=bool)
    kept_mask[[e.timestamp for e in kept]] = True
    assert 0 < kept_mask.sum() < len(query_set), "kept and dropped queries must both be present"
    map32 = np.zeros((len(map_set), 2), dtype=np.float32)
    for ndx, e in enumerate(map_set):
        map32[ndx] = e.position
    rows = KDTree(map32).query_radius(query_xy, D.FILTER_RADIUS)
    f_off = np.zeros(len(query_xy) + 1, dtype=np.int64)
    f_off[1:] = np.cumsum([len(r) for r in rows])
    f_idx = np.concatenate([np.sort(r) for r in rows]).astype(np.int32)
    my_off, my_idx = D.radius_rows(query_xy, map32.astype(np.float64), D.FILTER_RADIUS)
    assert np.array_equal(f_off, my_off) and np.array_equal(f_idx, my_idx), "filter case: the fp64 rule misses a reference row"
    assert np.array_equal(np.diff(f_off) > 0, kept_mask)
    flips = int((np.diff(D.radius_rows(query_xy, map_xy, D.FILTER_RADIUS)[0]) != np.diff(f_off)).sum())
    out.update(filter_map_xy=map_xy, filter_query_xy=query_xy, filter_kept=kept_mask, filter_off=f_off, filter_didx=D.delta_encode(f_idx),
               filter_rows_changed_by_float32=np.int64(flips))

    # relative poses: both reference functions; d0 = the deviation of the restated device formula from them
    for kind in ("local", "utm"):
        poses, ia, ib = D.pose_set(kind)
        ref_neg = np.stack([mu.relative_pose(poses[a], poses[b]) for a, b in zip(ia, ib)])
        ref_plain = np.stack([mp.relative_pose(poses[a], poses[b]) for a, b in zip(ia, ib)])
        mine_neg, st = D.relative_poses(poses, ia, ib, True)
        mine_plain, _ = D.relative_poses(poses, ia, ib, False)
        assert not st.any()
        truth_neg, _ = D.relative_poses(poses, ia, ib, True, dtype=np.longdouble)
        out.update({f"poses_{kind}": poses, f"poses_{kind}_ia": ia, f"poses_{kind}_ib": ib, f"poses_{kind}_ref_neg": ref_neg,
                    f"poses_{kind}_ref_plain": ref_plain,
                    f"poses_{kind}_d0_neg": np.float64(np.abs(mine_neg - ref_neg).max()),
                    f"poses_{kind}_d0_plain": np.float64(np.abs(mine_plain - ref_plain).max()),
                    f"poses_{kind}_ref_err_vs_longdouble": np.float64(np.abs(ref_neg - truth_neg).max()),
                    f"poses_{kind}_restated_err_vs_longdouble": np.float64(np.abs(mine_neg - truth_neg).max())})
        print(kind, {k: float(v) for k, v in out.items() if k.startswith(f"poses_{kind}_") and np.ndim(v) == 0})

    # masks: the tables come from find_neighbours_ndx, the masks from the reference's in_sorted_array loops
    xy = D.mask_positions()
    p_off, p_idx = reference_rows(mr, xy, D.MASK_RADII[0], drop_anchor=True)
    n_off, n_idx = reference_rows(mr, xy, D.MASK_RADII[1])
    assert p_off[11] == p_off[10] and p_off[80] == p_off[79], "tuples 10 and 79 must have no positives"
    out.update(mask_xy=xy, mask_pos_off=p_off, mask_pos_idx=p_idx, mask_non_off=n_off, mask_non_idx=n_idx)
    pos_rows, non_rows = D.rows_of(p_off, p_idx), D.rows_of(n_off, n_idx)
    for B in D.MASK_BATCHES:
        labels = D.mask_labels(B)
        pm = np.array([[du.in_sorted_array(e, pos_rows[label]) for e in labels] for label in labels], dtype=bool)
        nm = np.array([[not du.in_sorted_array(e, non_rows[label]) for e in labels] for label in labels], dtype=bool)
        assert len(set(labels.tolist())) < B and 79 in labels and (B == 4 or 10 in labels) and pm.any() and nm.any()
        out.update({f"mask{B}_labels": labels, f"mask{B}_pos": pm, f"mask{B}_neg": nm})

    path = os.path.join(HERE, "tuples_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays; float32 map changes {flips} rows")


if __name__ == "__main__":
    main()
