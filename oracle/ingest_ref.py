"""TEST INFRASTRUCTURE ONLY (CPU oracle).  numpy restatement of the reference scan loaders:
read_pc of datasets/mulran/mulran_raw.py:19-25 / datasets/kitti/kitti_raw.py:16-22 and the preprocessing of
PointCloudLoader.__call__, misc/point_clouds.py:95-111 (that module itself imports open3d and cannot be imported)."""
import numpy as np

GROUND_PLANE_LEVEL = {"mulran": -0.9, "kitti": -1.5, "southbay": -1.6}


def read_pc(raw_bytes_or_array):
    pc = np.frombuffer(raw_bytes_or_array, dtype=np.float32) if isinstance(raw_bytes_or_array, (bytes, bytearray)) \
        else np.asarray(raw_bytes_or_array, dtype=np.float32).reshape(-1)
    return np.reshape(pc, (-1, 4))[:, :3]                                    # mulran_raw.py:22-24


def preprocess(pc, dataset_type="mulran", remove_zero_points=True, remove_ground_plane=True):
    if remove_zero_points:
        mask = np.all(np.isclose(pc, 0), axis=1)                             # point_clouds.py:103-105
        pc = pc[~mask]
    if remove_ground_plane:
        mask = pc[:, 2] > GROUND_PLANE_LEVEL[dataset_type]                   # :107-109
        pc = pc[mask]
    return pc


def filter_batch(raw, offsets, dataset_type="mulran", remove_zero_points=True, remove_ground_plane=True):
    """`preprocess` per scan of a staged batch: raw (rows, 3|4) float32, scan b = rows [offsets[b], offsets[b+1]); rows
    behind offsets[-1] are not part of the batch.  Returns (survivors (N,3), survivor offsets)."""
    parts, off = [], [0]
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        parts.append(preprocess(raw[lo:hi, :3], dataset_type, remove_zero_points, remove_ground_plane))
        off.append(off[-1] + len(parts[-1]))
    return (np.concatenate(parts) if parts else np.zeros((0, 3), np.float32)), off


def keep_loop(pc, dataset_type="mulran", remove_zero_points=True, remove_ground_plane=True):
    """The same two lines as a plain loop over the rows, in Python floats: np.isclose(v, 0) is |v| <= 1e-8 (atol, the
    rtol term vanishes against 0; NaN is not close), and `pc[:, 2] > level` compares in the array's float32, i.e.
    against float32(level).  Returns the keep mask."""
    level = float(np.float32(GROUND_PLANE_LEVEL[dataset_type]))
    keep = []
    for x, y, z in np.asarray(pc, np.float32)[:, :3].tolist():
        k = True
        if remove_zero_points and abs(x) <= 1e-8 and abs(y) <= 1e-8 and abs(z) <= 1e-8:
            k = False
        if remove_ground_plane and not (z > level):
            k = False
        keep.append(k)
    return np.array(keep, dtype=bool)
