"""Golden vectors of the training augmentation.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference tree).

The reference's own `datasets/augmentation.py` and `misc/poses.py` are imported from their files and run as they are.
`torchvision` is not installed, so a one-class stand-in for `transforms.Compose` (call the list in order) is registered
before the import.  The reference classes draw from the global generators of Python, NumPy and torch; this script feeds
them the draws of the restatement (tests/augment_ref.py) by patching, for the duration of one call,
    random.random / random.uniform, np.random.rand / randn / choice / uniform, torch.randn_like / torch.rand,
each of which pops the next prepared value, so the reference computes with exactly the numbers the device would draw.

Conversions, because a reference class cannot always run on what the previous one returned under the installed
torch / numpy: `RandomTranslation` adds an ndarray to a tensor and `RandomRotation` multiplies a tensor by an ndarray
(`coords @ R`); the script hands these two an ndarray view of the cloud and turns the result back into a tensor.  Both
stay float32 on either side, so no value changes.

The 6-DoF perturbation lives inside `MulranTraining6DOFDataset.__getitem__` (`datasets/mulran/mulran_train.py`), whose
base class reads dataset files.  That module is imported from its file too, with two stand-in modules registered first:
`datasets.base_datasets`, whose `TrainingDataset` holds two clouds and one relative pose in memory, and
`datasets.quantization`, whose `Quantizer` keeps every point in order.  `misc.poses` is the reference's own.  The
reference's `__getitem__` then runs as it is and returns the perturbed positive cloud and the updated pose; a second run on
the same draws with the identity as the pair's pose returns the perturbation matrix itself.  No reference source text is
stored: the fixture holds inputs, draws and outputs only.

    python tests/golden/make_golden_augment.py
"""
from __future__ import annotations

import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("EGONN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import augment_ref as R  # noqa: E402


def load_reference():
    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, x):
            for t in self.transforms:
                x = t(x)
            return x
    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tr.Compose = Compose
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    mods = []
    for name, rel in (("ref_augmentation", "datasets/augmentation.py"), ("ref_poses", "misc/poses.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods.append(m)
    return mods


class _MemoryDataset:
    """stands in for datasets.base_datasets.TrainingDataset: item 0 is the anchor, item 1 its only positive"""

    def __init__(self, *a, **k):
        self.clouds, self.queries = [], []

    def __getitem__(self, ndx):
        return self.clouds[ndx], ndx

    def get_positives(self, ndx):
        return np.array([1])


class _KeepAll:
    """stands in for datasets.quantization.Quantizer: every point survives, in order"""

    def __call__(self, pc):
        return pc, torch.arange(len(pc))


def load_local_phase(poses):
    for name in ("datasets", "datasets.base_datasets", "datasets.quantization", "misc"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["datasets.base_datasets"].TrainingDataset = _MemoryDataset
    sys.modules["datasets.quantization"].Quantizer = _KeepAll
    sys.modules["misc.poses"] = poses
    spec = importlib.util.spec_from_file_location("ref_mulran_train", os.path.join(REF, "datasets/mulran/mulran_train.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.MulranTraining6DOFDataset


class Feed:
    """the prepared values of one call, per patched function, popped in the order the reference asks for them"""

    def __init__(self):
        self.q = {k: [] for k in ("random", "uniform", "rand", "randn", "choice", "np_uniform", "randn_like", "torch_rand")}
        self.saved = {}

    def __enter__(self):
        q = self.q
        self.saved = {(random, "random"): random.random, (random, "uniform"): random.uniform,
                      (np.random, "rand"): np.random.rand, (np.random, "randn"): np.random.randn,
                      (np.random, "choice"): np.random.choice, (np.random, "uniform"): np.random.uniform,
                      (torch, "randn_like"): torch.randn_like, (torch, "rand"): torch.rand}
        random.random = lambda: q["random"].pop(0)
        random.uniform = lambda a, b: a + (b - a) * q["uniform"].pop(0)
        np.random.rand = lambda *s: np.full(s, q["rand"].pop(0), np.float64)
        np.random.randn = lambda *s: np.asarray(q["randn"].pop(0), np.float64).reshape(s)
        np.random.choice = lambda a, size=None, replace=True: q["choice"].pop(0)
        np.random.uniform = lambda low=0.0, high=1.0: low + (high - low) * q["np_uniform"].pop(0)
        torch.randn_like = lambda t: torch.from_numpy(q["randn_like"].pop(0)).to(t.dtype).reshape(t.shape)
        torch.rand = lambda *s: torch.from_numpy(np.asarray(q["torch_rand"].pop(0), np.float32)).reshape(*s)
        return self

    def __exit__(self, *exc):
        for (mod, name), fn in self.saved.items():
            setattr(mod, name, fn)
        left = {k: len(v) for k, v in self.q.items() if v}
        assert exc[0] is not None or not left, f"draws prepared but never asked for: {left}"


def run_train_transform(A, pts, P, sid):
    """the reference's TrainTransform classes one by one on a tensor, with the two ndarray conversions of the docstring"""
    d = R.scan_draws(P, sid, len(pts))
    e = torch.from_numpy(pts.copy())
    with Feed() as f:
        f.q["randn_like"].append(d["jitter_normal"].astype(np.float32))
        e = A.JitterPoints(sigma=P.sigma, clip=P.clip)(e)
        f.q["uniform"].append(d["r_u"])
        f.q["choice"].append(np.nonzero(d["removed"])[0])
        e = A.RemoveRandomPoints(r=(P.r_min, P.r_max))(e)
        removed = (e == 0).all(dim=1).numpy()
        f.q["randn"].append(d["trans_normal"])
        e = torch.from_numpy(np.asarray(A.RandomTranslation(max_delta=P.max_delta)(e.numpy())))
        if P.stages & R.ROTATE:
            f.q["rand"].append(d["rot_u"])
            e = torch.from_numpy(np.asarray(A.RandomRotation(max_theta=P.max_theta, axis=np.array([0, 0, 1]))(e.numpy())))
        assert e.dtype == torch.float32
        before = e.clone()
        f.q["random"].append(d["block_u"])
        on = d["block_u"] < P.block_p
        if on:
            f.q["uniform"] += [d["area_u"], d["aspect_u"], d["x_u"], d["y_u"]]
        blk = A.RemoveRandomBlock(p=P.block_p, scale=tuple(P.scale), ratio=tuple(P.ratio))
        params = np.zeros(4)
        if on:      # get_params alone first, for the fixture; it consumes the same four draws again
            f.q["uniform"] += [d["area_u"], d["aspect_u"], d["x_u"], d["y_u"]]
            params = np.array([float(v) for v in blk.get_params(e)])
        e = blk(e)
        erased = ((e == 0).all(dim=1) & ~(before == 0).all(dim=1)).numpy()
    return e.numpy(), removed, erased, bool(on), params, before.numpy()


def run_set_transform(A, pts, P):
    Q = R.set_draws(P)
    e = torch.from_numpy(pts.copy())
    with Feed() as f:
        if P.stages & R.SET_ROTATE:
            f.q["rand"].append(Q["rot_u"])
            e = torch.from_numpy(np.asarray(A.RandomRotation(max_theta=P.set_max_theta, axis=np.array([0, 0, 1]))(e.numpy())))
        f.q["random"].append(Q["flip_u"])
        e = A.RandomFlip(list(P.flip_p))(e)
    return e.numpy(), Q["flip"]


def run_rigid(Local, pts, P, sid, T_rel):
    """the reference's local-phase __getitem__ on an in-memory pair -> (perturbed positive, m, m @ T_rel)"""
    d = R.scan_draws(P, sid, len(pts))
    ds = Local("", "", _KeepAll(), rot_max=P.rot_max, trans_max=P.trans_max)
    ds.clouds = [torch.zeros((1, 3)), torch.from_numpy(pts.copy())]
    got = []
    for pose in (T_rel, np.eye(4, dtype=np.float32)):
        ds.queries = [types.SimpleNamespace(positives_poses={1: torch.from_numpy(pose.copy())})]
        with Feed() as f:
            f.q["choice"].append(np.array([1]))
            f.q["np_uniform"].append(d["rigid_u"])
            f.q["torch_rand"].append(d["rigid_u24"].reshape(1, 2))
            _, pos, T = ds[0]
        got.append((pos.numpy(), T.numpy()))
    assert np.array_equal(got[0][0], got[1][0])
    return got[0][0], got[1][1], got[0][1]


def main():
    A, poses = load_reference()
    Local = load_local_phase(poses)
    out = {}
    cases = []
    # both modes; seeds searched so that the block is drawn and not drawn and every flip branch appears
    want = {(1, True), (1, False), (2, True), (2, False)}
    flips = {0, 1, -1}
    sid = 0
    while want or flips:
        sid += 1
        for mode in (1, 2):
            P = R.Params(seed=20240 + mode, draw=3, set_id=sid, stages=(R.MODE1 if mode == 1 else R.MODE2) | (R.SET1 if mode == 1 else R.SET2))
            on = R.scan_draws(P, sid, 1)["block_u"] < P.block_p
            fl = R.set_draws(P)["flip"]
            if (mode, on) in want or fl in flips:
                want.discard((mode, on))
                flips.discard(fl)
                cases.append((mode, sid, P))
    for ci, (mode, sid, P) in enumerate(cases):
        n = 1500 + 700 * (ci % 4)
        pts = R.cloud(100 + ci, n)
        o1, removed, erased, on, params, before = run_train_transform(A, pts, P, sid)
        o2, flip = run_set_transform(A, o1, P)
        k = f"c{ci}_"
        out[k + "meta"] = np.array([mode, sid, P.seed, P.draw, P.set_id, int(on), flip], np.int64)
        out[k + "points"], out[k + "stage1"], out[k + "stage2"] = pts, o1, o2
        out[k + "removed"], out[k + "erased"], out[k + "block"], out[k + "before_block"] = removed, erased, params, before
    out["n_cases"] = np.array(len(cases))
    P = R.Params(seed=77, draw=1, stages=R.RIGID, rot_max=np.pi, trans_max=5.0)
    for ri, sid in enumerate((4, 9)):
        pts = R.cloud(300 + ri, 1200)
        T_rel = np.eye(4, dtype=np.float32)
        T_rel[:3, :3] = np.array([[0.8, -0.6, 0], [0.6, 0.8, 0], [0, 0, 1]], np.float32)
        T_rel[:3, 3] = [3.5, -1.25, 0.125 * (ri + 1)]
        o, m, T = run_rigid(Local, pts, P, sid, T_rel)
        out[f"r{ri}_meta"] = np.array([sid, P.seed, P.draw], np.int64)
        out[f"r{ri}_points"], out[f"r{ri}_out"], out[f"r{ri}_m"], out[f"r{ri}_T_rel"], out[f"r{ri}_T"] = pts, o, m, T_rel, T
    path = os.path.join(HERE, "augment_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases)} transform cases, 2 rigid cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
