"""ORACLE — TEST INFRASTRUCTURE ONLY.  Never imported by the product path (egonn_amd/).

float64 restatement of the EgoNN eval graph, ONE FUNCTION PER STAGE, written from the reference model definition
(models/minkgl.py, layers/eca_block.py, layers/pooling.py, datasets/quantization.py) and oracle/egonn_ref.py.  A stage takes its
input maps in the row order of an oracle.egonn_ref.SparseLevels and the state dict; nothing is rounded to fp32 in between, so a
stage's output is the ground truth for whatever produced the same input:

  conv0(lv, feats)                 level-0 map (k=5 convolution + BN + ReLU), 32 channels
  block(lv, i, x_prev)             level-i map (k2s2 + BN + ReLU, conv1, conv2, ECA gate, downsample branch, residual, ReLU),
                                   with the intermediates: the gate[b][c] among them
  local_head(lv, x3, x4)           descriptors, keypoints, sigma of every level-3 row (and the pre-activations)
  global_head(lv, x5, x6, x7, pool)  global descriptor for GeM / MAC / SPoC

bf16 = True rounds (to nearest even) exactly where the HIP forward stores a bf16 map — y, t1, t2 and the block output of a block,
the level-4 lateral and u3 of the local head, g7 / u6 / g6 / u5 of the global head, the level-0 map — and rounds the sparse-conv
weights to bf16; everything else stays float64.

The second half restates every stage through the fp32 oracle (oracle/egonn_ref.py) on the same input rounded to fp32 ("teacher
forcing"): its deviation from the float64 stage is the noise floor of one fp32 evaluation of that stage, e_ref.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

try:
    from . import egonn_ref as ref
    from . import me_ops as ops
except ImportError:  # oracle/ on sys.path
    import egonn_ref as ref  # type: ignore
    import me_ops as ops  # type: ignore

F64 = np.float64
F32 = np.float32
PLANES = ref.PLANES
BN_EPS = 1e-5


def round_bf16(a):
    """float64 -> nearest bf16 (ties to even, through fp32), returned as float64"""
    f = np.ascontiguousarray(a, dtype=F32)
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    out = r.view(F32).astype(F64)
    return np.where(np.isfinite(f), out, f.astype(F64))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _softplus(x):
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def _scan_of_rows(c4):
    return np.asarray(c4)[:, 0].astype(np.int64)


def segment_mean(x, c4, B):
    out = np.zeros((B, x.shape[1]), dtype=F64)
    b = _scan_of_rows(c4)
    for i in range(B):
        r = b == i
        if r.any():
            out[i] = x[r].sum(axis=0) / float(r.sum())
    return out


def segment_max(x, c4, B):
    out = np.zeros((B, x.shape[1]), dtype=F64)
    b = _scan_of_rows(c4)
    for i in range(B):
        r = b == i
        if r.any():
            out[i] = x[r].max(axis=0)
    return out


def keypoint_position_f64(mode, step, c3, level, off):
    """Quantizer.keypoint_position (datasets/quantization.py:60-72, 93-103) in float64; step as the fp32 values the kernels get"""
    s = np.asarray([F32(v) for v in (list(step) * 3)[:3]], dtype=F64)
    c = (np.asarray(c3, dtype=F64) + 0.5) * s
    kp = c + np.asarray(off, dtype=F64) * (float(1 << level) * s) / 2.0
    if mode == 0:
        return kp
    theta = np.pi * (kp[:, 0] - 180.0) / 180.0
    return np.stack([np.cos(theta) * kp[:, 1], np.sin(theta) * kp[:, 1], kp[:, 2]], axis=1)


def keypoint_position_f32(mode, step, c3, level, off):
    """the same in the reference's exact fp32 operation order — (C + 0.5) * q + offset * (stride * q) / 2, every operation rounded
    once — as the quantizers of oracle/egonn_ref.py evaluate it.  Returns (positions, theta, radius): theta and radius (fp32, None
    for Cartesian) are what cos / sin are taken of and multiplied by."""
    s = np.asarray([F32(v) for v in (list(step) * 3)[:3]], dtype=F32)
    c = ((np.asarray(c3).astype(F32) + F32(0.5)) * s).astype(F32)
    size = (F32(1 << level) * s).astype(F32)
    kp = (c + ((np.asarray(off, dtype=F32) * size).astype(F32) / F32(2.0)).astype(F32)).astype(F32)
    if mode == 0:
        return kp, None, None
    theta = ((F32(np.pi) * (kp[:, 0] - F32(180.0))).astype(F32) / F32(180.0)).astype(F32)
    x = (np.cos(theta).astype(F32) * kp[:, 1]).astype(F32)
    y = (np.sin(theta).astype(F32) * kp[:, 1]).astype(F32)
    return np.stack([x, y, kp[:, 2]], axis=1).astype(F32), theta, kp[:, 1].copy()


class Stages:
    """The eval graph in float64, stage by stage.  sd: state dict (numpy); mode 0 Cartesian / 1 polar and step: the quantizer."""

    def __init__(self, state_dict: Dict[str, np.ndarray], mode: int = 0, step=(0.1,), bf16: bool = False):
        self.sd = {k: np.asarray(v, dtype=F64) for k, v in state_dict.items() if np.asarray(v).dtype.kind == "f"}
        self.mode, self.step, self.bf16 = int(mode), [float(s) for s in np.atleast_1d(step)], bool(bf16)

    # ------------------------------------------------------------------ pieces
    def _r(self, x):
        return round_bf16(x) if self.bf16 else x

    def _w(self, key):
        """sparse-conv kernel (rounded to bf16 with bf16 maps)"""
        return round_bf16(self.sd[key]) if self.bf16 else self.sd[key]

    def _bn(self, x, prefix):
        sd = self.sd
        inv = 1.0 / np.sqrt(sd[prefix + ".bn.running_var"] + BN_EPS)
        return (x - sd[prefix + ".bn.running_mean"]) * inv * sd[prefix + ".bn.weight"] + sd[prefix + ".bn.bias"]

    @staticmethod
    def _conv(maps, x, w, n_out):
        out = np.zeros((n_out, w.shape[-1]), dtype=F64)
        for k, (j, o) in enumerate(maps):
            if len(j):
                out[o] += x[j] @ w[k]            # every output row appears at most once per offset
        return out

    def _tconv(self, lv, level_out, x, w):
        maps = [(o, j) for j, o in lv.kmap(level_out, level_out + 1, 2)]
        return self._conv(maps, x, w, lv.n(level_out))

    def _mlp(self, x, prefix):
        sd = self.sd
        h = np.maximum(x @ sd[prefix + ".net.0.linear.weight"].T + sd[prefix + ".net.0.linear.bias"], 0.0)
        return h @ sd[prefix + ".net.2.linear.weight"].T + sd[prefix + ".net.2.linear.bias"]

    # ------------------------------------------------------------------ stages
    def conv0(self, lv, feats):
        """models/minkgl.py:138-140: relu(bn0(conv k=5 (features)))"""
        x = self._conv(lv.kmap(0, 0, 5), np.asarray(feats, dtype=F64).reshape(lv.n(0), 1), self.sd["trunk.convs.0.kernel"], lv.n(0))
        return self._r(np.maximum(self._bn(x, "trunk.bn.0"), 0.0))

    def block(self, lv, i, x_prev, B=None):
        """models/minkgl.py:143-150 for level i: relu(bn(conv k2s2)), then the ECABasicBlock (layers/eca_block.py:56-73).
        Returns a dict: out, gate (B, C), y, t1, t2."""
        B = lv.batch_size if B is None else B
        pre = f"trunk.blocks.{i}.0"
        n = lv.n(i)
        x_prev = np.asarray(x_prev, dtype=F64)
        y = self._r(np.maximum(self._bn(self._conv(lv.kmap(i - 1, i, 2), x_prev, self._w(f"trunk.convs.{i}.kernel"), n),
                                        f"trunk.bn.{i}"), 0.0))
        m3 = lv.kmap(i, i, 3)
        t1 = self._r(np.maximum(self._bn(self._conv(m3, y, self._w(pre + ".conv1.kernel"), n), pre + ".norm1"), 0.0))
        t2 = self._bn(self._conv(m3, t1, self._w(pre + ".conv2.kernel"), n), pre + ".norm2")
        # ECALayer (eca_block.py:21-36): per-scan channel means (of the accumulators: the conv2 epilogue sums them before the
        # store), Conv1d over the channel axis with zero padding, sigmoid
        c4 = lv.coords[i]
        mean = segment_mean(t2, c4, B)
        w = self.sd[pre + ".eca.conv.weight"].reshape(-1)
        k = len(w)
        pad = (k - 1) // 2
        mp = np.pad(mean, ((0, 0), (pad, pad)))
        gate = _sigmoid(sum(w[j] * mp[:, j:j + mean.shape[1]] for j in range(k)))
        t2 = self._r(t2)
        if (pre + ".downsample.0.kernel") in self.sd:
            res = self._bn(y @ self.sd[pre + ".downsample.0.kernel"], pre + ".downsample.1")
        else:
            res = y
        out = self._r(np.maximum(t2 * gate[_scan_of_rows(c4)] + res, 0.0))
        return {"out": out, "gate": gate, "y": y, "t1": t1, "t2": t2}

    def local_head(self, lv, x3, x4, ignore_kp=False):
        """MinkHead over levels 3, 4 (models/minkgl.py:46-60) + the three regressors (:175-225, 287-308)"""
        sd = self.sd
        l4 = self._r(np.asarray(x4, dtype=F64) @ sd["local_head.conv1x1.4.kernel"])
        u3 = self._r(self._tconv(lv, 3, l4, self._w("local_head.tconv.4.kernel")))
        xl = u3 + np.asarray(x3, dtype=F64) @ sd["local_head.conv1x1.3.kernel"]
        d = self._mlp(xl, "local_descriptor_decoder")
        nrm = np.sqrt((d * d).sum(axis=1, keepdims=True))
        desc = d / np.maximum(nrm, 1e-12)
        pre_kp = self._mlp(xl, "local_keypoint_regressor")
        off = np.zeros_like(pre_kp) if ignore_kp else np.tanh(pre_kp)
        kp = keypoint_position_f64(self.mode, self.step, lv.coords[3][:, 1:], 3, off)
        pre_sg = self._mlp(xl, "local_sigma_regressor")
        return {"descriptors": desc, "keypoints": kp, "sigma": _softplus(pre_sg), "pre_tanh": pre_kp, "pre_softplus": pre_sg,
                "offsets": off, "input": xl}

    def global_head(self, lv, x5, x6, x7, pool="GeM", B=None):
        """MinkHead over levels 5, 6, 7 + descriptor decoder + pooling (layers/pooling.py:46-86): (B, 256)"""
        B = lv.batch_size if B is None else B
        sd = self.sd
        g7 = self._r(np.asarray(x7, dtype=F64) @ sd["global_head.conv1x1.7.kernel"])
        u6 = self._r(self._tconv(lv, 6, g7, self._w("global_head.tconv.7.kernel")))
        g6 = self._r(u6 + np.asarray(x6, dtype=F64) @ sd["global_head.conv1x1.6.kernel"])
        u5 = self._r(self._tconv(lv, 5, g6, self._w("global_head.tconv.6.kernel")))
        g5 = u5 + np.asarray(x5, dtype=F64) @ sd["global_head.conv1x1.5.kernel"]
        gd = self._mlp(g5, "global_descriptor_decoder")
        c4 = lv.coords[5]
        if pool == "MAC":
            return segment_max(gd, c4, B)
        if pool == "SPoC":
            return segment_mean(gd, c4, B)
        p = float(F32(self.sd["global_pooling.pooling.p"].reshape(-1)[0]))
        t = segment_mean(np.power(np.maximum(gd, 1e-6), p), c4, B)
        return np.power(t, 1.0 / p)                      # an empty scan: mean 0 -> 0

    # ------------------------------------------------------------------ chained (host tests)
    def forward(self, lv, feats, B=None, pool="GeM", ignore_kp=False):
        B = lv.batch_size if B is None else B
        x = {0: self.conv0(lv, feats)}
        gates = {}
        for i in range(1, 8):
            r = self.block(lv, i, x[i - 1], B)
            x[i], gates[i] = r["out"], r["gate"]
        return {"levels": x, "gates": gates, "local": self.local_head(lv, x[3], x[4], ignore_kp),
                "global": self.global_head(lv, x[5], x[6], x[7], pool, B)}


# ----------------------------------------------------------------------------- the fp32 oracle, stage by stage (teacher forcing)
class RefStages:
    """The same stages through oracle/egonn_ref.py (numpy fp32, every operation rounded), fed the given input rounded to fp32."""

    def __init__(self, state_dict, mode=0, step=(0.1,)):
        step = [float(s) for s in np.atleast_1d(step)]
        q = ref.CartesianQuantizer(step[0]) if mode == 0 else ref.PolarQuantizer(step)
        self.o = ref.EgoNNOracle(state_dict, q)

    def conv0(self, lv, feats):
        sd = self.o.sd
        x = ops.conv_forward(np.asarray(feats, dtype=F32).reshape(-1, 1), sd["trunk.convs.0.kernel"], lv.kmap(0, 0, 5), lv.n(0))
        return ref.relu(ref.batchnorm_eval(x, sd, "trunk.bn.0"))

    def block(self, lv, i, x_prev):
        sd = self.o.sd
        x = ops.conv_forward(np.asarray(x_prev, dtype=F32), sd[f"trunk.convs.{i}.kernel"], lv.kmap(i - 1, i, 2), lv.n(i))
        x = ref.relu(ref.batchnorm_eval(x, sd, f"trunk.bn.{i}"))
        return self.o._eca_block(x, lv, i, f"trunk.blocks.{i}.0")

    def local_head(self, lv, x3, x4, ignore_kp=False):
        o = self.o
        xl = o.head({3: np.asarray(x3, dtype=F32), 4: np.asarray(x4, dtype=F32)}, lv, "local_head", ref.LOCAL_LEVELS)
        desc = ref.l2_normalize(o._mlp(xl, "local_descriptor_decoder"))
        off = np.tanh(o._mlp(xl, "local_keypoint_regressor")).astype(F32)
        if ignore_kp:
            off = np.zeros_like(off)
        kp = o.quantizer.keypoint_position(lv.coords[3][:, 1:], [8, 8, 8], off)
        return {"descriptors": desc, "keypoints": kp, "sigma": ref.softplus(o._mlp(xl, "local_sigma_regressor"))}

    def global_head(self, lv, x5, x6, x7, pool="GeM", B=None):
        o = self.o
        B = lv.batch_size if B is None else B
        g = o.head({5: np.asarray(x5, dtype=F32), 6: np.asarray(x6, dtype=F32), 7: np.asarray(x7, dtype=F32)}, lv, "global_head",
                   ref.GLOBAL_LEVELS)
        g = o._mlp(g, "global_descriptor_decoder")
        return {"GeM": o.gem, "MAC": o.mac, "SPoC": o.spoc}[pool](g, lv.coords[5], B)
