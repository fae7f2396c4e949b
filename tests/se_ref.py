"""float64 numpy restatement of the SE gate (SELayer.fc on the per-sample means, reference layers/senet_block.py:39-49) and
of its five gradients, for the GPU test of egonn_se_gate / egonn_se_gate_backward; test_se_host.py checks it against float64
torch autograd of the same two nn.Linear layers."""
import numpy as np

SHAPES = [(1, 16), (3, 32), (5, 64), (2, 128), (67, 256)]       # (B, C): hidden 1 and 16, a batch that is no multiple of a wave


def inputs(B, c, seed, dead_sample=None):
    """seeded fp32 (mean, w1, b1, w2, b2, grad_gate).  dead_sample: every pre-ReLU value of that sample is negative (w1 >= 0,
    its means <= -0.5, |b1| small), so its hidden layer is dead and its gate is sigmoid(b2)."""
    rng = np.random.default_rng(seed)
    h = c // 16
    mean = rng.standard_normal((B, c))
    w1 = rng.standard_normal((h, c)) * np.sqrt(2.0 / c) * 2.0
    b1 = rng.standard_normal(h) * 0.1
    w2 = rng.standard_normal((c, h)) * np.sqrt(2.0 / h)
    b2 = rng.standard_normal(c) * 0.3
    gg = rng.standard_normal((B, c))
    if dead_sample is not None:
        w1 = np.abs(w1)
        mean[dead_sample] = -np.abs(mean[dead_sample]) - 0.5
    return tuple(np.ascontiguousarray(v, np.float32) for v in (mean, w1, b1, w2, b2, gg))


def forward(mean, w1, b1, w2, b2):
    """-> gate (B, C), hidden (B, H) post-ReLU, pre (B, H) pre-ReLU, all float64"""
    mean, w1, b1, w2, b2 = (np.asarray(v, np.float64) for v in (mean, w1, b1, w2, b2))
    pre = mean @ w1.T + b1
    hid = np.maximum(pre, 0.0)
    return 1.0 / (1.0 + np.exp(-(hid @ w2.T + b2))), hid, pre


def backward(grad_gate, mean, w1, b1, w2, b2):
    """-> dict of float64 gradients: mean, w1, b1, w2, b2 (ReLU backward by hidden > 0)"""
    gate, hid, _ = forward(mean, w1, b1, w2, b2)
    mean, w1, w2, gg = (np.asarray(v, np.float64) for v in (mean, w1, w2, grad_gate))
    dz2 = gg * gate * (1.0 - gate)
    dz1 = (dz2 @ w2) * (hid > 0)
    return {"mean": dz1 @ w1, "w1": dz1.T @ mean, "b1": dz1.sum(0), "w2": dz2.T @ hid, "b2": dz2.sum(0)}
