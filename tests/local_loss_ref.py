"""Float64 restatement of the batched local-head loss (egonn_local_loss / BatchedKeypointCorrLoss), in this project's own words:
per pair the keypoint searches, the probabilistic chamfer and point-to-point terms, the correspondence cross-entropy, every
metric of KeypointCorrLoss and the analytic gradients to the six keypoint / sigma / descriptor arrays; over the batch the mean
loss, the mean metrics and gradients divided by the number of pairs.  Pinned to real reference outputs
(tests/golden/local_losses.npz) by tests/test_local_loss_batch_host.py; the oracle of the GPU edge batches.

Also the generator of those edge batches (`edge_batches`) and the margins that make them unambiguous in float64 (`margins`)."""
import numpy as np

STAT_KEYS = ('loss', 'kp_per_cloud', 'repeatability', 'chamfer_pure', 'chamfer_weighted', 'mean_sigma', 'loss_chamfer', 'loss_p2p',
             'keypoint_loss', 'correspondence_loss', 'matching_keypoints', 'matching_descriptors', 'pos_similarity',
             'neg_similarity')
GRAD_KEYS = ("kp1", "kp2", "sigma1", "sigma2", "desc1", "desc2")
GAMMAS = dict(gamma_chamfer=1.0, gamma_p2p=1.0, gamma_c=1.0, gamma_k=1.0, beta=2.0, dist_th=0.5)     # make_losses defaults


def _dist(a, b):
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))


def _unit(x, d):
    out = np.zeros_like(x)
    nz = d > 0
    out[nz] = x[nz] / d[nz, None]
    return out


def pair_f64(p, gammas=GAMMAS, want_margins=False):
    """one pair (dict of pc1 pc2 kp1 kp2 sigma1 sigma2 desc1 desc2 M) -> dict(stats {key: value}, grads {key: array}, ...)"""
    g = gammas
    f = {k: np.asarray(v, np.float64) for k, v in p.items()}
    kp1, kp2, s1, s2, d1, d2 = f["kp1"], f["kp2"], f["sigma1"][:, 0], f["sigma2"][:, 0], f["desc1"], f["desc2"]
    R, t = f["M"][:3, :3], f["M"][:3, 3]
    n1, n2 = len(kp1), len(kp2)
    kp1t = kp1 @ R.T + t
    D = _dist(kp1t, kp2)
    ndx1, ndx2 = D.argmin(1), D.argmin(0)                      # first minimum = lowest index
    md1, md2 = D[np.arange(n1), ndx1], D[ndx2, np.arange(n2)]
    s12, s21 = 0.5 * (s1 + s2[ndx1]), 0.5 * (s2 + s1[ndx2])
    loss1, loss2 = (np.log(s12) + md1 / s12).mean(), (np.log(s21) + md2 / s21).mean()
    st = {"kp_per_cloud": 0.5 * (n1 + n2), "repeatability": (md1 <= g["dist_th"]).mean(),
          "chamfer_pure": 0.5 * (md1.mean() + md2.mean()),
          "chamfer_weighted": 0.5 * ((1 / s12) / (1 / s12).mean() * md1).mean() + 0.5 * ((1 / s21) / (1 / s21).mean() * md2).mean(),
          "mean_sigma": 0.5 * (s12.mean() + s21.mean())}
    st["loss_chamfer"] = g["gamma_chamfer"] * 0.5 * (loss1 + loss2)
    P1, P2 = _dist(kp1, f["pc1"]), _dist(kp2, f["pc2"])
    i1, i2 = P1.argmin(1), P2.argmin(1)
    e1, e2 = P1[np.arange(n1), i1], P2[np.arange(n2), i2]
    st["loss_p2p"] = 0.5 * (e1.mean() + e2.mean())
    st["keypoint_loss"] = st["loss_chamfer"] + g["gamma_p2p"] * st["loss_p2p"]
    # correspondence term
    scale = np.exp(g["beta"])
    keep = md1 <= g["dist_th"]
    K = int(keep.sum())
    S = scale * (d1[keep] @ d2.T)
    tg = ndx1[keep]
    if K > 0:
        mx = S.max(1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(S - mx).sum(1))
        corr = (lse - S[np.arange(K), tg]).mean()
        am = S.argmax(1)
        neg = S.copy()
        neg[:, tg] = 0.0                                        # every column that is the class of ANY kept row
        st.update(matching_descriptors=float((am == tg).sum()), pos_similarity=am.astype(np.float64).mean(),   # (sic) index mean
                  neg_similarity=neg.max(1).mean())
    else:
        corr = np.nan
        st.update(matching_descriptors=0.0, pos_similarity=0.0, neg_similarity=0.0)
    st["correspondence_loss"] = corr
    st["matching_keypoints"] = float(K)
    st["loss"] = g["gamma_k"] * st["keypoint_loss"] + g["gamma_c"] * corr
    # gradients of st["loss"]
    wk = g["gamma_k"] * g["gamma_chamfer"] * 0.5
    gm1, gm2 = wk / n1 / s12, wk / n2 / s21
    gs12, gs21 = wk / n1 * (1 / s12 - md1 / s12 ** 2), wk / n2 * (1 / s21 - md2 / s21 ** 2)
    u1, u2 = _unit(kp1t - kp2[ndx1], md1), _unit(kp1t[ndx2] - kp2, md2)
    gt = gm1[:, None] * u1
    gk2 = -gm2[:, None] * u2
    np.add.at(gk2, ndx1, -gm1[:, None] * u1)
    np.add.at(gt, ndx2, gm2[:, None] * u2)
    gs1, gs2 = 0.5 * gs12, 0.5 * gs21
    np.add.at(gs2, ndx1, 0.5 * gs12)
    np.add.at(gs1, ndx2, 0.5 * gs21)
    wp = g["gamma_k"] * g["gamma_p2p"] * 0.5
    gk1 = gt @ R + wp / n1 * _unit(kp1 - f["pc1"][i1], e1)
    gk2 = gk2 + wp / n2 * _unit(kp2 - f["pc2"][i2], e2)
    gd1, gd2 = np.zeros_like(d1), np.zeros_like(d2)
    if K > 0:
        Pm = np.exp(S - lse[:, None])
        Pm[np.arange(K), tg] -= 1.0
        dS = g["gamma_c"] * scale / K * Pm
        gd1[keep] = dS @ d2
        gd2 = dS.T @ d1[keep]
    else:
        gd1[:], gd2[:] = np.nan, np.nan
    out = {"stats": st, "grads": dict(kp1=gk1, kp2=gk2, sigma1=gs1[:, None], sigma2=gs2[:, None], desc1=gd1, desc2=gd2),
           "ndx1": ndx1, "ndx2": ndx2, "i1": i1, "i2": i2, "keep": keep}
    if want_margins:
        def gap(M):                                             # relative gap of the two smallest of every row; exact ties skipped
            if M.shape[1] < 2:
                return np.inf
            two = np.partition(M, 1, axis=1)[:, :2]
            a, b = two[:, 0], two[:, 1]
            ok = b > a
            return np.min((b[ok] - a[ok]) / b[ok]) if ok.any() else np.inf
        top = np.inf
        if K > 0 and S.shape[1] > 1:
            two = -np.partition(-S, 1, axis=1)[:, :2]
            top = np.min((two[:, 0] - two[:, 1]) / np.maximum(np.abs(two[:, 0]), np.abs(two[:, 1])))
        out["margins"] = {"nn": min(gap(D), gap(D.T), gap(P1), gap(P2)), "dist_th": np.min(np.abs(md1 - g["dist_th"])),
                          "top_logit": top}
    return out


def batch_f64(pairs, gammas=GAMMAS, want_margins=False):
    """a batch -> dict(loss, stats {key: mean}, pair_stats [ {key: value} ], grads [ {key: array / len(pairs)} ], pairs [...])"""
    res = [pair_f64(p, gammas, want_margins) for p in pairs]
    n = len(pairs)
    stats = {k: np.mean([r["stats"][k] for r in res]) for k in STAT_KEYS}
    return {"loss": stats["loss"], "stats": stats, "pair_stats": [r["stats"] for r in res],
            "grads": [{k: r["grads"][k] / n for k in GRAD_KEYS} for r in res], "pairs": res}


# ----------------------------------------------------------------------------- edge batches (seeded)
# The seeds are chosen so that float64 alone decides every search, threshold and arg-max with a margin (`margins`,
# asserted by tests/test_local_loss_batch_host.py): random draws can put two neighbours within 1e-4 relative of each other.
def _edge_pair(rng, n1, n2, m1, m2, far=False, shared_class=False):
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    ang = rng.uniform(-0.6, 0.6)
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    t = rng.uniform(-3, 3, 3) * np.array([1, 1, 0.1])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    box = np.array([12.0, 12.0, 2.0])
    kp1 = rng.uniform(-1, 1, (n1, 3)) * box
    if shared_class and n1 >= 4:                               # rows 1..3 crowd around row 0: one class for several kept rows
        kp1[1:4] = kp1[0] + rng.normal(0, 0.02, (3, 3))
    ns = min(n1, n2)
    kp2 = np.concatenate([kp1[:ns] @ R.T + t + rng.normal(0, 0.05, (ns, 3)), rng.uniform(-1, 1, (n2 - ns, 3)) * box])
    if shared_class and n1 >= 4 and n2 >= 4:
        kp2[1:4] = kp2[1:4] + np.array([0.0, 0.0, 30.0])       # their own partners move away: kp2[0] is the nearest of rows 0..3
    if far:
        kp2 = kp2 + np.array([0.0, 0.0, 100.0])                # nothing within dist_th
    pc1 = rng.uniform(-1, 1, (m1, 3)) * box
    pc2 = rng.uniform(-1, 1, (m2, 3)) * box
    d1 = rng.standard_normal((n1, 128))
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    d2 = np.concatenate([d1[:ns] + 0.4 * rng.standard_normal((ns, 128)), rng.standard_normal((n2 - ns, 128))])
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    return dict(pc1=f32(pc1), pc2=f32(pc2), kp1=f32(kp1), kp2=f32(kp2), sigma1=f32(rng.uniform(0.05, 1.5, (n1, 1))),
                sigma2=f32(rng.uniform(0.05, 1.5, (n2, 1))), desc1=f32(d1), desc2=f32(d2), M=f32(M))


def _plant_cloud(p, side, kp_row, cloud_row, exact=False):
    """move cloud point `cloud_row` of a side next to (exact: onto) keypoint `kp_row`: it becomes that keypoint's nearest point"""
    kp, pc = p["kp" + side], p["pc" + side]
    pc[cloud_row] = kp[kp_row] if exact else kp[kp_row] + np.array([0.004, -0.003, 0.002], np.float32)


def edge_batches(chunk):
    """{name: (pairs, expect)}: expect lists (pair, side, keypoint row, cloud row) plants the oracle's search must return and
    the other planted facts.  `chunk` = LL_CLOUD_CHUNK."""
    out = {}
    rng = np.random.default_rng(2048)
    # ---- three pairs, uneven keypoint counts, clouds on each side of the chunk length
    a = _edge_pair(rng, 1, 65, 1, chunk - 1)
    b = _edge_pair(rng, 64, 33, chunk, chunk + 1)
    c = _edge_pair(rng, 257, 31, 3 * chunk + 7, chunk + 1)
    plants = []
    for (pi, p, side, m) in ((1, b, "1", chunk), (1, b, "2", chunk + 1), (2, c, "1", 3 * chunk + 7), (2, c, "2", chunk + 1)):
        rows = [0, m - 1, chunk - 1] + ([chunk] if m > chunk else []) + ([2 * chunk - 1, 2 * chunk, 3 * chunk] if m > 3 * chunk else [])
        for k, r in enumerate(dict.fromkeys(rows)):
            _plant_cloud(p, side, k, r)
            plants.append((pi, side, k, r))
    _plant_cloud(a, "2", 0, chunk - 2)
    plants.append((0, "2", 0, chunk - 2))
    # duplicates: kp2[12] := kp2[5] in pair c (kp1'[5] ties between them -> 5); cloud rows 40 and 900 both the nearest of kp1[20]
    c["kp2"][12] = c["kp2"][5]
    _plant_cloud(c, "1", 20, 900)
    c["pc1"][40] = c["pc1"][900]
    plants.append((2, "1", 20, 40))
    # a keypoint exactly on a cloud point: zero distance, zero point-to-point gradient
    _plant_cloud(c, "1", 30, 77, exact=True)
    plants.append((2, "1", 30, 77))
    out["three"] = ([a, b, c], {"plants": plants, "kp_tie": (2, 5, 5), "zero_p2p": (2, "1", 30)})
    # ---- eight pairs: a pair with no correspondence at position 3, shared classes at position 5, a chunk-straddling cloud
    rng = np.random.default_rng(2043)
    shapes = [(32, 63, 50, 60), (33, 64, 300, 1), (63, 32, 70, 80), (31, 1, 90, 40), (65, 257, chunk + 1, 200), (64, 65, 120, 130),
              (1, 1, 10, 10), (33, 31, 60, 50)]
    ps = [_edge_pair(rng, *s, far=(i == 3), shared_class=(i == 5)) for i, s in enumerate(shapes)]
    out["eight"] = (ps, {"nan_pair": 3, "shared_pair": 5})
    # ---- one pair
    rng = np.random.default_rng(2050)
    out["one"] = ([_edge_pair(rng, 65, 64, chunk + 1, 1)], {})
    return out


def pack(pairs):
    """the packed arrays and int32 offsets of egonn_local_loss from a list of pair dicts (numpy)"""
    cat = lambda k: np.concatenate([p[k] for p in pairs])
    off = lambda k: np.concatenate([[0], np.cumsum([len(p[k]) for p in pairs])]).astype(np.int32)
    return dict(clouds1=cat("pc1"), cloud_off1=off("pc1"), kp1=cat("kp1"), sigma1=cat("sigma1"), desc1=cat("desc1"), kp_off1=off("kp1"),
                clouds2=cat("pc2"), cloud_off2=off("pc2"), kp2=cat("kp2"), sigma2=cat("sigma2"), desc2=cat("desc2"), kp_off2=off("kp2"),
                transforms=np.stack([p["M"] for p in pairs]).astype(np.float32))
