"""TEST INFRASTRUCTURE ONLY (CPU oracle; see oracle/me_ops.py header).  numpy restatement of the retrieval part of
the reference's Evaluator.evaluate (eval/evaluate.py:66-88; identical lines in MinkLocGLEvaluator.evaluate
:168-184).  The reference's np.argsort is not stable; ties are broken by the lower map index here (kind='stable'),
which is what the HIP path defines.  Pinned on the reference's own lines: plain numpy, importable anywhere."""
import numpy as np


def knn(query_embeddings, map_embeddings, k):
    idx = np.empty((len(query_embeddings), k), dtype=np.int32)
    dist = np.empty((len(query_embeddings), k), dtype=np.float32)
    for i, q in enumerate(query_embeddings):
        embed_dist = np.linalg.norm(map_embeddings - q, axis=1)                 # eval/evaluate.py:81
        nn = np.argsort(embed_dist, kind="stable")[:k]                           # :82
        idx[i, :len(nn)], dist[i, :len(nn)] = nn, embed_dist[nn]
        idx[i, len(nn):], dist[i, len(nn):] = -1, np.inf
    return idx, dist


def recall(nn_ndx, query_positions, map_positions, radius, k):
    tp = {r: [0] * k for r in radius}
    for qi in range(len(nn_ndx)):
        valid = nn_ndx[qi][nn_ndx[qi] >= 0]                                     # a -1 tail (k > m) sits at the end
        delta = query_positions[qi] - map_positions[valid]                      # :85
        euclid_dist = np.full(k, np.inf)
        euclid_dist[:len(valid)] = np.linalg.norm(delta, axis=1)                # :86
        tp = {r: [tp[r][nn] + (1 if (euclid_dist[:nn + 1] <= r).any() else 0) for nn in range(k)] for r in radius}   # :88
    n = max(len(nn_ndx), 1)
    return {r: [tp[r][nn] / n for nn in range(k)] for r in radius}              # :91


def recall_counts(nn_ndx, query_positions, map_positions, radius, k):
    """The integers behind `recall` (:88): tp[r][nn] = number of queries with a retrieved element among the first nn+1
    within radius r.  Positions as given (feed float64); -1 entries of nn_ndx are "nothing retrieved"."""
    tp = np.zeros((len(radius), k), dtype=np.int64)
    for qi in range(len(nn_ndx)):
        row = np.asarray(nn_ndx[qi])
        euclid_dist = np.full(k, np.inf)
        ok = row >= 0
        euclid_dist[ok] = np.linalg.norm(query_positions[qi] - map_positions[row[ok]], axis=1)
        best = np.minimum.accumulate(euclid_dist)
        for ri, r in enumerate(radius):
            tp[ri] += best <= r
    return tp


U32 = 2.0 ** -24                                                                # unit roundoff of fp32


def knn_tol(d):
    """Relative error bound of one fp32 distance of knn_dist_kernel (egonn_amd/csrc/retrieval.hip), first order in
    u = 2^-24, every term of the sum being non-negative:
      row[i] - q[i] rounds once                 -> each square carries 2u
      a lane chains L = ceil(d/64) fmaf          -> L roundings on a sum of non-negative terms: L u
      the 6-step butterfly adds                  -> 6u
      sqrtf halves the relative error of its argument and rounds once (correctly rounded)
    => ((L + 8) / 2 + 1) u;  4.2e-7 at d = 256.  Comparing two such distances: twice that."""
    return ((-(-int(d) // 64) + 8) / 2.0 + 1.0) * U32


def dist64(queries, database, block=8):
    """(nq, m) float64 L2 distances in the difference form (eval/evaluate.py:81)."""
    q, db = np.asarray(queries, np.float64), np.asarray(database, np.float64)
    out = np.empty((len(q), len(db)))
    for lo in range(0, len(q), block):
        diff = db[None, :, :] - q[lo:lo + block, None, :]
        out[lo:lo + block] = np.sqrt(np.einsum("qmd,qmd->qm", diff, diff))
    return out


def knn_certificate(queries, database, got_idx, got_dist, tol):
    """Complete statement of "a valid k-nearest list up to fp32 rounding".  Returns the list of violations (empty =
    accepted).  With D = float64 distances and kk = min(k, m), per query:
      1. got_idx[:kk] distinct and in [0, m); got_idx[kk:] == -1 and got_dist[kk:] == +inf
      2. |got_dist[j] - D[got_idx[j]]| <= tol * D[got_idx[j]]
      3. D[got_idx[j]] <= D[got_idx[j+1]] * (1 + 2 tol)                     (two rounded distances were compared)
      4. neighbours whose float64 distances are EQUAL come in index order, and a row left out whose distance equals the
         last returned one has a larger index than every returned row at that distance
      5. no row left out is closer than the last returned one by more than 2 tol (relative)"""
    D = dist64(queries, database)
    got_idx, got_dist = np.asarray(got_idx), np.asarray(got_dist, np.float64)
    nq, m = D.shape
    bad = []
    if got_idx.shape != got_dist.shape or got_idx.ndim != 2 or got_idx.shape[0] != nq:
        return [f"shape {got_idx.shape} / {got_dist.shape} for {nq} queries"]
    k = got_idx.shape[1]
    kk = min(k, m)
    for qi in range(nq):
        idx, dist = got_idx[qi], got_dist[qi]
        if not ((idx[kk:] == -1).all() and np.isposinf(dist[kk:]).all()):
            bad.append(f"q{qi}: tail beyond m is not (-1, inf)")
        head = idx[:kk]
        if not ((head >= 0) & (head < m)).all():
            bad.append(f"q{qi}: index out of range {head[(head < 0) | (head >= m)][:3]}")
            continue
        if len(np.unique(head)) != kk:
            bad.append(f"q{qi}: duplicate index")
            continue
        dd = D[qi, head]
        off = np.abs(dist[:kk] - dd) > tol * dd
        if off.any():
            j = int(np.argmax(off))
            bad.append(f"q{qi}: distance[{j}] {dist[j]!r} vs {dd[j]!r}")
        inv = dd[:-1] > dd[1:] * (1 + 2 * tol)
        if inv.any():
            j = int(np.argmax(inv))
            bad.append(f"q{qi}: order: position {j} ({dd[j]!r}) after a farther row ({dd[j + 1]!r})")
        order = np.argsort(dd, kind="stable")                       # equal distances keep their positions' order
        tie = dd[order][:-1] == dd[order][1:]
        if (tie & (head[order][:-1] > head[order][1:])).any():
            bad.append(f"q{qi}: tie not in index order")
        if kk < m:
            out = np.ones(m, bool)
            out[head] = False
            rest = np.where(out, D[qi], np.inf)
            if rest.min() * (1 + 2 * tol) < dd[-1]:
                bad.append(f"q{qi}: row {int(rest.argmin())} ({rest.min()!r}) left out, last returned {dd[-1]!r}")
            for j in np.flatnonzero(out & np.isin(D[qi], dd)):
                if (head[dd == D[qi, j]] > j).any():
                    bad.append(f"q{qi}: tie at the cut: row {int(j)} left out for a larger index")
                    break
    return bad


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two floats is exact in float64; one rounding to 53 bits precedes the
    rounding to 24 (double rounding, harmless for an error-bound check)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def knn_fp32(queries, database, k, block=16):
    """numpy fp32 restatement of the arithmetic of knn_dist_kernel / knn_select_kernel: lane l sums the elements
    l, l+64, ... with fmaf, a 6-step xor butterfly joins the 64 lanes, sqrtf; selection = stable argsort of the fp32
    distances.  NaN distances are never neighbours (-1 / inf tail)."""
    q, db = np.asarray(queries, np.float32), np.asarray(database, np.float32)
    nq, m, d = len(q), len(db), q.shape[1]
    L = -(-d // 64)
    pad = L * 64 - d
    qp, dbp = np.pad(q, ((0, 0), (0, pad))), np.pad(db, ((0, 0), (0, pad)))
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for lo in range(0, nq, block):
            df = dbp[None, :, :] - qp[lo:lo + block, None, :]                    # one rounding per element
            df = df.reshape(df.shape[0], m, L, 64)
            s = np.zeros((df.shape[0], m, 64), np.float32)
            for c in range(L):
                live = np.arange(64) + 64 * c < d                                  # a lane past d does not iterate
                s = np.where(live, _fma32(df[:, :, c], df[:, :, c], s), s)
            for o in (32, 16, 8, 4, 2, 1):
                s = s + s[:, :, np.arange(64) ^ o]
            dv = np.sqrt(s[:, :, 0])
            for j in range(dv.shape[0]):
                order = np.argsort(dv[j], kind="stable")
                order = order[~np.isnan(dv[j][order])][:k]
                idx[lo + j, :len(order)], dist[lo + j, :len(order)] = order, dv[j][order]
    return idx, dist


def knn_exact_int(queries, database, k):
    """Integer-valued inputs whose squared distances stay below 2^24: every partial sum is an integer and exact in fp32
    in any order, so the kernel's answer is fixed bit for bit: fp32 sqrt of the integer sum, stable argsort."""
    q, db = np.asarray(queries, np.int64), np.asarray(database, np.int64)
    assert (q == np.asarray(queries)).all() and (db == np.asarray(database)).all()
    idx = np.full((len(q), k), -1, np.int32)
    dist = np.full((len(q), k), np.inf, np.float32)
    for i in range(len(q)):
        s = ((db - q[i]) ** 2).sum(1)
        assert s.max(initial=0) < 2 ** 24
        dv = np.sqrt(s.astype(np.float32))
        nn = np.argsort(dv, kind="stable")[:k]
        idx[i, :len(nn)], dist[i, :len(nn)] = nn, dv[nn]
    return idx, dist


def recall_floor(query_positions, map_positions, r, origin=None):
    """Smallest |distance - r| below which fp32 could flip `distance <= r` in recall_kernel, for positions
    stored as fp32 offsets from `origin` (None: the float64 mean of the map positions, as egonn_amd/retrieval.py
    subtracts).  With L = the largest |offset| coordinate, pd = position_dim, u = 2^-24:
      each stored coordinate is off by <= u L; q - m of two such by <= 2 u L, plus one rounding of the difference
      (|q - m| <= 2 L): <= 4 u L per coordinate, <= 4 sqrt(pd) u L on the distance;
      the fmaf chain (pd roundings on non-negative terms) and sqrtf: ((pd + 2) / 2 + 1) u relative on a distance
      <= 2 sqrt(pd) L, i.e. <= (pd + 4) sqrt(pd) u L;   the radius itself is rounded to fp32: u r.
    => floor(r) = (pd + 8) sqrt(pd) u L + u r."""
    qp, mp = np.asarray(query_positions, np.float64), np.asarray(map_positions, np.float64)
    if origin is None:
        origin = mp.mean(axis=0) if len(mp) else np.zeros(qp.shape[1])
    L = max(np.abs(qp - origin).max(initial=0.0), np.abs(mp - origin).max(initial=0.0))
    pd = qp.shape[1]
    return (pd + 8) * np.sqrt(pd) * U32 * L + U32 * float(r)


def recall_margin_rows(query_positions, map_positions, radius, origin=None):
    """per query: min of |distance - r| / recall_floor(r) over EVERY map row and every radius, float64 (> 1: fp32
    cannot flip any comparison of that query, whatever the kNN retrieves)."""
    qp, mp = np.asarray(query_positions, np.float64), np.asarray(map_positions, np.float64)
    out = np.full(len(qp), np.inf)
    for r in radius:
        floor = recall_floor(qp, mp, r, origin)
        for lo in range(0, len(qp), 256):
            D = np.linalg.norm(qp[lo:lo + 256, None, :] - mp[None, :, :], axis=2)
            out[lo:lo + 256] = np.minimum(out[lo:lo + 256], np.abs(D - float(r)).min(axis=1, initial=np.inf) / floor)
    return out


def recall_margin(query_positions, map_positions, radius, origin=None):
    """min of recall_margin_rows over the queries: the inputs are decidable in fp32 iff this exceeds 1"""
    return float(recall_margin_rows(query_positions, map_positions, radius, origin).min(initial=np.inf))
