"""Numpy restatement of the feature matcher (include/fgreg.h "feature matching": fgr_feature_nn,
fgr_match_pairs), in fp64 unless said otherwise. Pinned to the reference's matching utilities by
tests/test_match_ref.py (fixture tests/golden/match_ref.npz); the GPU tests compare the kernels
against it. Not a test module."""
import numpy as np

DOT, EUCLID = 0, 1
SRC, MUTUAL, BILATERAL = 0, 1, 2


# ---- inputs -----------------------------------------------------------------------------------
def descriptors(seed, ns, nt, d, noise=0.5):
    """The one seeded recipe of the tests: unit-norm Gaussian source rows; target rows are
    copies of randomly chosen source rows plus Gaussian noise of norm ~ `noise`, renormalised;
    both rounded to fp32. -> src (ns, d), tgt (nt, d), pick (nt,) the copied source rows."""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((ns, d))
    src /= np.linalg.norm(src, axis=1, keepdims=True)
    pick = rng.integers(0, ns, nt)
    tgt = src[pick] + rng.standard_normal((nt, d)) * (noise / np.sqrt(d))
    tgt /= np.linalg.norm(tgt, axis=1, keepdims=True)
    return src.astype(np.float32), tgt.astype(np.float32), pick


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


# ---- fgr_feature_nn ---------------------------------------------------------------------------
def scores(q, k, metric):
    """(n_q, n_k) fp64 scores: q . k (DOT), q . k - |k|^2 / 2 (EUCLID)."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    s = q @ k.T
    if metric == EUCLID:
        s = s - 0.5 * (k * k).sum(1)[None, :]
    return s


def feature_nn(q, k, metric):
    """One segment -> nn (int32; the lowest index among equal scores, -1 without keys), best,
    second (the outputs: scores for DOT, squared distances max(0, |q|^2 - 2 s) for EUCLID;
    -inf / +inf where there is no such key), gap (best - second-best score, inf with < 2 keys)."""
    q = np.asarray(q, np.float64)
    n_q, n_k = len(q), len(k)
    ninf = np.full(n_q, -np.inf)
    if n_k == 0:
        nn, sb, ss = np.full(n_q, -1, np.int32), ninf, ninf
    else:
        s = scores(q, k, metric)
        nn = s.argmax(1).astype(np.int32)                    # numpy: the first maximum
        sb = s[np.arange(n_q), nn]
        if n_k > 1:
            s2 = s.copy()
            s2[np.arange(n_q), nn] = -np.inf
            ss = s2.max(1)
        else:
            ss = ninf
    gap = sb - ss if n_k > 1 else np.full(n_q, np.inf)
    if metric == EUCLID:
        q2 = (q * q).sum(1)
        best, second = np.maximum(0.0, q2 - 2 * sb), np.maximum(0.0, q2 - 2 * ss)
    else:
        best, second = sb, ss
    return nn, best, second, gap


def packed_nn(feats, lengths_src, lengths_tgt, metric, queries=None):
    """The packed batch of the forward: rows [src clouds ; tgt clouds], segment c matched
    against segment (c + B) % 2B. -> nn, best, second, gap over all rows, and `scale` =
    |q| max|k| per row (what the score bound is relative to)."""
    off = offsets(list(lengths_src) + list(lengths_tgt))
    B = len(lengths_src)
    queries = feats if queries is None else queries
    outs = []
    for c in range(2 * B):
        o = (c + B) % (2 * B)
        q, k = queries[off[c]:off[c + 1]], feats[off[o]:off[o + 1]]
        nn, best, second, gap = feature_nn(q, k, metric)
        kn = np.linalg.norm(np.asarray(k, np.float64), axis=1).max() if len(k) else 0.0
        outs.append((nn, best, second, gap, np.linalg.norm(np.asarray(q, np.float64), axis=1) * kn))
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(5))


def score_of(q, k, metric, idx):
    """fp64 score of key idx[r] for query r (idx >= 0)."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)[idx]
    s = (q * k).sum(1)
    return s - 0.5 * (k * k).sum(1) if metric == EUCLID else s


# ---- fgr_match_pairs --------------------------------------------------------------------------
def match_pairs(nn_src, nn_tgt, src_xyz, tgt_xyz, mode, max_ratio=0.0, best_src=None,
                second_src=None, best_tgt=None, second_tgt=None):
    """One pair -> a, b (ns + nt, 3) fp32, w (ns + nt,) fp32, n_match. The ratio test is the
    fp32 comparison best < (max_ratio * max_ratio) * second on the given values."""
    ns, nt = len(nn_src), len(nn_tgt)
    src_xyz = np.asarray(src_xyz, np.float32).reshape(ns, 3)
    tgt_xyz = np.asarray(tgt_xyz, np.float32).reshape(nt, 3)
    a, b = np.zeros((ns + nt, 3), np.float32), np.zeros((ns + nt, 3), np.float32)
    w = np.zeros(ns + nt, np.float32)
    r2 = np.float32(max_ratio) * np.float32(max_ratio)
    for i in range(ns):
        n = int(nn_src[i]) if 0 <= nn_src[i] < nt else -1
        a[i] = src_xyz[i]
        if n < 0:
            continue
        b[i] = tgt_xyz[n]
        on = mode != MUTUAL or nn_tgt[n] == i
        if on and max_ratio > 0:
            on = np.float32(best_src[i]) < r2 * np.float32(second_src[i])
        w[i] = 1.0 if on else 0.0
    for j in range(nt):
        n = int(nn_tgt[j]) if 0 <= nn_tgt[j] < ns else -1
        b[ns + j] = tgt_xyz[j]
        if n < 0:
            continue
        a[ns + j] = src_xyz[n]
        on = mode == BILATERAL
        if on and max_ratio > 0:
            on = np.float32(best_tgt[j]) < r2 * np.float32(second_tgt[j])
        w[ns + j] = 1.0 if on else 0.0
    return a, b, w, int(w.sum())


def index_pairs(nn_src, nn_tgt, w):
    """The (source index, target index) pairs of the w > 0 rows, in row order."""
    ns = len(nn_src)
    rows = np.flatnonzero(np.asarray(w) > 0)
    return [(int(r), int(nn_src[r])) if r < ns else (int(nn_tgt[r - ns]), int(r - ns)) for r in rows]


def residual2_f32(a, b, pose):
    """|R a + t - b|^2 as the kernel writes it out, fp32 without FMA:
    qx = ((R00 x + R01 y) + R02 z) + tx, d = q - b, d2 = ((dx dx) + dy dy) + dz dz."""
    P = np.asarray(pose, np.float32).reshape(3, 4)
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = []
    for r in range(3):
        qr = ((P[r, 0] * a[:, 0] + P[r, 1] * a[:, 1]) + P[r, 2] * a[:, 2]) + P[r, 3]
        d.append(qr - b[:, r])
    return ((d[0] * d[0]) + d[1] * d[1]) + d[2] * d[2]


def inliers_f32(a, b, w, pose, inlier_dist):
    """-> the count of w > 0 rows with d2 < r2 in the written-out fp32 arithmetic, and the
    smallest |d2 - r2| / r2 over those rows (the exact comparison's precondition)."""
    r2 = np.float32(inlier_dist) * np.float32(inlier_dist)
    on = np.asarray(w) > 0
    d2 = residual2_f32(a, b, pose)[on]
    gap = float(np.abs(d2.astype(np.float64) - float(r2)).min() / float(r2)) if on.any() else np.inf
    return int((d2 < r2).sum()), gap


def inliers(a, b, w, pose, inlier_dist):
    """The fp64 count."""
    P = np.asarray(pose, np.float64).reshape(3, 4)
    on = np.asarray(w) > 0
    q = np.asarray(a, np.float64)[on] @ P[:, :3].T + P[:, 3]
    return int((((q - np.asarray(b, np.float64)[on]) ** 2).sum(1) < float(inlier_dist) ** 2).sum())


# ---- the near-tie condition -------------------------------------------------------------------
def excused(q, k, metric, nn_dev, bound):
    """Rows whose device index may differ from the restatement's: the fp64 gap between best and
    second-best score is below 2 * bound * |q| max|k|, and the key the device chose scores within
    bound * |q| max|k| of the best. -> (differs, excusable) boolean arrays."""
    nn, _, _, gap = feature_nn(q, k, metric)
    differs = nn != nn_dev
    if not differs.any():
        return differs, differs.copy()
    scale = np.linalg.norm(np.asarray(q, np.float64), axis=1) * \
        np.linalg.norm(np.asarray(k, np.float64), axis=1).max()
    ok_idx = (nn_dev >= 0) & (nn_dev < len(k))
    got = np.where(ok_idx, nn_dev, 0)
    lost = score_of(q, k, metric, nn) - score_of(q, k, metric, got)
    return differs, differs & ok_idx & (gap < 2 * bound * scale) & (lost <= bound * scale)
