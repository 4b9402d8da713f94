"""numpy restatement of the RANSAC semantics of include/fgreg.h (csrc/ransac.hip), the reference
of tests/test_gpu_ransac.py; pinned on the CPU by tests/test_ransac_ref.py.

Everything discrete is restated exactly: the counter-based hash (common.h attn_drop_hash with
head = k, q = pair, k = hypothesis) in uint64 arithmetic masked to 32 bits, the ranks
(hash * m) >> 32, the strict eligibility w > w_min, the fp32 transform and distance in the
device's operation order (_icp_ref.transform32, numpy never fuses), the strict d2 < r2 with
r2 = r * r in fp32, the first-maximum selection and the refit loop's stopping rule. The solves
are fp64 np.linalg.svd Kabsch fits rounded once to fp32, where the device runs a Jacobi SVD: the
only place the two may differ, by rounding.
"""
import numpy as np

from _icp_ref import F32, offsets, rotation, transform32  # noqa: F401

M32 = np.uint64(0xFFFFFFFF)
EYE = np.eye(3, 4, dtype=F32)


def hash32(seed, head, q, k):
    """attn_drop_hash: broadcasts over array arguments -> uint64 holding 32-bit values."""
    u = lambda v: np.asarray(v, np.int64).astype(np.uint64) & M32
    with np.errstate(over='ignore'):
        x = u(seed) ^ ((u(head) * np.uint64(0x9E3779B9)) & M32)
        x = x ^ ((u(q) * np.uint64(0x85EBCA6B)) & M32)
        x = ((x ^ (x >> np.uint64(16))) * np.uint64(0x7FEB352D)) & M32
        x = x ^ ((u(k) * np.uint64(0xC2B2AE35)) & M32)
        x = ((x ^ (x >> np.uint64(15))) * np.uint64(0x846CA68B)) & M32
        return x ^ (x >> np.uint64(16))


def ranks(seed, pair, n_hyp, m):
    """-> (n_hyp, 3) int64 ranks into the eligible rows, r_k = (hash(seed, k, pair, h) * m) >> 32."""
    h = np.arange(n_hyp)
    cols = [(hash32(seed, k, pair, h) * np.uint64(m)) >> np.uint64(32) for k in range(3)]
    return np.stack(cols, 1).astype(np.int64)


def valid_ranks(rk, m):
    return (m >= 3) & (rk[:, 0] != rk[:, 1]) & (rk[:, 0] != rk[:, 2]) & (rk[:, 1] != rk[:, 2])


def eligible(w, w_min, n):
    """Strict, in fp32; a NaN weight is not eligible."""
    if w is None:
        return np.ones(n, bool)
    return np.asarray(w, F32) > F32(w_min)


def kabsch(a, b):
    """Unweighted fp64 Kabsch of rows a -> b ((..., n, 3) each, batched) -> (..., 3, 4) float64:
    H = sum (a - am)(b - bm)^T = U S V^T, R = V diag(1, 1, det) U^T, t = bm - R am."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    am, bm = a.mean(-2, keepdims=True), b.mean(-2, keepdims=True)
    H = np.swapaxes(a - am, -1, -2) @ (b - bm)
    U, _, Vt = np.linalg.svd(H)
    V = np.swapaxes(Vt, -1, -2)
    d = np.linalg.det(V @ np.swapaxes(U, -1, -2))
    D = np.zeros(H.shape)
    D[..., 0, 0] = D[..., 1, 1] = 1.0
    D[..., 2, 2] = np.where(d < 0, -1.0, 1.0)
    R = V @ D @ np.swapaxes(U, -1, -2)
    t = bm[..., 0, :] - (R @ am[..., 0, :, None])[..., 0]
    return np.concatenate([R, t[..., None]], -1)


def d2_rows(T, a, b):
    """fp32 d2 of every row a -> b under the (3, 4) float32 pose T, the device's rounding."""
    d = transform32(T, a) - np.asarray(b, F32)
    d2 = d[:, 0] * d[:, 0]
    d2 = d2 + d[:, 1] * d[:, 1]
    d2 = d2 + d[:, 2] * d[:, 2]
    assert d2.dtype == F32
    return d2


def r2_of(r):
    return F32(r) * F32(r)


def count(T, a, b, r):
    return int((d2_rows(T, a, b) < r2_of(r)).sum())


def gap(T, a, b, r):
    """min |d2 - r2| / r2 over the rows: how far the pass is from a different inlier set."""
    if len(a) == 0:
        return np.inf
    r2 = float(r2_of(r))
    return float(np.abs(d2_rows(T, a, b).astype(np.float64) - r2).min() / r2)


def sample_poses(a, b, rk, ok):
    """The minimal solves of the valid hypotheses -> (n_hyp, 3, 4) float64 (identity elsewhere)."""
    P = np.tile(np.eye(3, 4), (len(rk), 1, 1))
    if ok.any():
        P[ok] = kabsch(np.asarray(a, F32)[rk[ok]], np.asarray(b, F32)[rk[ok]])
    return P


def hypotheses(a, b, seed, pair, n_hyp, r):
    """a, b: the ELIGIBLE rows. -> (hyp_pose (n_hyp, 3, 4) float32, hyp_count (n_hyp,) int32)."""
    m = len(a)
    rk = ranks(seed, pair, n_hyp, m) if m > 0 else np.zeros((n_hyp, 3), np.int64)
    ok = valid_ranks(rk, m) & (m >= 3)
    P = sample_poses(a, b, rk, ok).astype(F32)
    cnt = np.array([count(P[h], a, b, r) if ok[h] else -1 for h in range(n_hyp)], np.int32)
    return P, cnt


def select(hyp_count):
    """The first maximum among the valid hypotheses, -1 if there is none."""
    c = np.asarray(hyp_count)
    return int(np.argmax(c)) if (c >= 0).any() else -1


def refit(a, b, T, c, r, n_refits):
    """The local optimisation from the winner (T float32, c) over the eligible rows a, b.
    -> dict: pose (3, 4) float32, n_updates, n_inliers, rmse (fp64), inl (bool over the eligible
    rows) and gaps, one per pose whose inlier set the loop used (T of every pass, every T')."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    T = np.asarray(T, F32).copy()
    r2 = r2_of(r)
    n_updates, gaps = 0, [gap(T, a, b, r)]
    for _ in range(n_refits):
        K = d2_rows(T, a, b) < r2
        if K.sum() < 3:
            break
        Tn = kabsch(a[K], b[K]).astype(F32)
        gaps.append(gap(Tn, a, b, r))
        cn = count(Tn, a, b, r)
        if cn < c:
            break
        T = Tn
        n_updates += 1
        if cn == c:
            break
        c = cn
    d2 = d2_rows(T, a, b)
    inl = d2 < r2
    n = int(inl.sum())
    rmse = float(np.sqrt(d2[inl].astype(np.float64).sum() / n)) if n else 0.0
    return {'pose': T, 'n_updates': n_updates, 'n_inliers': n, 'rmse': rmse, 'inl': inl,
            'gaps': gaps}


def ransac(a, b, w, r, n_hyp, seed=0, n_refits=4, w_min=0.0, pair=0, start=None):
    """One pair, the whole call. start = (best_hyp, T float32, c): begin the refits from a
    given winner (the device's) instead of the restated hypotheses.
    -> dict: pose, n_inliers, n_eligible, rmse, best_hyp, n_updates, mask (all rows, bool),
    hyp_pose, hyp_count (None with start), gaps."""
    a, b = np.asarray(a, F32).reshape(-1, 3), np.asarray(b, F32).reshape(-1, 3)
    el = eligible(w, w_min, len(a))
    ae, be = a[el], b[el]
    P = cnt = None
    if start is None:
        P, cnt = hypotheses(ae, be, seed, pair, n_hyp, r)
        best = select(cnt)
        start = (best, P[best] if best >= 0 else EYE, int(cnt[best]) if best >= 0 else 0)
    best, T, c = start
    mask = np.zeros(len(a), bool)
    if best < 0:
        return {'pose': EYE.copy(), 'n_inliers': 0, 'n_eligible': int(el.sum()), 'rmse': 0.0,
                'best_hyp': -1, 'n_updates': 0, 'mask': mask, 'hyp_pose': P, 'hyp_count': cnt,
                'gaps': []}
    out = refit(ae, be, T, c, r, n_refits)
    mask[np.flatnonzero(el)[out['inl']]] = True
    return {'pose': out['pose'], 'n_inliers': out['n_inliers'], 'n_eligible': int(el.sum()),
            'rmse': out['rmse'], 'best_hyp': best, 'n_updates': out['n_updates'], 'mask': mask,
            'hyp_pose': P, 'hyp_count': cnt, 'gaps': out['gaps']}


def planted_problem(seed, m, inlier_frac, noise, r):
    """m correspondences in the cube [-1, 1]^3, round(inlier_frac * m) of them planted: b = R a + t
    plus a displacement of length <= noise (uniform direction and length); the others get a b
    drawn from the cube at least 3 r away from R a + t, so the planted set is unambiguous. The
    pose is 40 degrees about a random axis and a translation in [-0.5, 0.5]^3.
    -> (a, b float32, pose (3, 4) float64, planted (m,) bool)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (m, 3))
    R = rotation(rng.normal(size=3), 40.0)
    t = rng.uniform(-0.5, 0.5, 3)
    truth = a @ R.T + t
    planted = np.zeros(m, bool)
    planted[rng.permutation(m)[:int(round(inlier_frac * m))]] = True
    u = rng.normal(size=(m, 3))
    u *= (rng.uniform(0.0, noise, m) / np.linalg.norm(u, axis=1))[:, None]
    b = truth + u
    for i in np.flatnonzero(~planted):
        while True:
            x = rng.uniform(-1.5, 1.5, 3)
            if np.linalg.norm(x - truth[i]) >= 3.0 * r:
                b[i] = x
                break
    return a.astype(F32), b.astype(F32), np.concatenate([R, t[:, None]], 1), planted
