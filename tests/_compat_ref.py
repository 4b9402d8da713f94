"""numpy restatement of the spatial-compatibility semantics of include/fgreg.h (csrc/compat.hip),
the reference of tests/test_gpu_compat.py; pinned on the CPU by tests/test_compat_ref.py.

Everything discrete is restated exactly: the fp32 lengths in the device's operation order (numpy
never fuses, and its fp32 sqrt is correctly rounded as the device's), the strict
| la - lb | < compat_dist with a zero diagonal, the rows of 64-bit words, c = popcount(row_i &
row_j), the int32 scores, the seed order (largest s, then lowest rank) and the consensus sets
(largest c, then lowest rank). Eligibility, the fp32 count, the selection and the refit loop are
tests/_ransac_ref.py's, by import. The solves are fp64 np.linalg.svd Kabsch fits rounded once to
fp32, where the device runs a Jacobi SVD over moments: the only place the two may differ, by
rounding.
"""
import numpy as np

import _ransac_ref as rr
from _ransac_ref import EYE, F32, count, eligible, kabsch, refit, rotation, select  # noqa: F401

_POP8 = np.array([bin(v).count('1') for v in range(256)], np.int64)


def lengths32(x):
    """(m, 3) float32 -> (m, m) float32 |x_i - x_j|: dx = x_i - x_j, ((dx dx) + dy dy) + dz dz."""
    x = np.asarray(x, F32)
    d = [x[:, None, k] - x[None, :, k] for k in range(3)]
    l2 = d[0] * d[0]
    l2 = l2 + d[1] * d[1]
    l2 = l2 + d[2] * d[2]
    assert l2.dtype == F32
    return np.sqrt(l2)


def length_gaps(a, b):
    """| la - lb | (m, m) float32, the quantity compared with compat_dist."""
    with np.errstate(invalid='ignore'):
        return np.abs(lengths32(a) - lengths32(b))


def first_order(a, b, compat_dist):
    """The ELIGIBLE rows a, b -> SC (m, m) bool: strict, NaN -> 0, zero diagonal."""
    with np.errstate(invalid='ignore'):
        S = length_gaps(a, b) < F32(compat_dist)
    np.fill_diagonal(S, False)
    return S


def pack_bits(S):
    """(m, m) bool -> (m, ceil(m / 64)) uint64, bit j % 64 of word j // 64; bits past m are 0."""
    m = len(S)
    W = (m + 63) // 64
    P = np.zeros((m, W * 64), np.uint8)
    P[:, :m] = S
    by = np.packbits(P.reshape(m, W, 8, 8), axis=-1, bitorder='little')[..., 0]     # (m, W, 8)
    return np.ascontiguousarray(by).view('<u8')[..., 0] if m else np.zeros((0, 0), np.uint64)


def popcount(x):
    """Per 64-bit word."""
    x = np.ascontiguousarray(x, np.uint64)
    return _POP8[x.view(np.uint8).reshape(x.shape + (8,))].sum(-1)


def second_order(bits):
    """bits (m, W) uint64 -> (c (m, m) int64 = popcount(row_i & row_j), s (m,) int32 =
    sum_j SC_ij c_ij with SC_ij read back from the bits)."""
    m, W = bits.shape
    c = np.zeros((m, m), np.int64)
    for i0 in range(0, m, 64):
        c[i0:i0 + 64] = popcount(bits[i0:i0 + 64, None, :] & bits[None, :, :]).sum(-1)
    j = np.arange(m)
    S = ((bits[:, j // 64] >> (j % 64).astype(np.uint64)) & np.uint64(1)).astype(bool) if m else \
        np.zeros((0, 0), bool)
    s = (c * S).sum(1)
    assert s.max(initial=0) < 2 ** 31
    return c, s.astype(np.int32)


def seed_ranks(s, n_seeds):
    """The min(n_seeds, m) ranks with the largest s, ties to the lowest rank, in that order."""
    s = np.asarray(s, np.int64)
    return np.lexsort((np.arange(len(s)), -s))[:n_seeds]


def consensus(S, c, i, k):
    """Seed i's members: i and the <= k - 1 compatible ranks with the largest c_ij, ties to the
    lowest j. A set: it is returned sorted only to have one form; the device sums the members'
    moments in another fixed order, which the fp64 rounding alone could see."""
    nb = np.flatnonzero(S[i])
    nb = nb[np.lexsort((nb, -c[i, nb]))][:k - 1]
    return np.sort(np.concatenate([[i], nb])).astype(np.int64)


def seeds(a, b, compat_dist, r, n_seeds, k):
    """a, b: the ELIGIBLE rows. -> dict: S, c, s, seed_rank (n_seeds, -1 unused), members (list,
    None where invalid), seed_pose (n_seeds, 3, 4) float32, seed_count (n_seeds,) int32."""
    a, b = np.asarray(a, F32).reshape(-1, 3), np.asarray(b, F32).reshape(-1, 3)
    S = first_order(a, b, compat_dist)
    c, s = second_order(pack_bits(S))
    rank = np.full(n_seeds, -1, np.int64)
    top = seed_ranks(s, n_seeds)
    rank[:len(top)] = top
    P = np.tile(EYE, (n_seeds, 1, 1))
    cnt = np.full(n_seeds, -1, np.int32)
    members = [None] * n_seeds
    for q, i in enumerate(top):
        mem = consensus(S, c, i, k)
        if len(mem) >= 3:
            members[q] = mem
            P[q] = kabsch(a[mem], b[mem]).astype(F32)
            cnt[q] = count(P[q], a, b, r)
    return {'S': S, 'c': c, 's': s, 'seed_rank': rank, 'members': members, 'seed_pose': P,
            'seed_count': cnt}


def compat(a, b, w, compat_dist, r, n_seeds=64, k=16, n_refits=4, w_min=0.0, start=None):
    """One pair, the whole call. start = (best_seed, T float32, c): begin the refits from a given
    winner (the device's) instead of the restated one.
    -> dict: pose, n_inliers, n_eligible, rmse, best_seed, n_updates, mask (all rows, bool),
    row_score (all rows, -1 ineligible), seed_row (-1 unused), seed_pose, seed_count, members,
    gaps, first (the winner's pose and count before any refit)."""
    a, b = np.asarray(a, F32).reshape(-1, 3), np.asarray(b, F32).reshape(-1, 3)
    el = eligible(w, w_min, len(a))
    rows = np.flatnonzero(el)
    ae, be = a[el], b[el]
    sd = seeds(ae, be, compat_dist, r, n_seeds, k)
    row_score = np.full(len(a), -1, np.int32)
    row_score[rows] = sd['s']
    seed_row = np.where(sd['seed_rank'] >= 0, rows[np.maximum(sd['seed_rank'], 0)] if len(rows) else -1,
                        -1).astype(np.int32)
    if start is None:
        best = select(sd['seed_count'])
        start = (best, sd['seed_pose'][best] if best >= 0 else EYE,
                 int(sd['seed_count'][best]) if best >= 0 else 0)
    best, T, c = start
    mask = np.zeros(len(a), bool)
    out = {'n_eligible': int(el.sum()), 'best_seed': best, 'row_score': row_score,
           'seed_row': seed_row, 'seed_pose': sd['seed_pose'], 'seed_count': sd['seed_count'],
           'members': sd['members'], 'first': (np.asarray(T, F32).copy(), c)}
    if best < 0:
        out.update(pose=EYE.copy(), n_inliers=0, rmse=0.0, n_updates=0, mask=mask, gaps=[])
        return out
    fit = refit(ae, be, T, c, r, n_refits)
    mask[rows[fit['inl']]] = True
    out.update(pose=fit['pose'], n_inliers=fit['n_inliers'], rmse=fit['rmse'],
               n_updates=fit['n_updates'], mask=mask, gaps=fit['gaps'])
    return out


def planted_unit(seed, m=600, frac=0.05, sigma=0.005, r=0.03):
    """m correspondences with a in the unit cube, round(frac * m) of them planted: b = R a + t
    plus N(0, sigma^2) noise per coordinate; the others get a b drawn from the target's bounding
    box, widened by 3 r, at least 3 r away from R a + t, so the planted set is unambiguous. The pose is 40 degrees
    about a random axis and a translation in [-0.5, 0.5]^3.
    -> (a, b float32, pose (3, 4) float64, planted (m,) bool)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 1.0, (m, 3))
    R = rotation(rng.normal(size=3), 40.0)
    t = rng.uniform(-0.5, 0.5, 3)
    truth = a @ R.T + t
    lo, hi = truth.min(0) - 3.0 * r, truth.max(0) + 3.0 * r
    planted = np.zeros(m, bool)
    planted[rng.permutation(m)[:int(round(frac * m))]] = True
    b = truth + rng.normal(scale=sigma, size=(m, 3))
    for i in np.flatnonzero(~planted):
        while True:
            x = rng.uniform(lo, hi)
            if np.linalg.norm(x - truth[i]) >= 3.0 * r:
                b[i] = x
                break
    return a.astype(F32), b.astype(F32), np.concatenate([R, t[:, None]], 1), planted


def pose_errors(T, truth):
    """(rotation error in degrees, |dt|) of a (3, 4) pose against the truth."""
    T, truth = np.asarray(T, np.float64), np.asarray(truth, np.float64)
    cosv = (np.trace(T[:, :3] @ truth[:, :3].T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(cosv, -1.0, 1.0)))), float(np.linalg.norm(T[:, 3] - truth[:, 3]))
