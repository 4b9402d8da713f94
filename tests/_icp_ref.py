"""numpy restatement of the ICP semantics of include/fgreg.h (csrc/icp.hip), the reference of
tests/test_gpu_icp.py; pinned on the CPU by tests/test_icp_ref.py.

What is fp32 on the device is fp32 here, in the same operation order (numpy rounds every
float32 operation once and never fuses): the transform ((R0 px + R1 py) + R2 pz) + t, the
distance ((dx dx) + dy dy) + dz dz, the radius r * r and the strict test d2 < r2. The nearest
target is found by brute force with np.argmin, whose first minimum is the lowest index: the
tie rule. Moments, fitness, rmse and the information matrix are fp64; the update is an
np.linalg.svd Kabsch, rounded to fp32 before the next pass reads it; the stopping rule is the
device's, with rel_fitness / rel_rmse rounded to fp32 as the C ABI passes them.
"""
import numpy as np

F32 = np.float32


def transform32(pose, p):
    """pose (3, 4), p (n, 3), both float32 -> q (n, 3) float32, the device's rounding."""
    T, p = np.asarray(pose, F32), np.asarray(p, F32)
    cols = [((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)]
    return np.stack(cols, 1).astype(F32)


def dist2(q, s):
    """q (n, 3), s (m, 3) float32 -> d2 (n, m) float32, dist2g's rounding."""
    d = [q[:, None, k] - s[None, :, k] for k in range(3)]
    d2 = d[0] * d[0]
    d2 = d2 + d[1] * d[1]
    d2 = d2 + d[2] * d[2]
    assert d2.dtype == F32
    return d2


def associate(src, tgt, pose, r, chunk=1024):
    """One pass -> (idx (n,) int32: nearest target row or -1, d2 (n,) float32: its d2 or +inf,
    gaps): gaps = (smallest second-nearest d2 minus nearest d2 over the source points,
    smallest |nearest d2 - r2|), +inf where undefined -- how far the pass is from a different
    discrete result."""
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    n, m = len(src), len(tgt)
    idx = np.full(n, -1, np.int32)
    d2o = np.full(n, np.inf, F32)
    gap_nn = gap_r = np.inf
    if n == 0 or m == 0:
        return idx, d2o, (gap_nn, gap_r)
    r2 = F32(r) * F32(r)
    q = transform32(pose, src)
    for a in range(0, n, chunk):
        d2 = dist2(q[a:a + chunk], tgt)
        j = np.argmin(d2, 1)                               # first minimum: the lowest index
        best = d2[np.arange(len(j)), j]
        inl = best < r2
        idx[a:a + chunk] = np.where(inl, j, -1)
        d2o[a:a + chunk] = np.where(inl, best, np.inf)
        if m >= 2:
            two = np.partition(d2.astype(np.float64), 1, axis=1)[:, :2]
            gap_nn = min(gap_nn, float((two[:, 1] - two[:, 0]).min()))
        gap_r = min(gap_r, float(np.abs(best.astype(np.float64) - float(r2)).min()))
    return idx, d2o, (gap_nn, gap_r)


def moments(src, tgt, idx, d2):
    """fp64 sums over the inliers -> (n, sum p, sum s, sum p s^T, sum d2)."""
    k = idx >= 0
    p = np.asarray(src, np.float64)[k]
    s = np.asarray(tgt, np.float64)[idx[k]]
    return int(k.sum()), p.sum(0), s.sum(0), p.T @ s, float(np.asarray(d2, np.float64)[k].sum())


def fitness_rmse(n_inl, sum_d2, n_src):
    f = n_inl / n_src if n_src > 0 else 0.0
    e = float(np.sqrt(sum_d2 / n_inl)) if n_inl > 0 else 0.0
    return f, e


def kabsch(n, sp, ss, sps):
    """The update from the moments -> (3, 4) float64: H = sum p s^T - sum p sum s^T / n,
    R = V diag(1, 1, det) U^T, t = mean s - R mean p."""
    H = sps - np.outer(sp, ss) / n
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(V @ U.T)) or 1.0])
    R = V @ D @ U.T
    t = ss / n - R @ (sp / n)
    return np.concatenate([R, t[:, None]], 1)


def solve(src, tgt, idx, d2):
    """One update from given correspondences -> (pose (3, 4) float64, fitness, rmse)."""
    n, sp, ss, sps, sd = moments(src, tgt, idx, d2)
    f, e = fitness_rmse(n, sd, len(src))
    return kabsch(n, sp, ss, sps), f, e


def information(tgt, idx):
    """sum over the inliers of J^T J, J = [I | -[s]x], translation first -> (6, 6) float64,
    from n, sum s and sum s s^T (the device's form)."""
    s = np.asarray(tgt, np.float64)[idx[idx >= 0]]
    n, ss, M = len(s), s.sum(0), s.T @ s
    A = np.array([[0.0, ss[2], -ss[1]], [-ss[2], 0.0, ss[0]], [ss[1], -ss[0], 0.0]])
    G = np.zeros((6, 6))
    G[:3, :3] = n * np.eye(3)
    G[:3, 3:] = A
    G[3:, :3] = A.T
    G[3:, 3:] = np.trace(M) * np.eye(3) - M
    return G


def information_loop(tgt, idx):
    """The same matrix point by point, from the definition."""
    G = np.zeros((6, 6))
    for j in idx[idx >= 0]:
        x, y, z = np.asarray(tgt, np.float64)[j]
        J = np.concatenate([np.eye(3), -np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])], 1)
        G += J.T @ J
    return G


def icp(src, tgt, pose, r, max_iters=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """One pair. -> dict: pose (3, 4) float32, fitness, rmse (fp64, before the fp32 store),
    n_iters, idx / d2 of the last pass run (the returned pose's), gaps: one (gap_nn, gap_r)
    per pass."""
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    T = np.asarray(pose, F32).copy()
    rel_f, rel_e = float(F32(rel_fitness)), float(F32(rel_rmse))
    n_iters, gaps = 0, []
    f_prev = e_prev = 0.0
    k = 0
    while True:
        idx, d2, gap = associate(src, tgt, T, r)
        gaps.append(gap)
        n, sp, ss, sps, sd = moments(src, tgt, idx, d2)
        f, e = fitness_rmse(n, sd, len(src))
        converged = k >= 1 and abs(f - f_prev) < rel_f and abs(e - e_prev) < rel_e
        f_prev, e_prev = f, e
        if converged or n < 3 or k == max_iters:
            break
        T = kabsch(n, sp, ss, sps).astype(F32)
        n_iters = k + 1
        k += 1
    return {'pose': T, 'fitness': f, 'rmse': e, 'n_iters': n_iters, 'idx': idx, 'd2': d2,
            'gaps': gaps}


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def pack(clouds):
    """list of (n_i, 3) -> (packed (N, 3) float32, offsets int64)."""
    lens = [len(c) for c in clouds]
    rows = [np.asarray(c, F32).reshape(-1, 3) for c in clouds]
    return np.concatenate(rows).astype(F32).reshape(-1, 3), offsets(lens)


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def loop_problem(seed):
    """The whole-loop input: a 10^3 lattice of pitch 0.1 jittered by +-0.02 as the target, 600
    of its points with sigma 0.002 noise as the source, an initial pose 8 degrees and +-0.04
    off the identity, r = 0.06. -> (src, tgt, pose0 (3, 4) float32, r)."""
    rng = np.random.default_rng(seed)
    g = np.arange(10) * 0.1
    tgt = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    tgt = (tgt + rng.uniform(-0.02, 0.02, tgt.shape)).astype(F32)
    pick = rng.choice(len(tgt), 600, replace=False)
    src = (tgt[pick].astype(np.float64) + rng.normal(0.0, 0.002, (600, 3))).astype(F32)
    R = rotation(rng.normal(size=3), 8.0)
    c = tgt.astype(np.float64).mean(0)
    t = c - R @ c + rng.uniform(-0.04, 0.04, 3)           # the rotation is about the centroid
    return src, tgt, np.concatenate([R, t[:, None]], 1).astype(F32), 0.06
