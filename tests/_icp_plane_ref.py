"""numpy restatement of the normals and point-to-plane ICP semantics of include/fgreg.h
(csrc/normals.hip: fgr_estimate_normals, csrc/icp.hip: fgr_icp_plane), the reference of
tests/test_gpu_icp_plane.py; pinned on the CPU by tests/test_icp_plane_ref.py.

What is fp32 on the device is fp32 here, in the same operation order (tests/_icp_ref.py): the
transform, the distance, r * r and the strict test d2 < r2, the differences d = s - p of the
normals' moments. Sums are fp64 (numpy's order, not the device's: the two differ by fp64
rounding). The eigenvector comes from np.linalg.eigh and the update from np.linalg.solve; the
singular test is the device's Cholesky pivot rule, restated.
"""
import numpy as np

from _icp_ref import F32, associate, dist2, fitness_rmse, pack, rotation, transform32  # noqa: F401

CONVERGED, MAX_ITERS, FEW_INLIERS, SINGULAR = 0, 1, 2, 3
MIN_INLIERS = 6


# ---------------------------------------------------------------------------------------------
# normals
# ---------------------------------------------------------------------------------------------
def normals(pts, radius, view=None, chunk=1024):
    """One cloud. -> dict: normals (n, 3) float32 ((0, 0, 0) where invalid), valid (n,) bool,
    count (n,) neighbours (the point itself included), gap (n,) = the eigen-gap
    (l1 - l0) / l2 of the covariance (0 where l2 <= 0 or invalid), evals (n, 3) = l0 <= l1 <= l2,
    margin (n,) =
    |normal . (view - p)| / |view - p| (0 where view = p or invalid): how far the sign is from
    flipping."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    n = len(pts)
    view = np.zeros(3) if view is None else np.asarray(view, F32).astype(np.float64)
    out = np.zeros((n, 3), F32)
    valid = np.zeros(n, bool)
    count = np.zeros(n, np.int64)
    gap, margin, evals = np.zeros(n), np.zeros(n), np.zeros((n, 3))
    r2 = F32(radius) * F32(radius)
    for a in range(0, n, chunk):
        near = dist2(pts[a:a + chunk], pts) < r2
        for i in range(a, min(a + chunk, n)):
            d = (pts[near[i - a]] - pts[i]).astype(np.float64)      # fp32 difference, then fp64
            count[i] = len(d)
            if len(d) < 3:
                continue
            m = d.sum(0) / len(d)
            C = d.T @ d / len(d) - np.outer(m, m)
            w, V = np.linalg.eigh(C)
            v = V[:, 0] / np.linalg.norm(V[:, 0])
            to_view = view - pts[i].astype(np.float64)
            dot = float(v @ to_view)
            if dot < 0 or (dot == 0 and v[np.flatnonzero(v)[0]] < 0):
                v = -v
            out[i] = v.astype(F32)
            valid[i] = True
            evals[i] = w
            gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
            nv = np.linalg.norm(to_view)
            margin[i] = abs(dot) / nv if nv > 0 else 0.0
    return {'normals': out, 'valid': valid, 'count': count, 'gap': gap, 'margin': margin,
            'evals': evals}


def comparable(ref, gap_min=0.05, margin_min=1e-6):
    """The normals a device result is compared on: the eigenvector is determined (gap) and so
    is its sign (margin)."""
    return ref['valid'] & (ref['gap'] >= gap_min) & (ref['margin'] >= margin_min)


# ---------------------------------------------------------------------------------------------
# point-to-plane ICP
# ---------------------------------------------------------------------------------------------
def inliers(idx, nrm):
    """idx of associate() with the candidates whose target has the zero normal removed."""
    idx = np.asarray(idx, np.int32).copy()
    k = idx >= 0
    nrm = np.asarray(nrm, F32).reshape(-1, 3)
    idx[k] = np.where((nrm[idx[k]] == 0).all(1), -1, idx[k])
    return idx


def terms(src, tgt, nrm, pose, idx, d2):
    """fp64 sums over the inliers (idx already filtered by inliers()) ->
    (n, sum d2, sum rho^2, A = sum a a^T (6, 6), g = sum a rho (6,)), a = [n | q x n],
    rho = n . (q - s), from the fp32 q = T p, s and n."""
    k = idx >= 0
    q = transform32(pose, np.asarray(src, F32)[k]).astype(np.float64)
    s = np.asarray(tgt, np.float64).reshape(-1, 3)[idx[k]]
    nn = np.asarray(nrm, F32).reshape(-1, 3).astype(np.float64)[idx[k]]
    rho = (nn * (q - s)).sum(1)
    a = np.concatenate([nn, np.cross(q, nn)], 1)
    return (int(k.sum()), float(np.asarray(d2, np.float64)[k].sum()), float((rho * rho).sum()),
            a.T @ a, a.T @ rho)


def cholesky_ok(A):
    """The device's singular test: False where a pivot of the Cholesky factorisation is
    <= 1e-12 trace(A)."""
    L = np.zeros((6, 6))
    tr = np.trace(A)
    for j in range(6):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 1e-12 * tr:
            return False
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return True


def exp_so3(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def update(pose, A, g):
    """T <- [dR R | dR t + x_t] from the fp32 pose -> (3, 4) float64."""
    x = np.linalg.solve(A, -g)
    dR = exp_so3(x[3:])
    T = np.asarray(pose, F32).astype(np.float64)
    return np.concatenate([dR @ T[:, :3], (dR @ T[:, 3] + x[:3])[:, None]], 1)


def measures(n, sd2, srho2, n_src):
    f, e = fitness_rmse(n, sd2, n_src)
    return f, e, (float(np.sqrt(srho2 / n)) if n > 0 else 0.0)


def step(src, tgt, nrm, pose, idx, d2, k=0, max_iters=1, prev=None, rel_f=0.0, rel_e=0.0):
    """Pass k from given (filtered) correspondences -> dict: fitness, rmse, plane_rmse, info,
    status (None while the pair goes on), pose (the next one, float64, or None)."""
    n, sd2, srho2, A, g = terms(src, tgt, nrm, pose, idx, d2)
    f, e, pe = measures(n, sd2, srho2, len(src))
    status = None
    if k >= 1 and prev is not None and abs(f - prev[0]) < rel_f and abs(e - prev[1]) < rel_e:
        status = CONVERGED
    elif n < MIN_INLIERS:
        status = FEW_INLIERS
    elif not cholesky_ok(A):
        status = SINGULAR
    elif k == max_iters:
        status = MAX_ITERS
    return {'fitness': f, 'rmse': e, 'plane_rmse': pe, 'info': A, 'n': n, 'status': status,
            'pose': update(pose, A, g) if status is None else None}


def icp_plane(src, tgt, nrm, pose, r, max_iters=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """One pair. -> dict: pose (3, 4) float32, fitness, rmse, plane_rmse (fp64, before the fp32
    store), n_iters, status, info, idx / d2 of the last pass run (the returned pose's; idx
    without the zero-normal candidates), gaps: one (gap_nn, gap_r) per pass, as associate."""
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    T = np.asarray(pose, F32).copy()
    rel_f, rel_e = float(F32(rel_fitness)), float(F32(rel_rmse))
    n_iters, gaps, prev, k = 0, [], None, 0
    while True:
        idx, d2, gap = associate(src, tgt, T, r)
        idx = inliers(idx, nrm)
        gaps.append(gap)
        st = step(src, tgt, nrm, T, idx, d2, k, max_iters, prev, rel_f, rel_e)
        prev = (st['fitness'], st['rmse'])
        if st['status'] is not None:
            break
        T = st['pose'].astype(F32)
        n_iters = k + 1
        k += 1
    return {'pose': T, 'fitness': st['fitness'], 'rmse': st['rmse'], 'plane_rmse': st['plane_rmse'],
            'n_iters': n_iters, 'status': st['status'], 'info': st['info'], 'idx': idx, 'd2': d2,
            'gaps': gaps}


def pose_errors(pose, truth):
    """(rotation angle in degrees, translation distance) of pose against truth, both (3, 4)."""
    P, G = np.asarray(pose, np.float64), np.asarray(truth, np.float64)
    c = (np.trace(P[:, :3] @ G[:, :3].T) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1)))), float(np.linalg.norm(P[:, 3] - G[:, 3]))


# ---------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------
ROOM_R, ROOM_NORMAL_RADIUS = 0.08, 0.06
# the whole-loop inputs: room_problem(seed, *LOOP_SIZES) with normals from LOOP_NORMAL_RADIUS, the
# seeds of 0..39 whose every pass stays >= 4e-5 r from a different discrete result in the
# restatement (fewer points than the default: the smallest gap shrinks with their number)
LOOP_SEEDS, LOOP_SIZES, LOOP_NORMAL_RADIUS = (0, 4, 12, 14, 28, 38), (1000, 120), 0.1
# the benefit inputs: room_problem(seed) at the default sizes, seeds of 0..11 on which the
# restatement's point-to-plane error after 10 updates is < 1/10 of point-to-point's
BENEFIT_SEEDS = (5, 10, 11)


def _room_sample(rng, n):
    """n points of the scene: the three walls x = -0.5, y = -0.5, z = -0.5 of a unit corner and
    a slanted 0.6 x 0.5 board inside it, by area, with 2 mm noise. The origin (the normals'
    viewpoint) is the room's centre and lies on none of the four planes."""
    u = rng.uniform(-0.5, 0.5, (n, 2))
    which = rng.choice(4, n, p=np.array([1, 1, 1, 0.3]) / 3.3)
    pts = np.empty((n, 3))
    for ax in range(3):
        k = which == ax
        pts[k] = np.insert(u[k], ax, -0.5, axis=1)
    k = which == 3
    board = np.stack([0.6 * u[k, 0], 0.5 * u[k, 1], np.zeros(k.sum())], 1)
    pts[k] = board @ rotation([1, -1, 0.3], 35.0).T + np.array([0.1, 0.05, -0.2])
    return pts + rng.normal(0.0, 0.002, pts.shape)


def room_problem(seed, n_tgt=3000, n_src=1500):
    """Source and target are independent samples of the scene, so no source point has its own
    copy in the target. The source is the sample moved by the inverse of `truth`; the start is
    4 degrees and +-0.03 off the truth. -> (src, tgt, pose0 (3, 4) float32, truth (3, 4)
    float64, r)."""
    rng = np.random.default_rng(seed)
    tgt = _room_sample(rng, n_tgt).astype(F32)
    R = rotation(rng.normal(size=3), 25.0)
    t = rng.uniform(-0.3, 0.3, 3)
    src = ((_room_sample(rng, n_src) - t) @ R).astype(F32)             # R^T (x - t)
    dR = rotation(rng.normal(size=3), 4.0)
    pose0 = np.concatenate([dR @ R, (dR @ t + rng.uniform(-0.03, 0.03, 3))[:, None]], 1)
    return src, tgt, pose0.astype(F32), np.concatenate([R, t[:, None]], 1), ROOM_R


def plane_only(seed, n_tgt=400, n_src=150):
    """One exact plane z = 0.25 with the exact normals (0, 0, 1): sum a a^T has rank 3 and its
    first pivot is exactly 0, the singular case. -> (src, tgt, tgt_normals, pose0, r)."""
    rng = np.random.default_rng(seed)
    tgt = np.concatenate([rng.uniform(0, 1, (n_tgt, 2)), np.full((n_tgt, 1), 0.25)], 1).astype(F32)
    src = np.concatenate([rng.uniform(0.1, 0.9, (n_src, 2)), np.full((n_src, 1), 0.26)], 1).astype(F32)
    nrm = np.tile(np.array([0, 0, 1], F32), (n_tgt, 1))
    return src, tgt, nrm, np.eye(3, 4, dtype=F32), 0.1


def patch(n, seed, noise=0.004):
    """n points of a tilted unit-square patch about (0.4, -0.3, 1.2) with `noise` off the plane:
    the origin is 1.2 from it and on neither side's boundary."""
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), rng.normal(0.0, noise, (n, 1))], 1)
    return (p @ rotation([2, 1, 0.5], 28.0).T + np.array([0.4, -0.3, 1.2])).astype(F32)


def lattice_slab(seed, m=24):
    """An m x m lattice of pitch 0.1 in the plane z = 0.8, jittered by +-0.02 in x, y and z (the
    jitter of _icp_ref.loop_problem's lattice, on one layer: a surface, so the normal exists)."""
    rng = np.random.default_rng(seed)
    g = np.arange(m) * 0.1
    p = np.stack(np.meshgrid(g, g, [0.8], indexing='ij'), -1).reshape(-1, 3)
    return (p + rng.uniform(-0.02, 0.02, p.shape)).astype(F32)


def normals_cases():
    """name -> (clouds, radius, view (n_clouds, 3) float32 or None): the inputs of the normals
    tests. tests/test_icp_plane_ref.py asserts, on the restatement alone, that at least 90 % of
    every cloud's valid normals are comparable()."""
    cases = {f'n{n}': ([patch(n, 100 + n)], 2.0 if n <= 3 else 0.45, None)     # 3: all neighbours
             for n in (1, 2, 3, 31, 32, 33, 65)}
    cases['ragged'] = ([patch(70, 1), np.zeros((0, 3), F32), patch(33, 2)], 0.4, None)
    dup = patch(60, 3)
    dup[40:50] = dup[:10]                                   # ten exact duplicates
    dup[50:54] = dup[50] + np.float32(3.0)                  # four copies of one far point: C = 0
    cases['duplicates'] = ([dup], 0.4, None)
    iso = patch(50, 4)
    iso[17] += np.float32(5.0)                              # no neighbour but itself
    iso[18] += np.float32(-7.0)
    iso[19] = iso[18] + np.float32(0.01)                    # a pair: two neighbours each
    cases['isolated'] = ([iso], 0.4, None)
    cases['lattice-r0.13'] = ([lattice_slab(5)], 0.13, None)
    cases['lattice-r0.36'] = ([lattice_slab(5)], 0.36, None)
    view = np.array([[0.3, -2.0, 1.5], [-1.0, 0.5, 4.0]], F32)
    cases['viewpoint'] = ([patch(80, 6), lattice_slab(7, 12)], 0.3, view)
    return cases
