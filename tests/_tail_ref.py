"""fp64 references and input generators for the loss / pose / metric kernels (csrc/loss.hip,
csrc/pose.hip) -- TEST INFRASTRUCTURE ONLY, imported by tests/test_tail_ref.py (CPU: pins these
references to the oracle and the golden fixtures, and checks the generators' conditions) and
tests/test_gpu_tail_kernels.py (GPU: the kernels row by row against them).

Every reference is a plain restatement of include/fgreg.h's contract (and of what
oracle/loss_oracle.py states for the same operation) in float64 on the CPU: numpy, and torch
where autograd is wanted. Packed layouts as the C ABI: pair b owns anchor rows
a_off[b]..a_off[b+1] and positive rows / logit columns p_off[b]..p_off[b+1].
Not a conftest and not collected (no test_ prefix).
"""
import math

import numpy as np
import torch

R_P, R_N = 0.12, 0.24                     # the ModelNet configuration's radii
CIRCLE_SCALE, CIRCLE_POS, CIRCLE_NEG = 10.0, 0.1, 1.4


def _f64(a):
    return np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)


def offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)


def point_dist(a, p):
    """Euclidean distances (n_a, n_p) by direct differences."""
    a, p = _f64(a), _f64(p)
    return np.sqrt(((a[:, None, :] - p[None, :, :]) ** 2).sum(-1))


# ---- InfoNCE ------------------------------------------------------------------------------
def _infonce_torch(logits, axyz, pxyz, a_off, p_off, r_p, r_n):
    """-> (pos (n_a,) int64 column or -1, mask (n_a,) bool, row_loss (n_a,) tensor,
    scalar tensor); logits a float64 tensor (n_a, n_cols), possibly requiring grad."""
    n_a, n_pairs = logits.shape[0], len(a_off) - 1
    pos = np.full(n_a, -1, np.int64)
    mask = np.zeros(n_a, bool)
    row_loss = [None] * n_a
    pair_terms = []
    for b in range(n_pairs):
        a0, a1, p0, p1 = int(a_off[b]), int(a_off[b + 1]), int(p_off[b]), int(p_off[b + 1])
        if p1 <= p0:                                    # empty positive cloud: NaN rows, unkept
            for i in range(a0, a1):
                row_loss[i] = logits.new_tensor(math.nan)
            pair_terms.append(logits.new_tensor(math.nan))
            continue
        if a1 <= a0:                                    # no anchor: 0 / 0
            pair_terms.append(logits.new_tensor(math.nan))
            continue
        dist = point_dist(axyz[a0:a1], pxyz[p0:p1])
        j1 = dist.argmin(1)                             # first (lowest) index on ties
        d1 = dist[np.arange(a1 - a0), j1]
        keep = d1 < r_p
        excl = dist < r_n
        excl[np.arange(a1 - a0), j1] = False
        blk = logits[a0:a1, p0:p1].masked_fill(torch.from_numpy(excl), -math.inf)
        rows = torch.arange(a1 - a0)
        per_row = torch.logsumexp(blk, 1) - blk[rows, torch.from_numpy(j1)]
        pos[a0:a1] = p0 + j1
        mask[a0:a1] = keep
        for k in range(a1 - a0):
            row_loss[a0 + k] = per_row[k]
        kt = torch.from_numpy(keep)
        pair_terms.append(per_row[kt].sum() / kt.sum())          # 0 / 0 = NaN for no kept row
    rl = torch.stack(row_loss) if n_a else logits.new_zeros(0)
    return pos, mask, rl, torch.stack(pair_terms).mean()


def infonce_rows(logits, axyz, pxyz, a_off, p_off, r_p=R_P, r_n=R_N):
    """Per anchor row: the positive's column (lowest index on ties, -1 for an empty positive
    cloud), row_mask (nearest positive closer than r_p) and row_loss = logsumexp over the
    pair's columns without the other points closer than r_n, minus the positive's logit (NaN
    for an empty positive cloud). And the reduced scalar: sum(loss[mask]) / sum(mask) per
    pair, then the mean over pairs (NaN as soon as one pair has no kept row)."""
    lt = torch.from_numpy(np.nan_to_num(_f64(logits), nan=0.0))
    pos, mask, rl, s = _infonce_torch(lt, axyz, pxyz, a_off, p_off, r_p, r_n)
    return pos, mask, rl.numpy(), float(s)


def infonce_dlogits(logits, axyz, pxyz, a_off, p_off, g, r_p=R_P, r_n=R_N):
    """g * d(scalar) / d(logits), dense (n_a, n_cols), by autograd on the restatement. The
    gradient passes through the finite pairs only (an empty selection hands none on, as the
    reference's NaN pair does), so it is finite even where the scalar is NaN."""
    lt = torch.from_numpy(np.nan_to_num(_f64(logits), nan=0.0)).requires_grad_(True)
    n_pairs = len(a_off) - 1
    pos, mask, rl, _ = _infonce_torch(lt, axyz, pxyz, a_off, p_off, r_p, r_n)
    total = lt.sum() * 0.0
    mt = torch.from_numpy(mask)
    for b in range(n_pairs):
        sl = slice(int(a_off[b]), int(a_off[b + 1]))
        if mask[sl].any():
            total = total + rl[sl][mt[sl]].sum() / int(mask[sl].sum()) / n_pairs
    total.backward()
    return g * lt.grad.numpy()


def infonce_row_weight(mask, a_off):
    """row_mask / (kept rows of the pair * n_pairs), 0 for a pair without a kept row: what
    fgreg.loss hands fgr_infonce_rows_bwd, in float32 as it computes it."""
    n_pairs = len(a_off) - 1
    w = np.zeros(len(mask), np.float32)
    for b in range(n_pairs):
        sl = slice(int(a_off[b]), int(a_off[b + 1]))
        k = np.float32(mask[sl].sum())
        if k > 0:
            w[sl] = mask[sl].astype(np.float32) / (k * np.float32(n_pairs))
    return w


# ---- circle loss ----------------------------------------------------------------------------
def pair_cdist(af, pf, a_off, p_off):
    """List over pairs of sqrt(sum_k (a_ik - p_jk)^2 + 1e-12), (n_a(b), n_p(b))."""
    af, pf = _f64(af), _f64(pf)
    out = []
    for b in range(len(a_off) - 1):
        a, p = af[a_off[b]:a_off[b + 1]], pf[p_off[b]:p_off[b + 1]]
        out.append(np.sqrt(((a[:, None, :] - p[None, :, :]) ** 2).sum(-1) + 1e-12))
    return out


def _lse(x, axis):
    m = x.max(axis, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis, keepdims=True))).squeeze(axis)


def _softplus(x):                                       # F.softplus: identity above 20
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def circle_lines(af, pf, axyz, pxyz, a_off, p_off, r_p=R_P, r_n=R_N):
    """-> (list over pairs of (row_loss, row_sel, col_loss, col_sel), scalar). A line's loss is
    softplus(lse(tp) + lse(tn)) / 10 with tp = 10 (fd - 0.1) max(fd - 0.1, 0) on the positives
    (point distance < r_p) and 0 elsewhere, tn = 10 (1.4 - fd) max(1.4 - fd, 0) on the negatives
    (> r_n) and 0 elsewhere; a line is selected when it holds a positive and a negative. Pair
    loss = (mean of selected rows + mean of selected columns) / 2 (NaN for an empty selection),
    the scalar the mean over pairs."""
    fds = pair_cdist(af, pf, a_off, p_off)
    lines, terms = [], []
    for b, fd in enumerate(fds):
        na, npos = fd.shape
        if na == 0 or npos == 0:
            nan = lambda n: np.full(n, np.nan)
            lines.append((nan(na), np.zeros(na, bool), nan(npos), np.zeros(npos, bool)))
            terms.append(np.nan)
            continue
        cd = point_dist(_f64(axyz)[a_off[b]:a_off[b + 1]], _f64(pxyz)[p_off[b]:p_off[b + 1]])
        pos, neg = cd < r_p, cd > r_n
        tp = np.where(pos, CIRCLE_SCALE * (fd - CIRCLE_POS) * np.maximum(fd - CIRCLE_POS, 0), 0.0)
        tn = np.where(neg, CIRCLE_SCALE * (CIRCLE_NEG - fd) * np.maximum(CIRCLE_NEG - fd, 0), 0.0)
        row = _softplus(_lse(tp, 1) + _lse(tn, 1)) / CIRCLE_SCALE
        col = _softplus(_lse(tp, 0) + _lse(tn, 0)) / CIRCLE_SCALE
        rs, cs = pos.any(1) & neg.any(1), pos.any(0) & neg.any(0)
        lines.append((row, rs, col, cs))
        mean = lambda v, s: v[s].sum() / s.sum() if s.any() else np.nan
        terms.append((mean(row, rs) + mean(col, cs)) / 2)
    return lines, float(np.mean(terms))


# ---- small reductions and maps --------------------------------------------------------------
def bce_mean(x, y):
    """nn.BCEWithLogitsLoss (mean): (1 - y) x - log_sigmoid(x)."""
    x, y = _f64(x), _f64(y)
    ls = np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))
    return float(((1.0 - y) * x - ls).mean())


def pose_inverse(pose):
    pose = _f64(pose)
    rt = np.swapaxes(pose[..., :3], -1, -2)
    return np.concatenate([rt, -(rt @ pose[..., 3:4])], -1)


def transform_points(xyz, seg_off, pose, inverse=False):
    """Rows of segment s -> R_s x + t_s with pose[s] (3, 4), or with its inverse."""
    xyz, pose = _f64(xyz), _f64(pose)
    if inverse:
        pose = pose_inverse(pose)
    out = np.empty_like(xyz)
    for s in range(len(seg_off) - 1):
        sl = slice(int(seg_off[s]), int(seg_off[s + 1]))
        out[sl] = xyz[sl] @ pose[s, :, :3].T + pose[s, :, 3]
    return out


def corr_loss(xyz, corr, w, seg_off, n_pairs, pose):
    """CorrCriterion('mae'), both directions: clouds c < n_pairs against pose[c], the others
    against the inverse of pose[c - n_pairs]; each direction sum(w |corr - T(xyz)|_1) /
    max(sum w, 1e-6) over all of its rows; the two added."""
    xyz, corr, w, pose = _f64(xyz), _f64(corr), _f64(w), _f64(pose)
    tgt = transform_points(xyz, seg_off, np.concatenate([pose, pose_inverse(pose)]))
    err = np.abs(corr - tgt).sum(1)
    n_src = int(seg_off[n_pairs])
    tot = 0.0
    for sl in (slice(0, n_src), slice(n_src, None)):
        tot += (w[sl] * err[sl]).sum() / max(w[sl].sum(), 1e-6)
    return float(tot)


def overlap_pool(prev, idx):
    """out[q] = clamp(mean of prev over the entries with -n_prev <= idx < n_prev, 0, 1), a
    negative index counting from the end (torch indexing); NaN for a row without one."""
    prev, idx = _f64(prev), np.asarray(idx, np.int64)
    n = len(prev)
    valid = (idx < n) & (idx >= -n)
    vals = np.where(valid, prev[np.where(valid, idx, 0) % max(n, 1)], 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.clip(vals.sum(1) / valid.sum(1), 0.0, 1.0)


def se3_compare(pred, gt):
    """pred (L, B, 3, 4), gt (B, 3, 4) -> (cosine, angle in degrees, translation error), each
    (L, B), of pred . inv(gt)."""
    pred, gt = _f64(pred), _f64(gt)
    ig = pose_inverse(gt)
    R = pred[..., :3] @ ig[None, :, :, :3]
    t = (pred[..., :3] @ ig[None, :, :, 3:4])[..., 0] + pred[..., 3]
    c = np.clip(0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0), -1.0, 1.0)
    return c, np.degrees(np.arccos(c)), np.linalg.norm(t, axis=-1)


# ---- pose -----------------------------------------------------------------------------------
def kabsch(a, b, w, threshold=0.85):
    """Weighted Procrustes of one problem, a, b (n, 3), w (n,) -> (3, 4): w <- w if w >
    threshold else 0 (threshold < 0: untouched), wn = w / max(sum w, 1e-6), centroids, H =
    (a - ca)^T ((b - cb) wn), U S V^T = svd(H), R = V U^T or V diag(1, 1, -1) U^T when
    det(V U^T) <= 0, t = cb - R ca."""
    a, b, w = _f64(a).reshape(-1, 3), _f64(b).reshape(-1, 3), _f64(w).reshape(-1).copy()
    if threshold >= 0:                                  # the ABI's threshold is a float32
        w[~(w > float(np.float32(threshold)))] = 0.0
    wn = w / max(w.sum(), 1e-6)
    ca, cb = (a * wn[:, None]).sum(0), (b * wn[:, None]).sum(0)
    H = (a - ca).T @ ((b - cb) * wn[:, None])
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    R = V @ U.T
    if np.linalg.det(R) <= 0:
        V = V.copy()
        V[:, 2] = -V[:, 2]
        R = V @ U.T
    return np.concatenate([R, (cb - R @ ca)[:, None]], 1)


def sigmoid_f32(x):
    """sigmoid in float64, rounded to float32 (the weight the threshold test sees)."""
    return (1.0 / (1.0 + np.exp(-_f64(x)))).astype(np.float32)


def pair_pose(xyz, corr, logits, seg_off, n_pairs, threshold=0.85):
    """xyz (n_tot, 3), corr (L, n_tot, 3), logits (L, n_tot), seg_off (2 n_pairs + 1) ->
    (L, n_pairs, 3, 4): kabsch of a = [src_kp ; tgt_corr_l], b = [src_corr_l ; tgt_kp],
    w = sigmoid([src_logit_l ; tgt_logit_l])."""
    xyz, corr = _f64(xyz), _f64(corr)
    L = corr.shape[0]
    out = np.empty((L, n_pairs, 3, 4))
    for l in range(L):
        w = sigmoid_f32(logits[l])
        for p in range(n_pairs):
            s = slice(int(seg_off[p]), int(seg_off[p + 1]))
            t = slice(int(seg_off[n_pairs + p]), int(seg_off[n_pairs + p + 1]))
            a = np.concatenate([xyz[s], corr[l][t]])
            b = np.concatenate([corr[l][s], xyz[t]])
            out[l, p] = kabsch(a, b, np.concatenate([w[s], w[t]]), threshold)
    return out


def weighted_residual(pose, a, b, w):
    """sum_i w_i |R a_i + t - b_i|^2."""
    pose, a, b, w = _f64(pose), _f64(a), _f64(b), _f64(w)
    r = a @ pose[:, :3].T + pose[:, 3] - b
    return float((w * (r * r).sum(1)).sum())


# ---- input generators (fixed seeds) ----------------------------------------------------------
# offsets with |o|^2 <= 3 lattice steps: the neighbours closer than r_p = 0.12 on the 1/16 lattice
_NEAR = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], np.int64)


def lattice_clouds(seed, a_lens, p_lens, modes=None):
    """Packed anchor and positive clouds (float32) with coordinates k / 16, k an integer in
    [0, 16]. On these the five-term float32 distance of the kernels is exact, every squared
    distance is a multiple of 1/256 (3/256 and 4/256 sit either side of r_p^2, 14/256 and
    16/256 either side of r_n^2 -- 15 is no sum of three squares), and exact ties are common.
    Per pair mode: 'near' (default) about 80 % of the anchors within r_p of a positive, three
    in ten of them placed midway between two positives of adjacent indices (a tie), and for
    more than 64 positives some that repeat the one 64 places earlier (a tie across the two
    passes of a wave); 'far' no anchor within r_n of any positive (no kept row); 'inside' every
    point of the pair within r_n of every other (only the positive survives the ignore mask)."""
    rng = np.random.default_rng(seed)
    modes = modes or ['near'] * len(a_lens)
    A, P = [], []
    for na, npos, mode in zip(a_lens, p_lens, modes):
        if mode == 'inside':
            p = rng.integers(0, 3, (npos, 3))
            a = rng.integers(0, 3, (na, 3))
        elif mode == 'far':
            p = rng.integers(0, 17, (npos, 3))
            a = rng.integers(0, 17, (na, 3))
            p[:, 0] = rng.integers(0, 7, npos)
            a[:, 0] = rng.integers(11, 17, na)
        else:
            p = rng.integers(0, 17, (npos, 3))
            for j in range(1, npos, 2):                 # odd index: two steps along x from its
                if rng.random() < 0.5:                  # even neighbour, a midpoint between them
                    p[j - 1, 0] = min(p[j - 1, 0], 14)
                    p[j] = p[j - 1] + (2, 0, 0)
            for j in range(64, npos):
                if rng.random() < 0.3:
                    p[j] = p[j - 64]
            a = rng.integers(0, 17, (na, 3))
            for i in range(na):
                u = rng.random()
                if npos == 0 or u >= 0.8:
                    continue
                j = int(rng.integers(0, npos))
                if u < 0.3 and npos >= 2:
                    j -= j % 2
                    if j + 1 < npos and np.array_equal(p[j + 1], p[j] + (2, 0, 0)):
                        a[i] = p[j] + (1, 0, 0)
                        continue
                a[i] = np.clip(p[j] + _NEAR[rng.integers(0, len(_NEAR))], 0, 16)
        A.append(a)
        P.append(p)
    cat = lambda L: (np.concatenate(L).astype(np.float64) / 16.0).astype(np.float32).reshape(-1, 3)
    return cat(A), cat(P)


def continuous_clouds(seed, a_lens, p_lens):
    """Packed clouds uniform in the unit cube (float32), about 80 % of the anchors moved to
    within 0.1 of a positive. Conditions of the input, asserted here in float64: no anchor-
    positive distance within 1e-4 of r_p or r_n, and each row's nearest and second nearest
    positives differ by more than 1e-5 -- so float32 and float64 agree on every discrete
    decision. A seed that misses them is a wrong seed, not a skip."""
    rng = np.random.default_rng(seed)
    A, P = [], []
    for na, npos in zip(a_lens, p_lens):
        p = rng.random((npos, 3))
        a = rng.random((na, 3))
        for i in range(na):
            if npos and rng.random() < 0.8:
                v = rng.normal(size=3)
                a[i] = p[rng.integers(0, npos)] + v / np.linalg.norm(v) * rng.uniform(0.01, 0.1)
        A.append(a.astype(np.float32))
        P.append(p.astype(np.float32))
        if na and npos:
            d = point_dist(A[-1], P[-1])
            assert np.abs(d - R_P).min() > 1e-4 and np.abs(d - R_N).min() > 1e-4, \
                f'seed {seed}: a distance within 1e-4 of r_p / r_n'
            if npos > 1:
                s = np.sort(d, 1)
                assert (s[:, 1] - s[:, 0]).min() > 1e-5, f'seed {seed}: near-tied nearest positive'
    return np.concatenate(A).reshape(-1, 3), np.concatenate(P).reshape(-1, 3)


def rotation(axis, deg):
    """Rodrigues rotation matrix (float64)."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    th = math.radians(deg)
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def random_pose(rng, max_deg=180.0, max_t=1.0):
    """(3, 4) float64: a rotation by up to max_deg about a random axis and a translation."""
    R = rotation(rng.normal(size=3), rng.uniform(-max_deg, max_deg))
    return np.concatenate([R, rng.uniform(-max_t, max_t, (3, 1))], 1)


def weights_away_from(rng, n, threshold=0.85, margin=1e-3):
    """Uniform [0, 1] weights (float32), none within `margin` of the threshold."""
    w = rng.random(n).astype(np.float32)
    near = np.abs(w.astype(np.float64) - threshold) < margin
    w[near] = np.float32(threshold + 2 * margin)
    return w


def logits_away_from(rng, n, threshold=0.85, margin=1e-3, scale=3.0):
    """Logits (float32) whose sigmoid is at least `margin` away from the threshold."""
    x = (rng.normal(size=n) * scale + math.log(threshold / (1 - threshold))).astype(np.float32)
    near = np.abs(sigmoid_f32(x).astype(np.float64) - threshold) < margin
    x[near] += np.float32(0.1)
    assert (np.abs(sigmoid_f32(x).astype(np.float64) - threshold) >= margin).all()
    return x


# ---- the parametrised cases of tests/test_gpu_tail_kernels.py -------------------------------
# Built here so that tests/test_tail_ref.py checks every case's input conditions on the CPU.
P_LAYOUTS = ([1, 63, 64], [65, 130, 7], [64, 0, 5])      # positives per pair (0: empty cloud)
A_LAYOUTS = ([3, 5, 1], [4, 0, 9])                       # anchors per pair (0: empty segment)
INFONCE_G = 0.37                                         # upstream gradient of the backward


def _infonce_cases():
    cases = {}
    for kind in ('lattice', 'continuous'):
        for pi, pl in enumerate(P_LAYOUTS):
            for ai, al in enumerate(A_LAYOUTS):
                cases[f'{kind}-p{pi}-a{ai}'] = dict(kind=kind, p_lens=pl, a_lens=al)
    cases['pm80'] = dict(kind='lattice', p_lens=P_LAYOUTS[1], a_lens=A_LAYOUTS[0], peak=80.0)
    cases['only-positive'] = dict(kind='lattice', p_lens=[5, 27, 70], a_lens=A_LAYOUTS[0],
                                  modes=['inside'] * 3)
    cases['no-kept-row'] = dict(kind='lattice', p_lens=P_LAYOUTS[1], a_lens=A_LAYOUTS[0],
                                modes=['near', 'far', 'near'])
    return cases


INFONCE_CASES = _infonce_cases()
# seeds for which every case's conditions hold (tests/test_tail_ref.py asserts them)
INFONCE_SEEDS = {'lattice-p0-a0': 1, 'lattice-p0-a1': 1, 'lattice-p1-a0': 2, 'lattice-p1-a1': 1,
                 'lattice-p2-a0': 2, 'lattice-p2-a1': 1, 'continuous-p0-a0': 1,
                 'continuous-p0-a1': 1, 'continuous-p1-a0': 2, 'continuous-p1-a1': 1,
                 'continuous-p2-a0': 1, 'continuous-p2-a1': 1, 'pm80': 2, 'only-positive': 1,
                 'no-kept-row': 1}


def infonce_inputs(name):
    """-> dict: axyz, pxyz (float32), a_off, p_off, n_cols (positives padded to a multiple of 8,
    as compute_loss_train pads them) and logits (n_anchor, n_cols) float32 ~ N(0, sigma = 2),
    NaN in the padding columns that belong to no pair; 'finite': the pairs meant to give a
    finite loss (anchors, positives, not 'far')."""
    c = INFONCE_CASES[name]
    seed = INFONCE_SEEDS[name]
    modes = c.get('modes') or ['near'] * len(c['a_lens'])
    if c['kind'] == 'lattice':
        axyz, pxyz = lattice_clouds(seed, c['a_lens'], c['p_lens'], modes)
    else:
        axyz, pxyz = continuous_clouds(seed, c['a_lens'], c['p_lens'])
    a_off, p_off = offsets(c['a_lens']), offsets(c['p_lens'])
    n_a, n_p = int(a_off[-1]), int(p_off[-1])
    n_cols = (n_p + 7) // 8 * 8
    rng = np.random.default_rng(seed + 1000)
    logits = np.full((n_a, n_cols), np.nan, np.float32)
    logits[:, :n_p] = (2.0 * rng.normal(size=(n_a, n_p))).astype(np.float32)
    if 'peak' in c:
        logits[:, :n_p] *= np.float32(c['peak'] / np.abs(logits[:, :n_p]).max())
    finite = [b for b in range(len(modes))
              if c['a_lens'][b] > 0 and c['p_lens'][b] > 0 and modes[b] != 'far']
    return dict(axyz=axyz, pxyz=pxyz, a_off=a_off, p_off=p_off, n_cols=n_cols, logits=logits,
                finite=finite, modes=modes, kind=c['kind'])


MIX_PAIRS = [(1, 1), (15, 17), (16, 16), (17, 33), (33, 2)]      # packed together in one call
CDIST_DIMS = [1, 32, 63, 64, 65, 130, 256]
CIRCLE_CASES = {
    # name: (pairs (n_a, n_p), d, modes, finite scalar expected)
    'small': ([(3, 2), (5, 70), (70, 5)], 20, None, True),
    'mix4': (MIX_PAIRS[1:], 32, None, True),
    'long': ([(1030, 2), (3, 1100)], 20, None, True),  # lines past the reduction's 1024 threads
    'mix': (MIX_PAIRS, 32, None, False),               # the (1, 1) pair cannot hold both kinds
    'no-negative': ([(3, 2), (5, 7)], 20, ['near', 'inside'], False),
    'empty-side': ([(3, 2), (0, 5), (4, 0)], 20, None, False),
}
CIRCLE_SEEDS = {'small': 1, 'mix4': 1, 'long': 1, 'mix': 3, 'no-negative': 1, 'empty-side': 1}


def feature_rows(rng, n, d, lo=0.005, hi=0.3):
    """(n, d) float32 rows of log-uniform scale: between two rows the Euclidean distance runs
    from well under the circle loss's 0.1 margin to well over its 1.4."""
    s = np.exp(rng.uniform(math.log(lo), math.log(hi), (n, 1))) * math.sqrt(32.0 / d)
    return (rng.normal(size=(n, d)) * s).astype(np.float32)


def circle_inputs(name):
    pairs, d, modes, finite = CIRCLE_CASES[name]
    seed = CIRCLE_SEEDS[name]
    a_lens, p_lens = [p[0] for p in pairs], [p[1] for p in pairs]
    axyz, pxyz = lattice_clouds(seed, a_lens, p_lens, modes)
    rng = np.random.default_rng(seed + 2000)
    af, pf = feature_rows(rng, sum(a_lens), d), feature_rows(rng, sum(p_lens), d)
    return dict(af=af, pf=pf, d=d, axyz=axyz, pxyz=pxyz, a_off=offsets(a_lens),
                p_off=offsets(p_lens), a_lens=a_lens, p_lens=p_lens, finite=finite,
                fd_off=offsets([a * p for a, p in pairs]))


def cdist_inputs(d):
    """The packed mix with random features of width d; anchor row 0 of the (15, 17) pair equals
    its positive row 3 (fd = sqrt(1e-12))."""
    a_lens, p_lens = [p[0] for p in MIX_PAIRS], [p[1] for p in MIX_PAIRS]
    rng = np.random.default_rng(100 + d)
    af = rng.normal(size=(sum(a_lens), d)).astype(np.float32)
    pf = rng.normal(size=(sum(p_lens), d)).astype(np.float32)
    af[1] = pf[1 + 3]
    return dict(af=af, pf=pf, d=d, a_off=offsets(a_lens), p_off=offsets(p_lens), a_lens=a_lens,
                p_lens=p_lens, fd_off=offsets([a * p for a, p in MIX_PAIRS]))
