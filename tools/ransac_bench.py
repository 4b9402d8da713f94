"""Timing of fgreg.ransac (csrc/ransac.hip) at the correspondence counts the forward produces:
HIP events around the call, medians over `reps` calls after a warm-up, one JSON line per
workload and hypothesis count.

  modelnet  8 pairs (fgreg.synthetic.make_batch('modelnet', 8)), r = 0.05
  3dmatch   one indoor_like_pair of 20k + 20k points, r = 0.1

A pair has one correspondence per coarse-level point of either cloud: the counts are the last
pyramid level's lengths of that batch under the workload's config (the preprocessor alone is
run, not the network). The rows themselves are planted: 30 % follow one rigid pose with noise
below 0.2 r, the others point anywhere in the cloud's box.

Per workload and n_hyp in 1024, 4096, 16384 (4 refits, every row eligible):
  ransac_us     fgreg.ransac: the three launches
  torch_us      the same hypotheses in batched torch on the same GPU (the same hash and ranks,
                torch.linalg.svd Kabsch fits in fp64, one (n_hyp, m) distance matrix per pair,
                argmax, 4 masked refits), pairs one after the other: the baseline, context only
  ratio         torch_us / ransac_us
  agree         both end on the same inlier count for every pair
  n_inliers, n_updates of the fgreg call

  python tools/ransac_bench.py [--reps 30] [--workloads modelnet,3dmatch] [--no-torch] [--once]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'boosting-fine-grained-feature-fusion-in-3d-point-cloud-registration_amd'))
import fgreg  # noqa: E402
from fgreg import _lib  # noqa: E402
from fgreg.backbone import host_layout  # noqa: E402
from fgreg.synthetic import indoor_like_pair, make_batch  # noqa: E402

N_REFITS = 4


def coarse_counts(name):
    """-> ([correspondences per pair], r): source plus target points at the coarsest level."""
    if name == 'modelnet':
        src, tgt, _ = make_batch('modelnet', 8)
        cfg, r = fgreg.config.get('modelnet'), 0.05
    else:
        s, t, _ = indoor_like_pair(0, n_points=20000)
        src, tgt, cfg, r = [s], [t], fgreg.config.get('3dmatch'), 0.1
    torch.manual_seed(0)
    model = fgreg.RegTR(cfg).eval().cuda()
    clouds = [torch.from_numpy(c).cuda() for c in list(src) + list(tgt)]
    with torch.no_grad():
        meta = model.preprocessor(clouds)
    lens, _ = host_layout(meta, len(meta['points']) - 1)
    B = len(src)
    return [lens[p] + lens[B + p] for p in range(B)], r


def planted(seed, m, r, inlier_frac=0.3):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (m, 3))
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K
    b = a @ R.T + rng.uniform(-0.5, 0.5, 3) + rng.normal(0, 0.2 * r / 3, (m, 3))
    out = rng.permutation(m)[int(inlier_frac * m):]
    b[out] = rng.uniform(-1.5, 1.5, (len(out), 3))
    return a.astype(np.float32), b.astype(np.float32)


def median_us(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


# ---- the baseline: the same hypotheses in batched torch ---------------------------------------
def _hash(seed, head, q, k):
    """common.h attn_drop_hash on int64 tensors holding 32-bit values."""
    M = 0xFFFFFFFF
    x = (seed ^ ((head * 0x9E3779B9) & M)) ^ ((q * 0x85EBCA6B) & M)
    x = ((x ^ (x >> 16)) * 0x7FEB352D) & M
    x = x ^ ((k * 0xC2B2AE35) & M)
    x = ((x ^ (x >> 15)) * 0x846CA68B) & M
    return x ^ (x >> 16)


def _kabsch(a, b, w):
    """Weighted fp64 Kabsch, batched: a, b (..., n, 3), w (..., n) -> R (..., 3, 3), t (..., 3)."""
    ws = w.sum(-1, keepdim=True).clamp_min(1.0)
    am, bm = (a * w[..., None]).sum(-2) / ws, (b * w[..., None]).sum(-2) / ws
    H = ((a - am[..., None, :]) * w[..., None]).transpose(-1, -2) @ (b - bm[..., None, :])
    U, _, Vh = torch.linalg.svd(H)
    V = Vh.transpose(-1, -2)
    d = torch.linalg.det(V @ U.transpose(-1, -2))
    D = torch.ones(H.shape[:-1], dtype=H.dtype, device=H.device)
    D[..., 2] = torch.where(d < 0, -1.0, 1.0)
    R = (V * D[..., None, :]) @ U.transpose(-1, -2)
    return R, bm - (R @ am[..., None])[..., 0]


def _d2(R, t, a, b):
    q = a @ R.float().transpose(-1, -2) + t.float()[..., None, :]
    return ((q - b) ** 2).sum(-1)


def torch_ransac(a, b, pair, n_hyp, seed, r, n_refits=N_REFITS):
    """One pair, a, b (m, 3) fp32 GPU tensors -> (R, t, inlier count); no host decision."""
    m = a.shape[0]
    h = torch.arange(n_hyp, device=a.device, dtype=torch.int64)
    rk = torch.stack([(_hash(seed, k, pair, h) * m) >> 32 for k in range(3)], 1)
    ok = (rk[:, 0] != rk[:, 1]) & (rk[:, 0] != rk[:, 2]) & (rk[:, 1] != rk[:, 2])
    R, t = _kabsch(a[rk].double(), b[rk].double(), torch.ones(n_hyp, 3, dtype=torch.float64, device=a.device))
    r2 = r * r
    cnt = (_d2(R, t, a, b) < r2).sum(1)
    best = torch.argmax(torch.where(ok, cnt, -1))
    R, t, c = R[best], t[best], cnt[best]
    for _ in range(n_refits):
        K = (_d2(R, t, a, b) < r2).double()
        Rn, tn = _kabsch(a.double(), b.double(), K)
        cn = (_d2(Rn, tn, a, b) < r2).sum()
        take = cn >= c
        R, t, c = torch.where(take, Rn, R), torch.where(take, tn, t), torch.where(take, cn, c)
    return R, t, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--workloads', default='modelnet,3dmatch')
    ap.add_argument('--n-hyp', default='1024,4096,16384')
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--once', action='store_true', help='one fgreg.ransac call per case (for a kernel trace)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ransac_bench needs a GPU')
    for name in args.workloads.split(','):
        counts, r = coarse_counts(name)
        rows = [planted(100 + p, m, r) for p, m in enumerate(counts)]
        A = [torch.from_numpy(x[0]).cuda() for x in rows]
        Bt = [torch.from_numpy(x[1]).cuda() for x in rows]
        for n_hyp in (int(v) for v in args.n_hyp.split(',')):
            call = lambda: fgreg.ransac(A, Bt, inlier_dist=r, n_hyp=n_hyp, seed=1, n_refits=N_REFITS)
            if args.once:
                call()
                torch.cuda.synchronize()
                continue
            res = {'workload': name, 'lib': os.path.basename(_lib.LIB_PATH), 'pairs': len(counts),
                   'rows': counts, 'r': r, 'n_hyp': n_hyp, 'reps': args.reps}
            res['ransac_us'] = median_us(call, args.reps)
            out = call()
            res['n_inliers'] = out['n_inliers'].cpu().tolist()
            res['n_updates'] = out['n_updates'].cpu().tolist()
            if not args.no_torch:
                base = lambda: [torch_ransac(a, b, p, n_hyp, 1, r) for p, (a, b) in enumerate(zip(A, Bt))]
                res['torch_us'] = median_us(base, max(args.reps // 3, 5), warmup=2)
                res['ratio'] = res['torch_us'] / res['ransac_us']
                res['torch_n_inliers'] = [int(x[2]) for x in base()]
                res['agree'] = res['torch_n_inliers'] == res['n_inliers']
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
