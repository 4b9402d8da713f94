"""Timing of fgreg.compat (csrc/compat.hip) at the correspondence counts the forward produces and
at the inlier ratios where it matters: HIP events around the call, medians over `reps` calls
after 3 warm-ups, one JSON line per workload and planted ratio.

  modelnet      8 pairs of about 1200 rows, r = 0.05
  3dmatch-2120  one pair of 2120 rows, r = 0.1
  3dmatch-3991  one pair of 3991 rows, r = 0.1

The rows are tools/ransac_bench.py's planted ones at 30 %, 5 % and 3 % inliers; compat_dist =
inlier_dist = r, 64 seeds, k = 16, 4 refits, every row eligible.

  compat_us     fgreg.compat: the six launches
  torch_us      the same rules in batched torch on the same GPU (torch.cdist lengths, the
                second order as a float m x m x m matmul, topk seeds and neighbours,
                torch.linalg.svd Kabsch fits in fp64, 4 masked refits), pairs one after the
                other: the baseline, context only (topk breaks ties its own way)
  ratio         torch_us / compat_us
  ransac_n_hyp  the smallest of 4096, 16384, .. 2^20 hypotheses at which fgreg.ransac reaches
                compat's inlier count on every pair (null: none does), ransac_us its time there
  n_inliers, n_planted, n_updates of the fgreg.compat call

  python tools/compat_bench.py [--reps 30] [--workloads modelnet,3dmatch-2120,3dmatch-3991]
                              [--ratios 0.3,0.05,0.03] [--no-torch] [--once]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ransac_bench import N_REFITS, _d2, _kabsch, median_us, planted  # noqa: E402
import fgreg  # noqa: E402  (ransac_bench put the package on the path)

N_SEEDS, K_SET = 64, 16
WORKLOADS = {'modelnet': ([1187, 1203, 1216, 1194, 1209, 1178, 1221, 1192], 0.05),
             '3dmatch-2120': ([2120], 0.1), '3dmatch-3991': ([3991], 0.1)}


def torch_compat(a, b, cdist, r, n_seeds=N_SEEDS, k=K_SET, n_refits=N_REFITS):
    """One pair, a, b (m, 3) fp32 GPU tensors -> (R, t, inlier count); no host decision."""
    m = a.shape[0]
    S = (torch.cdist(a, a) - torch.cdist(b, b)).abs() < cdist
    S.fill_diagonal_(False)
    Sf = S.float()
    C = Sf @ Sf                                             # exact: counts below 2^24
    seeds = torch.topk((Sf * C).sum(1), min(n_seeds, m)).indices
    cs = torch.where(S[seeds], C[seeds], -1.0)
    val, nb = torch.topk(cs, min(k - 1, m), dim=1)
    w = torch.cat([torch.ones(len(seeds), 1, device=a.device), (val >= 0).float()], 1).double()
    mem = torch.cat([seeds[:, None], nb], 1)
    R, t = _kabsch(a[mem].double(), b[mem].double(), w)
    r2 = r * r
    cnt = (_d2(R, t, a, b) < r2).sum(1)
    best = torch.argmax(torch.where(w.sum(1) >= 3, cnt, -1))
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
    ap.add_argument('--workloads', default='modelnet,3dmatch-2120,3dmatch-3991')
    ap.add_argument('--ratios', default='0.3,0.05,0.03')
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--no-ransac', action='store_true')
    ap.add_argument('--once', action='store_true', help='one fgreg.compat call per case (for a kernel trace)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('compat_bench needs a GPU')
    for name in args.workloads.split(','):
        counts, r = WORKLOADS[name]
        for frac in (float(v) for v in args.ratios.split(',')):
            rows = [planted(100 + p, m, r, frac) for p, m in enumerate(counts)]
            A = [torch.from_numpy(x[0]).cuda() for x in rows]
            Bt = [torch.from_numpy(x[1]).cuda() for x in rows]
            call = lambda: fgreg.compat(A, Bt, compat_dist=r, inlier_dist=r, n_seeds=N_SEEDS, k=K_SET,
                                        n_refits=N_REFITS)
            if args.once:
                call()
                torch.cuda.synchronize()
                continue
            res = {'workload': name, 'pairs': len(counts), 'rows': counts, 'r': r, 'planted': frac,
                   'n_planted': [int(frac * m) for m in counts], 'n_seeds': N_SEEDS, 'k': K_SET,
                   'reps': args.reps}
            res['compat_us'] = median_us(call, args.reps)
            out = call()
            res['n_inliers'] = out['n_inliers'].cpu().tolist()
            res['n_updates'] = out['n_updates'].cpu().tolist()
            if not args.no_torch:
                base = lambda: [torch_compat(a, b, r, r) for a, b in zip(A, Bt)]
                res['torch_us'] = median_us(base, max(args.reps // 3, 5), warmup=2)
                res['ratio'] = res['torch_us'] / res['compat_us']
                res['torch_n_inliers'] = [int(x[2]) for x in base()]
            if not args.no_ransac:
                res['ransac_n_hyp'] = res['ransac_us'] = None
                for n_hyp in (4096, 16384, 65536, 262144, 1048576):
                    rs = lambda: fgreg.ransac(A, Bt, inlier_dist=r, n_hyp=n_hyp, seed=1, n_refits=N_REFITS)
                    got = rs()['n_inliers'].cpu().tolist()
                    if all(g >= c for g, c in zip(got, res['n_inliers'])):
                        res['ransac_n_hyp'], res['ransac_us'] = n_hyp, median_us(rs, args.reps)
                        break
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
