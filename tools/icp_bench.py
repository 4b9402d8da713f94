"""Timing of fgreg.refine (csrc/icp.hip, csrc/normals.hip) at the sizes a consumer refines: HIP
events around the entry points, medians over `reps` calls after a warm-up, one JSON line per
workload and method.

  modelnet  8 pairs of 717 + 717 points (fgreg.synthetic.make_batch('modelnet', 8)), r = 0.05,
            normals from a 0.1 radius
  3dmatch   one indoor_like_pair of 20k + 20k points, r = 0.05, normals from a 0.1 radius
  lidar     one lidar_like_pair of 60k + 60k points over 60 m, r = 0.5, normals from a 1.0 radius

Per workload, from the ground-truth pose perturbed by 2 degrees and 0.4 r:
  score_us      fgr_registration_score: the grid build, one association pass, the finish
  icp0_us       fgr_icp with max_iters = 0: the grid build and one pass
  icp30_us      fgr_icp with max_iters = 30 and both tolerances 0, so that no pair stops early:
                31 association passes and 30 solves
  pass_us       (icp30_us - icp0_us) / 30: one association pass plus one solve
  icp30_default_us  max_iters = 30 with the default tolerances (pairs freeze when they converge)
  n_iters, fitness, inlier_rmse of that call (n_iters: the updates to convergence)
With --method point_to_plane the same figures for fgr_icp_plane, given the target normals
(estimated once, outside the timed calls), and
  normals_us    fgr_estimate_normals on the target clouds: the grid build, the cell sort, the
                eigen-solves
  n_valid       the targets' valid normals; status of the default call
score_us, forward_us and host_ms belong to the point_to_point line.
  forward_us    that workload's RegTR forward (random weights, eval), where a config exists
  host_ms       the same loop on the host in fp64 with scipy's cKDTree (workers = 16), the
                clouds already on the host: context only
Kernel-level times (association against solve) come from a kernel trace of `--once`.

  python tools/icp_bench.py [--reps 50] [--workloads modelnet,3dmatch,lidar] [--no-forward]
                            [--no-host] [--once] [--method both|point_to_point|point_to_plane]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'boosting-fine-grained-feature-fusion-in-3d-point-cloud-registration_amd'))
import fgreg  # noqa: E402
from fgreg import _lib  # noqa: E402
from fgreg.synthetic import indoor_like_pair, lidar_like_pair, make_batch  # noqa: E402


def rotation(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def perturbed(gt, r, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for T in np.asarray(gt, np.float64):
        dR = rotation(rng.normal(size=3), 2.0)
        out.append(np.concatenate([dR @ T[:, :3], (dR @ T[:, 3] + rng.uniform(-0.4 * r, 0.4 * r, 3))[:, None]], 1))
    return np.stack(out).astype(np.float32)


def workload(name):
    if name == 'modelnet':
        src, tgt, gt = make_batch('modelnet', 8)
        return src, tgt, gt, 0.05, 'modelnet', 0.1
    if name == '3dmatch':
        s, t, p = indoor_like_pair(0, n_points=20000)
        return [s], [t], p[None], 0.05, '3dmatch', 0.1
    s, t, p = lidar_like_pair(0, n_points=60000)
    return [s], [t], p[None], 0.5, None, 1.0


def median_us(fn, reps, warmup=5):
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


def host_icp(src, tgt, pose, r, max_iters=30, rel=1e-6):
    """Point-to-point ICP on the host: fp64, cKDTree with 16 workers -> (pose, n_iters)."""
    from scipy.spatial import cKDTree
    tree = cKDTree(tgt.astype(np.float64))
    p = src.astype(np.float64)
    T = pose.astype(np.float64)
    f_prev = e_prev = 0.0
    for k in range(max_iters + 1):
        d, j = tree.query(p @ T[:, :3].T + T[:, 3], distance_upper_bound=r, workers=16)
        inl = np.isfinite(d)
        n = int(inl.sum())
        f, e = n / len(p), (float(np.sqrt((d[inl] ** 2).mean())) if n else 0.0)
        if (k >= 1 and abs(f - f_prev) < rel and abs(e - e_prev) < rel) or n < 3 or k == max_iters:
            return T, k
        f_prev, e_prev = f, e
        a, b = p[inl], tgt[j[inl]].astype(np.float64)
        ca, cb = a.mean(0), b.mean(0)
        U, _, Vt = np.linalg.svd((a - ca).T @ (b - cb))
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
        R = Vt.T @ D @ U.T
        T = np.concatenate([R, (cb - R @ ca)[:, None]], 1)
    return T, max_iters


def forward_us(cfg_name, src, tgt, reps):
    cfg = fgreg.config.get(cfg_name)
    torch.manual_seed(0)
    model = fgreg.RegTR(cfg).eval().cuda()
    batch = lambda: {'src_xyz': [torch.from_numpy(s).cuda() for s in src],
                     'tgt_xyz': [torch.from_numpy(t).cuda() for t in tgt]}
    b = batch()
    with torch.no_grad():
        return median_us(lambda: model(dict(b)), reps, warmup=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--workloads', default='modelnet,3dmatch,lidar')
    ap.add_argument('--no-forward', action='store_true')
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--once', action='store_true', help='one ICP call per workload and method (for a kernel trace)')
    ap.add_argument('--method', default='both', choices=['both', 'point_to_point', 'point_to_plane'])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('icp_bench needs a GPU')
    methods = ['point_to_point', 'point_to_plane'] if args.method == 'both' else [args.method]
    for name in args.workloads.split(','):
        src, tgt, gt, r, cfg_name, normal_radius = workload(name)
        start = perturbed(gt, r)
        S, Tg = [torch.from_numpy(s).cuda() for s in src], [torch.from_numpy(t).cuda() for t in tgt]
        P = torch.from_numpy(start).cuda()
        for method in methods:
            plane = method == 'point_to_plane'
            kw = {}
            if plane:
                est = fgreg.estimate_normals(Tg, normal_radius)
                kw = {'method': method, 'tgt_normals': est['normals']}
            icp = lambda **k: fgreg.icp(S, Tg, P, r, **kw, **k)
            if args.once:
                icp(rel_fitness=0.0, rel_rmse=0.0)
                torch.cuda.synchronize()
                continue
            res = {'workload': name, 'method': method, 'lib': os.path.basename(_lib.LIB_PATH),
                   'pairs': len(src), 'n_src': int(src[0].shape[0]), 'n_tgt': int(tgt[0].shape[0]),
                   'r': r, 'reps': args.reps}
            if plane:
                res['normal_radius'] = normal_radius
                res['normals_us'] = median_us(lambda: fgreg.estimate_normals(Tg, normal_radius), args.reps)
                res['n_valid'] = est['n_valid'].cpu().tolist()
            else:
                res['score_us'] = median_us(lambda: fgreg.score(S, Tg, P, r), args.reps)
            res['icp0_us'] = median_us(lambda: icp(max_iters=0), args.reps)
            res['icp30_us'] = median_us(lambda: icp(rel_fitness=0.0, rel_rmse=0.0), args.reps)
            res['pass_us'] = (res['icp30_us'] - res['icp0_us']) / 30
            res['icp30_default_us'] = median_us(lambda: icp(), args.reps)
            out = icp()
            res['n_iters'] = out['n_iters'].cpu().tolist()
            res['fitness'] = [round(v, 4) for v in out['fitness'].cpu().tolist()]
            res['inlier_rmse'] = [round(v, 5) for v in out['inlier_rmse'].cpu().tolist()]
            if plane:
                res['status'] = out['status'].cpu().tolist()
            if cfg_name and not args.no_forward and not plane:
                res['forward_us'] = forward_us(cfg_name, src, tgt, max(args.reps // 5, 5))
            if not args.no_host and not plane:
                t0 = time.perf_counter()
                iters = [host_icp(s, t, p, r)[1] for s, t, p in zip(src, tgt, start)]
                res['host_ms'] = (time.perf_counter() - t0) * 1e3
                res['host_n_iters'] = iters
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
