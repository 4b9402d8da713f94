"""Timing of fgreg.match_features (csrc/match.hip) against a batched-torch restatement of the
same result, at the sizes the forward's descriptors have: HIP events around each call, the two
sides alternating in one loop after a warm-up, medians over `reps` rounds, one JSON line per
workload and metric.

  modelnet  8 pairs of 600 + 600 rows, d 256
  3dmatch   one pair of 2120 + 1871 rows, d 512

Descriptors are the tests' seeded recipe scaled to the post-LayerNorm norm sqrt(d); mode
'mutual'; metric 'euclidean' and 'bilinear' (W ~ N(0, 0.1), as the model initialises it).
  fgreg_us   match_features: the packing, (bilinear: X W_sym,) fgr_feature_nn, fgr_match_pairs
  nn_us      fgr_feature_nn alone on the packed rows (its outputs allocated inside the events)
  torch_us   per pair cdist (euclidean) or X W_sym Y^T (bilinear), argmin / argmax both ways, the
             mutual test, the gathered rows and weights -- the same dict entries a, b, w
  agree      the share of rows whose neighbour is the same on both sides (torch's fp32 products
             differ in the last bits, so near-ties may differ)
The kernel's own time and its share of the f16x3 pipe come from a kernel trace of `--trace`.

  python tools/match_bench.py [--reps 50] [--workloads modelnet,3dmatch] [--trace]
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
from fgreg import _lib, match  # noqa: E402
from fgreg.loss import _w_sym  # noqa: E402

WORKLOADS = {'modelnet': (8, 600, 600, 256), '3dmatch': (1, 2120, 1871, 512)}


def descriptors(seed, ns, nt, d):
    """tests/_match_ref.py's recipe: unit Gaussian source rows, targets noisy copies."""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((ns, d))
    src /= np.linalg.norm(src, axis=1, keepdims=True)
    tgt = src[rng.integers(0, ns, nt)] + rng.standard_normal((nt, d)) * (0.5 / np.sqrt(d))
    tgt /= np.linalg.norm(tgt, axis=1, keepdims=True)
    return (src * np.sqrt(d)).astype(np.float32), (tgt * np.sqrt(d)).astype(np.float32)


def torch_match(fs, ft, xs, xt, metric, Wsym):
    """The same result in batched torch: an n x m matrix per pair, argmin / argmax both ways."""
    a, b, w, nn_s, nn_t = [], [], [], [], []
    for f, g, x, y in zip(fs, ft, xs, xt):
        if metric == 'euclidean':
            m = torch.cdist(f, g)
            js, it = m.argmin(1), m.argmin(0)
        else:
            m = (f @ Wsym) @ g.t()
            js, it = m.argmax(1), m.argmax(0)
        mutual = it[js] == torch.arange(len(f), device=f.device)
        a.append(torch.cat([x, x[it]], 0))
        b.append(torch.cat([y[js], y], 0))
        w.append(torch.cat([mutual.float(), torch.zeros(len(g), device=f.device)], 0))
        nn_s.append(js)
        nn_t.append(it)
    return {'a': a, 'b': b, 'w': w, 'nn_src': nn_s, 'nn_tgt': nn_t}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--workloads', default='modelnet,3dmatch')
    ap.add_argument('--trace', action='store_true',
                    help='ten match_features calls per workload and metric and nothing else (for a kernel trace)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('match_bench needs a GPU')
    dev = torch.device('cuda:0')
    for name in args.workloads.split(','):
        B, ns, nt, d = WORKLOADS[name]
        pairs = [descriptors(100 + p, ns, nt, d) for p in range(B)]
        fs = [torch.from_numpy(s).to(dev) for s, _ in pairs]
        ft = [torch.from_numpy(t).to(dev) for _, t in pairs]
        g = torch.Generator().manual_seed(0)
        xs = [torch.rand(ns, 3, generator=g).to(dev) for _ in range(B)]
        xt = [torch.rand(nt, 3, generator=g).to(dev) for _ in range(B)]
        W = (0.1 * torch.randn(d, d, generator=g)).to(dev)
        for metric in ('euclidean', 'bilinear'):
            kw = {'metric': metric, 'mode': 'mutual'}
            if metric == 'bilinear':
                kw['W'] = W
            ours = lambda: fgreg.match_features(fs, ft, xs, xt, **kw)
            theirs = lambda: torch_match(fs, ft, xs, xt, metric, _w_sym(W))
            if args.trace:
                for _ in range(10):
                    ours()
                torch.cuda.synchronize()
                continue
            keys = torch.cat(fs + ft, 0).contiguous()
            off, kv_seg, _ = match._tables([ns] * B, [nt] * B, dev)
            nn_only = lambda: match.feature_nn(keys, keys, off, off, kv_seg, max(ns, nt), match.METRICS[metric])
            for _ in range(5):
                ours(), theirs(), nn_only()
            torch.cuda.synchronize()
            t_ours, t_theirs, t_nn = [], [], []
            for _ in range(args.reps):
                t, o = timed(ours)
                t_ours.append(t)
                t, r = timed(theirs)
                t_theirs.append(t)
                t_nn.append(timed(nn_only)[0])
            same = torch.cat([torch.cat(o['nn_src']).long() == torch.cat(r['nn_src']),
                              torch.cat(o['nn_tgt']).long() == torch.cat(r['nn_tgt'])])
            flop = 2.0 * 2 * B * ns * nt * d
            res = {'workload': name, 'metric': metric, 'lib': os.path.basename(_lib.LIB_PATH), 'pairs': B,
                   'n_src': ns, 'n_tgt': nt, 'd': d, 'reps': args.reps,
                   'fgreg_us': float(np.median(t_ours)), 'nn_us': float(np.median(t_nn)),
                   'torch_us': float(np.median(t_theirs)), 'agree': float(same.float().mean()),
                   'n_matches': o['n_matches'].cpu().tolist(),
                   'torch_n_matches': [int(x.sum()) for x in r['w']],
                   'nn_gflop': flop * 1e-9, 'nn_tflops_fp32_equiv': flop / (float(np.median(t_nn)) * 1e-6) * 1e-12}
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
