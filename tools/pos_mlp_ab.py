"""A/B of the learned positional embedding's MLP: the fused launch (ops.pos_mlp,
csrc/posmlp.hip) against the chain of five linear() launches it replaces
(PositionEmbeddingLearned.forward_chain: the kernels that existed before the fused one, so the
baseline), at the two workload shapes -- (n = 9544, d = 256), the coarse points of a ModelNet
B = 8 batch, and (n = 2120, d = 512), a 3DMatch pair -- and the whole forward's ms/step with
``pos_emb_type`` learned vs sine on ModelNet B = 8.

Event timing in windows of ``iters`` calls; the two sides alternate over ``rounds`` windows
each, and the spread reported is (max - min) of a side's windows, so a difference is to be read
against it. Two figures per side: ``eager`` = back-to-back launches from Python (what an eager
forward pays, host launch path included) and ``graph`` = the same calls captured ``GRAPH_REPS``
at a time into a HIP graph and replayed (device time: what the captured core of the forward
pays). Outputs of the two sides are compared first (same f16x3
products: rel_err of a few 1e-7). Writes one JSON object (--out, default stdout).
    python tools/pos_mlp_ab.py [--iters 200] [--rounds 7] [--steps 20] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE),
                                'boosting-fine-grained-feature-fusion-in-3d-point-cloud-registration_amd'))
import fgreg  # noqa: E402
from fgreg.transformer import PositionEmbeddingLearned  # noqa: E402

SHAPES = [(9544, 256), (2120, 512)]


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def ab(fa, fb, iters, rounds):
    for _ in range(10):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(fa, iters))
        tb.append(window(fb, iters))
    stat = lambda t: {'median_us': float(np.median(t)), 'min_us': float(min(t)),      # noqa: E731
                      'max_us': float(max(t)), 'spread_us': float(max(t) - min(t))}
    return stat(ta), stat(tb)


GRAPH_REPS = 20


def captured(fn):
    """fn() GRAPH_REPS times as one HIP graph -> a callable that replays it."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_REPS):
            fn()
    return g.replay


def mlp_case(n, d, iters, rounds, dev):
    torch.manual_seed(n + d)
    m = PositionEmbeddingLearned(3, d).to(dev).eval()
    xyz = (2 * torch.rand(n, 3, device=dev) - 1) * (1.0 if d == 256 else 3.0)
    with torch.no_grad():
        fused, chain = m(xyz), m.forward_chain(xyz)
        err = float((fused - chain).abs().max() / chain.abs().max())
        sf, sc = ab(lambda: m(xyz), lambda: m.forward_chain(xyz), iters, rounds)
        gf, gc = ab(captured(lambda: m(xyz)), captured(lambda: m.forward_chain(xyz)),
                    max(iters // GRAPH_REPS, 1), rounds)
    for st in (gf, gc):                              # per call, not per replay
        for k in st:
            st[k] /= GRAPH_REPS
    return {'n': n, 'd_model': d, 'rel_err_fused_vs_chain': err,
            'eager': {'fused': sf, 'chain_of_5': sc,
                      'speedup_median': sc['median_us'] / sf['median_us']},
            'graph': {'fused': gf, 'chain_of_5': gc,
                      'speedup_median': gc['median_us'] / gf['median_us']}}


def forward_case(steps, rounds, dev):
    from fgreg.synthetic import make_batch
    src, tgt, _ = make_batch('modelnet', 8)
    batch = lambda: {'src_xyz': [torch.from_numpy(s).to(dev) for s in src],           # noqa: E731
                     'tgt_xyz': [torch.from_numpy(t).to(dev) for t in tgt]}
    models = {}
    for kind in ('sine', 'learned'):
        torch.manual_seed(0)
        np.random.seed(0)
        models[kind] = fgreg.RegTR(fgreg.config.get('modelnet', pos_emb_type=kind)).to(dev).eval()
    b = batch()

    def step(kind):
        return lambda: models[kind](dict(b))
    ss, sl = ab(step('sine'), step('learned'), steps, rounds)
    return {'config': 'modelnet', 'B': 8, 'unit': 'us per forward (median of windows)',
            'sine': ss, 'learned': sl}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pos_mlp_ab: no GPU (timings are taken on the device only)')
    dev = torch.device('cuda:0')
    fgreg.load()
    res = {'tool': 'tools/pos_mlp_ab.py', 'device': torch.cuda.get_device_name(0),
           'iters': a.iters, 'rounds': a.rounds,
           'mlp': [mlp_case(n, d, a.iters, a.rounds, dev) for n, d in SHAPES],
           'forward': forward_case(a.steps, a.rounds, dev)}
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
