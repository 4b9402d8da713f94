"""A/B of the geometric structure embedding (fgreg.transformer.GeometricStructureEmbedding,
hidden_dim 256, angle_k 3): the fused path (fgr_geo_embed_indices + fgr_geo_embed_f16x3, two
launches) against the composed path it replaces (the indices kernel, torch sin / cos, two
linear() launches, torch reductions: forward_composed), at the coarse points of a ModelNet B = 8
batch (16 clouds) and of a 3DMatch pair (2 clouds). The 3DMatch model's own d_embed is 512, where
only the composed path exists; its coarse clouds are timed here at the kernel's width, 256.

For scale, the dense O(N^2) formula the reference evaluates -- the sinusoidal embedding of every
pair and triplet of a cloud, two Linears over all of them, then a gather of k columns per row --
is timed in torch on one cloud of about 600 points (``dense``; (N, N, k, 256) fp32 tensors).

Event timing in windows of ``iters`` calls; the two sides alternate over ``rounds`` windows each
and the spread reported is (max - min) of a side's windows, so a difference is to be read against
it. Two figures per side: ``eager`` = back-to-back calls from Python (host launch path included)
and ``graph`` = the same calls captured GRAPH_REPS at a time into a HIP graph and replayed (device
time: what the captured core of the forward pays). The two sides' outputs are compared first.
Writes one JSON object (--out, default stdout).
    python tools/geo_embed_ab.py [--iters 200] [--rounds 7] [--out FILE]"""
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
from fgreg import ops  # noqa: E402
from fgreg.backbone import host_layout  # noqa: E402
from fgreg.transformer import GeometricStructureEmbedding  # noqa: E402

GRAPH_REPS = 20
SHAPES = [('modelnet', 8, 0.05), ('3dmatch', 1, 0.2)]        # config, B, sigma_d


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def stat(t):
    return {'median_us': float(np.median(t)), 'min_us': float(min(t)), 'max_us': float(max(t)),
            'spread_us': float(max(t) - min(t))}


def ab(fa, fb, iters, rounds):
    for _ in range(10):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(fa, iters))
        tb.append(window(fb, iters))
    return stat(ta), stat(tb)


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


def coarse_points(config, B, dev):
    """The coarse level of the model's own pyramid on a synthetic batch -> (xyz, lengths)."""
    from fgreg.synthetic import make_batch
    src, tgt, _ = make_batch(config, B)
    model = fgreg.RegTR(fgreg.config.get(config)).to(dev).eval()
    batch = {'src_xyz': [torch.from_numpy(s).to(dev) for s in src],
             'tgt_xyz': [torch.from_numpy(t).to(dev) for t in tgt]}
    with torch.no_grad():
        meta = model._prepare(batch)
    lens, _ = host_layout(meta, len(meta['points']) - 1)
    return meta['points'][-1].contiguous(), [int(n) for n in lens]


def embed_case(config, B, sigma_d, iters, rounds, dev):
    xyz, lens = coarse_points(config, B, dev)
    torch.manual_seed(len(lens))
    m = GeometricStructureEmbedding(256, sigma_d=sigma_d).to(dev).eval()
    off = ops.offsets(lens, dev)
    fused = lambda: m(xyz, off, lens)                        # noqa: E731
    composed = lambda: m.forward_composed(xyz, off, lens)    # noqa: E731
    with torch.no_grad():
        assert ops.geo_embed_supported(xyz.shape[0], 256, 3)
        a, b = fused(), composed()
        err = float((a - b).abs().max() / b.abs().max())
        sf, sc = ab(fused, composed, iters, rounds)
        gf, gc = ab(captured(fused), captured(composed), max(iters // GRAPH_REPS, 1), rounds)
    for st in (gf, gc):                              # per call, not per replay
        for k in st:
            st[k] /= GRAPH_REPS
    return {'config': config, 'B': B, 'clouds': len(lens), 'n': int(xyz.shape[0]),
            'd_model': 256, 'angle_k': 3, 'rel_err_fused_vs_composed': err,
            'eager': {'fused': sf, 'composed': sc,
                      'speedup_median': sc['median_us'] / sf['median_us']},
            'graph': {'fused': gf, 'composed': gc,
                      'speedup_median': gc['median_us'] / gf['median_us']}}


def dense(m, pts):
    """The O(N^2) formula on one cloud pts (N, 3), in torch: every pair's distance and every
    (pair, neighbour) angle embedded and projected, then the k nearest columns of each row."""
    k, n = m.angle_k, pts.shape[0]
    d2 = (pts * pts).sum(1, keepdim=True) - 2 * pts @ pts.t() + (pts * pts).sum(1)[None, :]
    dist = d2.clamp(min=0).sqrt()
    knn = dist.topk(k + 1, dim=1, largest=False)[1][:, 1:]                  # (N, k)
    ref = pts[knn] - pts[:, None, :]                                        # (N, k, 3)
    anc = pts[None, :, :] - pts[:, None, :]                                 # (N, N, 3)
    ref, anc = ref[:, None, :, :].expand(n, n, k, 3), anc[:, :, None, :].expand(n, n, k, 3)
    ang = torch.atan2(torch.linalg.norm(torch.cross(ref, anc, dim=-1), dim=-1),
                      (ref * anc).sum(-1)) * m.factor_a                     # (N, N, k)
    pd = torch.nn.functional.linear(m.embedding(dist / m.sigma_d), m.proj_d.weight, m.proj_d.bias)
    pa = torch.nn.functional.linear(m.embedding(ang), m.proj_a.weight, m.proj_a.bias)
    pa = pa.max(dim=2)[0] if m.reduction_a == 'max' else pa.mean(dim=2)
    emb = pd + pa                                                           # (N, N, D)
    return torch.gather(emb, 1, knn[:, :, None].expand(n, k, emb.shape[-1])).max(dim=1)[0]


def dense_case(rounds, dev):
    xyz, lens = coarse_points('3dmatch', 1, dev)
    n = min(600, lens[0])                     # the first 600 coarse points of the source cloud
    pts = xyz[:n].contiguous()
    torch.manual_seed(1)
    m = GeometricStructureEmbedding(256).to(dev).eval()
    lens = [n]
    off = ops.offsets(lens, dev)
    with torch.no_grad():
        a, b = m(pts, off, lens[:1]), dense(m, pts)
        err = float((a - b).abs().max() / b.abs().max())
        for _ in range(3):
            dense(m, pts)
        t = [window(lambda: dense(m, pts), 3) for _ in range(rounds)]
        f = [window(lambda: m(pts, off, lens[:1]), 50) for _ in range(rounds)]
    return {'n': int(pts.shape[0]), 'rel_err_fused_vs_dense': err, 'dense_torch': stat(t),
            'fused': stat(f)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('geo_embed_ab: no GPU (timings are taken on the device only)')
    dev = torch.device('cuda:0')
    fgreg.load()
    res = {'tool': 'tools/geo_embed_ab.py', 'device': torch.cuda.get_device_name(0),
           'iters': a.iters, 'rounds': a.rounds, 'graph_reps': GRAPH_REPS,
           'embed': [embed_case(c, B, s, a.iters, a.rounds, dev) for c, B, s in SHAPES],
           'dense': dense_case(a.rounds, dev)}
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
