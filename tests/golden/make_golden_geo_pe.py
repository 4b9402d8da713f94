#!/usr/bin/env python3
"""Golden vectors for ``pos_emb_type: geometric`` (GeometricStructureEmbedding,
models/transformer/position_embedding.py:129-196), computed by running the REFERENCE itself.

TEST INFRASTRUCTURE ONLY, beside make_golden.py (whose helpers it imports and which it leaves
untouched): it needs the reference checkout and oracle/_ref/libkpconv_ref.so, and runs on the
CPU. Only the .npz files it writes travel.

  pos_embed_geo.npz               the reference class alone, hidden_dim 256, angle_k 3, both
                                  reduction_a values, on one cloud of 100 points at ModelNet
                                  scale (|x| <= 1) and one at 3DMatch scale (a few metres,
                                  off-centre). Also stored, per scale and reduction:
                                  ``e_ref`` = the reference's own error against the fp64
                                  restatement tests/_geo_ref.py (rel_err), which is the error
                                  of its expansion-form fp32 distances (x^2 - 2 x.y + y^2)
  forward_modelnet_geo_pe.npz     forward_modelnet_small's config, pairs and seed on the
                                  reference RegTR with, after construction,
                                  ``model.pos_embed = GeometricStructureEmbedding(cfg.d_embed,
                                  sigma_d=SIGMA_D)`` and ``model.Geoembeding = True`` (attribute
                                  assignment only: the reference has no conf key for it)
  train_modelnet_geo_pe.npz       make_golden.make_train's recipe on that model: losses, gnorm /
                                  gsum of every parameter, the full gradient of the four
                                  pos_embed.proj_* tensors and of TRAIN_FULL_GRADS

sigma_d: the class default 0.2 is a 3DMatch value (metres; coarse spacing ~0.2 m). The ModelNet
clouds live in the unit cube and their coarse points are ~0.07 apart (median nearest-neighbour
distance of the fixture's coarse clouds: 0.069), so the model fixtures use SIGMA_D = 0.05
(d_ij ~ 1..3, the range the default gives at 3DMatch scale). It is stored in the
fixture's cfg_overrides as ``geo_sigma_d``.

Weights are named_weights.named_value(key, shape, seed); ``embedding.div_term`` is a buffer of
constants and keeps the reference's own values (stored under ``sd.``, like the kernel points).

The generator asserts that on the class fixture's inputs the reference's own knn_id sets equal
the fp64 nearest-neighbour sets (no duplicate points, no near tie that its fp32 distances rank
the other way), and that the forward fixture can tell the embeddings apart: src_feat differs from
forward_modelnet_small's by rel_err > 1e-2.

Usage:  python tests/golden/make_golden_geo_pe.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
import make_golden as mg  # noqa: E402
import _geo_ref as gr  # noqa: E402
from named_weights import named_state_dict, named_value  # noqa: E402

SIGMA_D = 0.05
GEO = dict(mg.SMALL_MODELNET, pos_emb_type='geometric', geo_sigma_d=SIGMA_D)
PE_SEED = 3
PE_POINTS = 100
PE_DIM = 256
PE_K = 3
MIN_DIFF = 1e-2        # geometric vs sine src_feat, rel_err (tolerance of the tests: 1e-4)
PROJ_KEYS = [f'pos_embed.proj_{p}.{t}' for p in 'da' for t in ('weight', 'bias')]


def _rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))


def make_pos_embed_geo():
    from models.transformer.position_embedding import GeometricStructureEmbedding
    rng = np.random.default_rng(PE_SEED)
    pts = {
        'modelnet': rng.uniform(-1.0, 1.0, (PE_POINTS, 3)),
        '3dmatch': rng.uniform(-1.5, 1.5, (PE_POINTS, 3)) + np.array([2.5, -1.0, 1.2]),
    }
    arrays = {'sd_seed': np.int64(PE_SEED), 'angle_k': np.int64(PE_K)}
    for red in ('max', 'mean'):
        m = GeometricStructureEmbedding(PE_DIM, angle_k=PE_K, reduction_a=red).eval()
        sd = m.state_dict()
        keys = [(k, list(v.shape)) for k, v in sd.items()]
        new = {k: torch.from_numpy(named_value(k, s, PE_SEED, 0.0)) for k, s in keys}
        new['embedding.div_term'] = sd['embedding.div_term']       # constants, not weights
        m.load_state_dict(new)
        arrays['sd_keys'] = np.bytes_(repr(keys))
        arrays['div_term'] = sd['embedding.div_term'].numpy()
        for name, p in pts.items():
            x = torch.from_numpy(p.astype(np.float32))
            with torch.no_grad():
                y = m(x.unsqueeze(0))
                knn_id = m.get_embedding_indices(x.unsqueeze(0))[2][0].numpy()
            assert tuple(y.shape) == (PE_POINTS, PE_DIM)
            nn64 = gr.knn(x.numpy(), [PE_POINTS], PE_K)
            assert all(set(knn_id[i]) == set(nn64[i]) for i in range(PE_POINTS)), name
            assert float(gr.knn_margin(x.numpy(), [PE_POINTS], PE_K).min()) > 1e-3, name
            y64 = gr.forward(x.numpy(), [PE_POINTS], PE_K, m.sigma_d, m.sigma_a,
                             sd['embedding.div_term'].double(), new['proj_d.weight'],
                             new['proj_d.bias'], new['proj_a.weight'], new['proj_a.bias'], red)
            e_ref = _rel_err(y.numpy(), y64.numpy())
            print(f'pos_embed_geo {name} {red}: reference vs fp64 restatement rel_err {e_ref:.3g}')
            arrays[f'in.{name}'] = x.numpy()
            arrays[f'out.{name}.{red}'] = y.numpy()
            arrays[f'e_ref.{name}.{red}'] = np.float64(e_ref)
    mg.save('pos_embed_geo', **arrays)


def _pairs():
    pairs = [mg.modelnet_like_pair(i, n_raw=512) for i in range(2)]     # forward_modelnet_small's
    return [p[0] for p in pairs], [p[1] for p in pairs]


def run_forward(fr, fk, src, tgt, bias=4.0, seed=0):
    """make_golden.run_forward with the structure embedding switched on between construction
    and the weight load (the reference is not edited)."""
    from models.transformer.position_embedding import GeometricStructureEmbedding
    cfg = mg.load_cfg('modelnet.yaml', **mg.SMALL_MODELNET)
    torch.manual_seed(seed)
    np.random.seed(seed)
    cwd = os.getcwd()
    os.chdir(mg.REF)
    try:
        model = fr.RegTR(cfg)
    finally:
        os.chdir(cwd)
    model.pos_embed = GeometricStructureEmbedding(cfg.d_embed, sigma_d=SIGMA_D)
    model.Geoembeding = True
    model.preprocessor = fk.Preprocessor(cfg)
    sd = model.state_dict()
    keys_shapes = [(k, tuple(v.shape)) for k, v in sd.items() if not k.startswith('feature_criterion')]
    stored = {k: v.numpy() for k, v in sd.items() if 'kernel_points' in k or k.endswith('div_term')}
    vals = named_state_dict(keys_shapes, seed, bias, stored)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in vals.items()},
                                                strict=False)
    assert not unexpected and all(k.startswith('feature_criterion') for k in missing), missing
    model.sd_keys_shapes, model.sd_seed = keys_shapes, seed
    model.eval()
    batch = {'src_xyz': [torch.from_numpy(c) for c in src],
             'tgt_xyz': [torch.from_numpy(c) for c in tgt]}
    with torch.no_grad(), mg.cuda_to_cpu():
        out = model(batch)
    return model, batch['kpconv_meta'], out


def make_forward(fr, fk):
    src, tgt = _pairs()
    model, meta, out = run_forward(fr, fk, src, tgt)
    keys = [k for k, _ in model.sd_keys_shapes]
    assert all(k in keys for k in PROJ_KEYS) and 'pos_embed.embedding.div_term' in keys
    xyz_c = meta['points'][-1].numpy()
    lens = [int(n) for n in meta['stack_lengths'][-1]]
    nn = gr.knn(xyz_c, lens, 3)
    d1 = np.linalg.norm(xyz_c[nn[:, 0]] - xyz_c, axis=1)
    print(f'coarse clouds {lens}: nearest-neighbour distance median {np.median(d1):.3f}, '
          f'/ SIGMA_D = {np.median(d1) / SIGMA_D:.2f}; smallest knn margin '
          f'{gr.knn_margin(xyz_c, lens, 3).min():.3g}')
    sine = np.load(os.path.join(HERE, 'forward_modelnet_small.npz'))
    for b in range(2):
        diff = _rel_err(out['src_feat'][b].numpy(), sine[f'out.src_feat.{b}'])
        print(f'geometric vs sine src_feat.{b}: rel_err {diff:.3g}')
        assert diff > MIN_DIFF, ('the fixture cannot tell the embeddings apart', b, diff)
    arrays = mg.pack_forward(model, meta, out, GEO, src, tgt, 4.0)
    arrays['sd.pos_embed.embedding.div_term'] = model.state_dict()['pos_embed.embedding.div_term'].numpy()
    arrays['geo_sigma_d'] = np.float64(SIGMA_D)
    mg.save('forward_modelnet_geo_pe', **arrays)


def make_train(fr, fk):
    """make_golden.make_train on the geometric-PE model (same pairs, seed, loss inputs)."""
    src, tgt = _pairs()
    model, meta, out = run_forward(fr, fk, src, tgt)
    lf = np.load(os.path.join(HERE, 'loss_modelnet_small.npz'))
    model.feature_criterion.W.data.copy_(torch.from_numpy(lf['W']))
    model.feature_criterion_un.W.data.copy_(torch.from_numpy(lf['W_un']))
    model.train()
    batch = {'src_xyz': [torch.from_numpy(c) for c in src],
             'tgt_xyz': [torch.from_numpy(c) for c in tgt],
             'pose': torch.from_numpy(lf['pose']),
             'src_overlap': [torch.from_numpy(lf[f'src_overlap.{b}']) for b in range(2)],
             'tgt_overlap': [torch.from_numpy(lf[f'tgt_overlap.{b}']) for b in range(2)]}
    model.zero_grad()
    with mg.cuda_to_cpu():
        pred = model(batch)
        losses = model.compute_loss(pred, batch)
        losses['total'].backward()
    arrays = {}
    for k, v in losses.items():
        arrays[f'loss.{k}'] = np.float32(v.item())
    n_pe = 0
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.double()
        arrays[f'gnorm.{k}'] = np.float64(g.norm().item())
        arrays[f'gsum.{k}'] = np.float64(g.sum().item())
        if k in mg.TRAIN_FULL_GRADS or k in PROJ_KEYS:
            arrays[f'grad.{k}'] = p.grad.numpy()
            n_pe += k in PROJ_KEYS
    assert n_pe == 4, n_pe
    mg.save('train_modelnet_geo_pe', **arrays)


if __name__ == '__main__':
    fr, fk = mg.import_reference()
    make_pos_embed_geo()
    make_forward(fr, fk)
    make_train(fr, fk)
