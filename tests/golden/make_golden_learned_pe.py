#!/usr/bin/env python3
"""Golden vectors for ``pos_emb_type: learned`` (PositionEmbeddingLearned,
models/transformer/position_embedding.py:52-71), computed by running the REFERENCE itself.

TEST INFRASTRUCTURE ONLY, beside make_golden.py (whose helpers it imports and which it leaves
untouched): it needs the reference checkout and oracle/_ref/libkpconv_ref.so, and runs on the
CPU. Only the .npz files it writes travel.

  pos_embed_learned.npz                    the reference class alone, d_model 256 and 512, on
                                           points at ModelNet scale (|x| <= 1), at 3DMatch scale
                                           (a few metres, off-centre) and one all-zero point
  forward_modelnet_learned_pe.npz          forward_modelnet_small's config, pairs and seed plus
                                           pos_emb_type='learned'
  forward_modelnet_learned_pe_decoder.npz  the same with direct_regress_coor=False: the MLP is
                                           then in the state_dict under pos_embed.* and under
                                           correspondence_decoder.pos_embed.* (one module)
  train_modelnet_learned_pe.npz            make_golden.make_train's recipe on the learned-PE
                                           model: losses, gnorm / gsum of every parameter, the
                                           full gradient of the ten pos_embed.mlp.* tensors and
                                           of TRAIN_FULL_GRADS

Weights are named_weights.named_value(key, shape, seed), so the fixtures store key / shape
lists and seeds, not weights.

The forward fixture must be able to tell the two embeddings apart: the generator asserts that
the reference's src_feat with the learned embedding differs from forward_modelnet_small's by
rel_err > 1e-2 (the test tolerance is 1e-4). Observed here: 0.62 (pair 0), 0.63 (pair 1).

The training fixture is run exactly as make_golden.make_train runs its own (torch's default
thread count). That matters: this network's gradient is discontinuous at ReLU kinks
(tests/test_gpu_train.py, module docstring), and the reference itself lands on either side of
one of them depending on its GEMMs' summation order -- with torch.set_num_threads(1) instead,
the reference's own gradient of kpf_encoder.encoder_blocks.1.res2net.layer1.0.bn3.bias (and of
that block's downsample.1.bias) moves by 1.1e-2 relative Frobenius, for the learned and for
the sine model alike (train_modelnet_small's recipe has the same property); every other
stored figure moves by less than 1e-2.

Usage:  python tests/golden/make_golden_learned_pe.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_golden as mg  # noqa: E402
from named_weights import named_value  # noqa: E402

LEARNED = dict(mg.SMALL_MODELNET, pos_emb_type='learned')
PE_SEED = 3
PE_POINTS = 100
MIN_DIFF = 1e-2        # learned vs sine src_feat, rel_err (tolerance of the tests: 1e-4)


def _rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))


def make_pos_embed_learned():
    from models.transformer.position_embedding import PositionEmbeddingLearned
    rng = np.random.default_rng(PE_SEED)
    pts = {
        'modelnet': rng.uniform(-1.0, 1.0, (PE_POINTS, 3)),
        '3dmatch': rng.uniform(-1.5, 1.5, (PE_POINTS, 3)) + np.array([2.5, -1.0, 1.2]),
    }
    pts['modelnet'][17] = 0.0                       # an all-zero point
    arrays = {'sd_seed': np.int64(PE_SEED)}
    for d in (256, 512):
        m = PositionEmbeddingLearned(3, d).eval()
        sd = m.state_dict()
        keys = [(k, list(v.shape)) for k, v in sd.items()]
        m.load_state_dict({k: torch.from_numpy(named_value(k, s, PE_SEED, 0.0)) for k, s in keys})
        arrays[f'sd_keys.{d}'] = np.bytes_(repr(keys))
        for name, p in pts.items():
            x = torch.from_numpy(p.astype(np.float32))
            with torch.no_grad():
                y = m(x)
            arrays[f'in.{name}'] = x.numpy()
            arrays[f'out.{name}.{d}'] = y.numpy()
    mg.save('pos_embed_learned', **arrays)


def _pairs():
    pairs = [mg.modelnet_like_pair(i, n_raw=512) for i in range(2)]     # forward_modelnet_small's
    return [p[0] for p in pairs], [p[1] for p in pairs]


def make_forward(fr, fk):
    src, tgt = _pairs()
    cfg = mg.load_cfg('modelnet.yaml', **LEARNED)
    model, meta, out = mg.run_forward(fr, fk, cfg, src, tgt)
    assert any(k.startswith('pos_embed.mlp.') for k, _ in model.sd_keys_shapes)
    sine = np.load(os.path.join(HERE, 'forward_modelnet_small.npz'))
    for b in range(2):
        diff = _rel_err(out['src_feat'][b].numpy(), sine[f'out.src_feat.{b}'])
        print(f'learned vs sine src_feat.{b}: rel_err {diff:.3g}')
        assert diff > MIN_DIFF, ('the fixture cannot tell the embeddings apart', b, diff)
    mg.save('forward_modelnet_learned_pe', **mg.pack_forward(model, meta, out, LEARNED, src, tgt, 4.0))

    over = dict(LEARNED, direct_regress_coor=False)
    cfg = mg.load_cfg('modelnet.yaml', **over)
    model, meta, out = mg.run_forward(fr, fk, cfg, src, tgt)
    keys = [k for k, _ in model.sd_keys_shapes]
    assert 'pos_embed.mlp.8.weight' in keys and 'correspondence_decoder.pos_embed.mlp.8.weight' in keys
    mg.save('forward_modelnet_learned_pe_decoder',
            **mg.pack_forward(model, meta, out, over, src, tgt, 4.0))


def make_train(fr, fk):
    """make_golden.make_train on the learned-PE model (same pairs, seed, loss inputs)."""
    src, tgt = _pairs()
    cfg = mg.load_cfg('modelnet.yaml', **LEARNED)
    model, meta, out = mg.run_forward(fr, fk, cfg, src, tgt)
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
        if k in mg.TRAIN_FULL_GRADS or k.startswith('pos_embed.mlp.'):
            arrays[f'grad.{k}'] = p.grad.numpy()
            n_pe += k.startswith('pos_embed.mlp.')
    assert n_pe == 10, n_pe
    mg.save('train_modelnet_learned_pe', **arrays)


if __name__ == '__main__':
    fr, fk = mg.import_reference()
    make_pos_embed_learned()
    make_forward(fr, fk)
    make_train(fr, fk)
