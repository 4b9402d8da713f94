#!/usr/bin/env python3
"""Golden vectors for ``transformer_act: gelu`` (models/transformer/transformers.py:265-273:
_get_activation_fn returns F.gelu, the exact erf form), computed by running the REFERENCE
itself.

TEST INFRASTRUCTURE ONLY, beside make_golden.py (whose helpers it imports and which it leaves
untouched): it needs the reference checkout and oracle/_ref/libkpconv_ref.so, and runs on the
CPU. Only the .npz files it writes travel.

  forward_modelnet_gelu.npz           forward_modelnet_small's config, pairs and seed plus
                                      transformer_act='gelu' (pre-norm, forward_pre)
  forward_modelnet_gelu_postnorm.npz  the same with pre_norm=False (forward_post)
  train_modelnet_gelu.npz             make_golden.make_train's recipe on the GELU model: losses,
                                      gnorm / gsum of every parameter, the full gradient of
                                      TRAIN_FULL_GRADS and of layer 0's linear1.{weight, bias}

Weights are named_weights.named_value(key, shape, seed), so the fixtures store key / shape
lists and seeds, not weights. The activation has no parameters: the key list is the ReLU
model's.

The forward fixture must be able to tell the two activations apart: the generator asserts that
the reference's src_feat with GELU differs from forward_modelnet_small's by rel_err > 1e-2
(100 x the forward tests' 1e-4 tolerance, the condition MIN_DIFF states for the learned
positional embedding). Observed here: 0.134 / 0.134 (pairs 0 / 1). The post-norm fixture has no
ReLU twin on the same pairs (forward_modelnet_postnorm uses other pairs and another seed), so
the generator asserts the same condition for it against a ReLU run of the reference made on
the spot: 0.143 / 0.132.

The training fixture is run exactly as make_golden.make_train runs its own (torch's default
thread count; see make_golden_learned_pe.py on why that matters at the network's ReLU kinks --
the KPConv / Res2Net encoder keeps its ReLUs, only the transformer's FFN is smooth now).

Usage:  python tests/golden/make_golden_gelu.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_golden as mg  # noqa: E402

GELU = dict(mg.SMALL_MODELNET, transformer_act='gelu')
GELU_POST = dict(GELU, pre_norm=False)
MIN_DIFF = 1e-2        # GELU vs ReLU src_feat, rel_err (tolerance of the tests: 1e-4)
L0_FFN = ('transformer_encoder.layers.0.linear1.weight', 'transformer_encoder.layers.0.linear1.bias')


def _rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))


def _pairs():
    pairs = [mg.modelnet_like_pair(i, n_raw=512) for i in range(2)]     # forward_modelnet_small's
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _assert_differs(out, relu_feat, what):
    for b in range(2):
        diff = _rel_err(out['src_feat'][b].numpy(), relu_feat[b])
        print(f'{what}: gelu vs relu src_feat.{b}: rel_err {diff:.3g}')
        assert diff > MIN_DIFF, ('the fixture cannot tell the activations apart', what, b, diff)


def make_forward(fr, fk):
    src, tgt = _pairs()
    cfg = mg.load_cfg('modelnet.yaml', **GELU)
    model, meta, out = mg.run_forward(fr, fk, cfg, src, tgt)
    assert model.transformer_encoder.layers[0].activation is torch.nn.functional.gelu
    relu = np.load(os.path.join(HERE, 'forward_modelnet_small.npz'))
    assert repr([(k, list(sh)) for k, sh in model.sd_keys_shapes]) == _keys_repr(relu), \
        'the key list is the ReLU model\'s'
    _assert_differs(out, [relu[f'out.src_feat.{b}'] for b in range(2)], 'pre-norm')
    mg.save('forward_modelnet_gelu', **mg.pack_forward(model, meta, out, GELU, src, tgt, 4.0))

    cfg = mg.load_cfg('modelnet.yaml', **GELU_POST)
    model, meta, out = mg.run_forward(fr, fk, cfg, src, tgt)
    assert model.transformer_encoder.layers[0].activation is torch.nn.functional.gelu
    assert not model.transformer_encoder.layers[0].normalize_before
    _, _, out_relu = mg.run_forward(fr, fk, mg.load_cfg('modelnet.yaml', **dict(GELU_POST, transformer_act='relu')),
                                    src, tgt)
    _assert_differs(out, [t.numpy() for t in out_relu['src_feat']], 'post-norm')
    mg.save('forward_modelnet_gelu_postnorm',
            **mg.pack_forward(model, meta, out, GELU_POST, src, tgt, 4.0))


def _keys_repr(npz):
    raw = npz['sd_keys'].item()
    return raw.decode() if isinstance(raw, bytes) else str(raw)


def make_train(fr, fk):
    """make_golden.make_train on the GELU model (same pairs, seed, loss inputs)."""
    src, tgt = _pairs()
    cfg = mg.load_cfg('modelnet.yaml', **GELU)
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
    n_ffn = 0
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.double()
        arrays[f'gnorm.{k}'] = np.float64(g.norm().item())
        arrays[f'gsum.{k}'] = np.float64(g.sum().item())
        if k in mg.TRAIN_FULL_GRADS or k in L0_FFN:
            arrays[f'grad.{k}'] = p.grad.numpy()
            n_ffn += k in L0_FFN
    assert n_ffn == 2, n_ffn
    mg.save('train_modelnet_gelu', **arrays)


if __name__ == '__main__':
    fr, fk = mg.import_reference()
    make_forward(fr, fk)
    make_train(fr, fk)
