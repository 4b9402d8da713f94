#!/usr/bin/env python3
"""Golden vectors for TransformerCrossEncoder.get_attentions() (models/transformer/
transformers.py:61-81), computed by running the REFERENCE itself.

TEST INFRASTRUCTURE ONLY, beside make_golden.py (whose helpers it imports and which it leaves
untouched): it needs the reference checkout and oracle/_ref/libkpconv_ref.so, and runs on the
CPU. Only the .npz files it writes travel; they hold arrays only.

  attn_modelnet_small.npz      the maps of forward_modelnet_small's forward (same config, pairs
                               and seed; pre-norm, forward_pre)
  attn_modelnet_postnorm.npz   the maps of forward_modelnet_postnorm's forward (forward_post)

The four full stacks ((L, B, Ns, Ns), (L, B, Nt, Nt), (L, B, Ns, Nt), (L, B, Nt, Ns)) are
about 10.5 MB per model, so a fixture stores a row subset: for every layer, pair and map the
query rows 0, 32, 64, ... plus the cloud's last valid row, with ALL key columns (the padded
ones included: they are exactly 0 in the reference). Keys:

  lens                       (2B,) coarse lengths, src clouds then tgt clouds
  shape.<map>                the reference's full shape of the stack
  rows.src.<b>, rows.tgt.<b> the stored query rows of pair b's src / tgt cloud
  <map>.<b>                  (L, len(rows), Nk_max) rows of pair b, map in src_satt, tgt_satt,
                             src_xatt, tgt_xatt
  max_prob                   the largest weight of the forward

The generator asserts what the tests rely on: every valid row sums to 1 within 1e-6, padded key
columns are exactly 0, and the model's outputs equal the forward fixture's bit for bit (the same
forward was run).

Usage:  python tests/golden/make_golden_attention.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_golden as mg  # noqa: E402

STEP = 32
MAPS = ('src_satt', 'tgt_satt', 'src_xatt', 'tgt_xatt')


def stored_rows(n):
    """Query rows 0, STEP, 2 STEP, ... and the last valid row of a cloud of n rows."""
    return np.unique(np.append(np.arange(0, n, STEP), n - 1)).astype(np.int64)


def pack(model, out, forward_name):
    fwd = np.load(os.path.join(HERE, forward_name + '.npz'))
    B = len(out['src_feat'])
    for b in range(B):                       # the forward this fixture belongs to
        assert np.array_equal(out['src_feat'][b].numpy(), fwd[f'out.src_feat.{b}']), forward_name
    (src_satt, tgt_satt), (src_xatt, tgt_xatt) = model.transformer_encoder.get_attentions()
    stacks = dict(zip(MAPS, (src_satt, tgt_satt, src_xatt, tgt_xatt)))
    lens = [t.shape[0] for t in out['src_kp']] + [t.shape[0] for t in out['tgt_kp']]
    ns, nt = max(lens[:B]), max(lens[B:])
    L = src_satt.shape[0]
    assert tuple(src_satt.shape) == (L, B, ns, ns) and tuple(tgt_satt.shape) == (L, B, nt, nt)
    assert tuple(src_xatt.shape) == (L, B, ns, nt) and tuple(tgt_xatt.shape) == (L, B, nt, ns)
    arrays = {'lens': np.asarray(lens, np.int64)}
    top = 0.0
    for name, t in stacks.items():
        arrays[f'shape.{name}'] = np.asarray(t.shape, np.int64)
    for b in range(B):
        n_of = {'src': lens[b], 'tgt': lens[B + b]}
        for side in ('src', 'tgt'):
            arrays[f'rows.{side}.{b}'] = stored_rows(n_of[side])
        for name, t in stacks.items():
            q_side = name[:3]
            k_side = q_side if 'satt' in name else ('tgt' if q_side == 'src' else 'src')
            a = t[:, b].numpy()
            nq, nk = n_of[q_side], n_of[k_side]
            assert a.dtype == np.float32
            assert np.abs(a[:, :nq, :nk].astype(np.float64).sum(-1) - 1).max() < 1e-6, name
            assert not a[:, :, nk:].any(), (name, 'padded key columns must be exactly 0')
            assert np.isfinite(a).all()
            top = max(top, float(a[:, :nq].max()))
            arrays[f'{name}.{b}'] = np.ascontiguousarray(a[:, arrays[f'rows.{q_side}.{b}']])
    arrays['max_prob'] = np.float64(top)
    print(f'{forward_name}: lens {lens}, largest weight {top:.4g}')
    return arrays


def make(fr, fk):
    # forward_modelnet_small (make_golden.make_forward (1))
    cfg = mg.load_cfg('modelnet.yaml', **mg.SMALL_MODELNET)
    pairs = [mg.modelnet_like_pair(i, n_raw=512) for i in range(2)]
    model, _, out = mg.run_forward(fr, fk, cfg, [p[0] for p in pairs], [p[1] for p in pairs])
    mg.save('attn_modelnet_small', **pack(model, out, 'forward_modelnet_small'))
    # forward_modelnet_postnorm (make_golden.make_forward_postnorm)
    cfg = mg.load_cfg('modelnet.yaml', **dict(mg.SMALL_MODELNET, pre_norm=False))
    pairs = [mg.modelnet_like_pair(i + 9, n_raw=512) for i in range(2)]
    model, _, out = mg.run_forward(fr, fk, cfg, [p[0] for p in pairs], [p[1] for p in pairs],
                                   seed=11)
    mg.save('attn_modelnet_postnorm', **pack(model, out, 'forward_modelnet_postnorm'))


if __name__ == '__main__':
    make(*mg.import_reference())
