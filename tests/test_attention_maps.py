"""CPU twin of test_gpu_attention_maps.py: what the attention-map feature states without a GPU.
The reference fixtures (tests/golden/attn_modelnet_*.npz) have the shapes, rows and sums the GPU
test relies on; the padded layout of layer.satt_weights / xatt_weights equals
nn.MultiheadAttention's own on a padded batch; get_attentions(), the training forward and
fgreg.pipeline refuse what they must before any device work."""
import os

import numpy as np
import pytest
import torch

from _attn_weights_ref import head_mean_weights
from conftest import GOLDEN, forward_fixture, golden

MAPS = ('src_satt', 'tgt_satt', 'src_xatt', 'tgt_xatt')
FIXTURES = {'attn_modelnet_small': ('forward_modelnet_small', [331, 333, 328, 331], 0.0053),
            'attn_modelnet_postnorm': ('forward_modelnet_postnorm', [314, 313, 324, 316], 0.134)}


@pytest.mark.parametrize('name', list(FIXTURES))
def test_reference_fixture(name):
    fwd_name, lens, top = FIXTURES[name]
    assert os.path.getsize(os.path.join(GOLDEN, name + '.npz')) < (1 << 20)
    d, fwd = golden(name), golden(fwd_name)
    B = 2
    assert [int(n) for n in d['lens']] == lens
    assert [fwd[f'out.src_kp.{b}'].shape[0] for b in range(B)] + \
           [fwd[f'out.tgt_kp.{b}'].shape[0] for b in range(B)] == lens
    ns, nt = max(lens[:B]), max(lens[B:])
    L = 3
    want = {'src_satt': (L, B, ns, ns), 'tgt_satt': (L, B, nt, nt), 'src_xatt': (L, B, ns, nt),
            'tgt_xatt': (L, B, nt, ns)}
    n_of = {'src': lens[:B], 'tgt': lens[B:]}
    biggest = 0.0
    for nm in MAPS:
        assert tuple(int(x) for x in d[f'shape.{nm}']) == want[nm]
        q = nm[:3]
        k = q if 'satt' in nm else ('tgt' if q == 'src' else 'src')
        for b in range(B):
            rows = d[f'rows.{q}.{b}']
            n = n_of[q][b]
            assert rows.tolist() == sorted(set(range(0, n, 32)) | {n - 1})
            a = d[f'{nm}.{b}']
            assert a.dtype == np.float32 and a.shape == (L, len(rows), want[nm][3])
            nk = n_of[k][b]
            assert not a[:, :, nk:].any()                            # padded key columns: exact 0
            assert np.abs(a.astype(np.float64).sum(-1) - 1).max() <= 2e-7 * 2    # every stored row is valid
            biggest = max(biggest, float(a.max()))
    assert biggest <= float(d['max_prob']) and abs(float(d['max_prob']) - top) <= 0.05 * top


def test_padded_layout_equals_multihead_attention():
    """_store_maps on packed (N, max_len) maps of 2 pairs of unequal lengths: every (side, pair)
    block equals what nn.MultiheadAttention returns for that pair padded with a
    key_padding_mask (fp64), padded key columns and padded query rows are 0."""
    import fgreg
    from fgreg.transformer import Segments, TransformerCrossEncoderLayer
    nhead, dh, B = 2, 4, 2
    d = nhead * dh
    lens = [5, 9, 7, 4]                                   # src_0, src_1, tgt_0, tgt_1
    g = torch.Generator().manual_seed(3)
    mha = torch.nn.MultiheadAttention(d, nhead).double()
    x = torch.randn(sum(lens), d, generator=g, dtype=torch.float64)
    W, bias = mha.in_proj_weight.detach(), mha.in_proj_bias.detach()
    q, k = x @ W[:d].t() + bias[:d], x @ W[d:2 * d].t() + bias[d:2 * d]
    seg = Segments(lens, 'cpu')
    assert seg.max_len == 9
    packed = [head_mean_weights(q, k, lens, lens, ks, nhead, dh ** -0.5, seg.max_len)
              for ks in ([0, 1, 2, 3], [2, 3, 0, 1])]
    layer = TransformerCrossEncoderLayer(d, nhead, 16, 0.0, normalize_before=True,
                                         sa_val_has_pos_emb=True, ca_val_has_pos_emb=True)
    assert layer.satt_weights is None and layer.xatt_weights is None
    layer._store_maps(packed, seg)
    start = np.cumsum([0] + lens)
    for maps, cross in ((layer.satt_weights, False), (layer.xatt_weights, True)):
        assert isinstance(maps, tuple) and len(maps) == 2
        for s in (0, 1):
            clouds = list(range(s * B, (s + 1) * B))
            keys = [(c + B) % (2 * B) if cross else c for c in clouds]
            nq, nk = max(lens[c] for c in clouds), max(lens[c] for c in keys)
            assert maps[s].shape == (B, nq, nk)
            xq, xk = torch.zeros(nq, B, d, dtype=torch.float64), torch.zeros(nk, B, d, dtype=torch.float64)
            pad = torch.ones(B, nk, dtype=torch.bool)
            for b, (c, kc) in enumerate(zip(clouds, keys)):
                xq[:lens[c], b] = x[start[c]:start[c + 1]]
                xk[:lens[kc], b] = x[start[kc]:start[kc + 1]]
                pad[b, :lens[kc]] = False
            with torch.no_grad():
                _, w = mha(xq, xk, xk, key_padding_mask=pad)
            for b, (c, kc) in enumerate(zip(clouds, keys)):
                got = maps[s][b]
                assert float((got[:lens[c]] - w[b, :lens[c]]).abs().max()) <= 1e-12
                assert not bool(got[lens[c]:].any())                 # padded query rows: 0 here
                assert not bool(got[:, lens[kc]:].any()) and not bool(w[b, :, lens[kc]:].any())
    assert fgreg.RegTR is not None


def test_refusals_need_no_gpu():
    import fgreg
    cfg, sd, src, tgt, _, _ = forward_fixture('forward_modelnet_small')
    model = fgreg.RegTR(cfg).eval()
    enc = model.transformer_encoder
    assert enc.record_attention is False
    assert 'in_proj_tap' not in ''.join(model.state_dict())     # no new state: checkpoints load as before
    with pytest.raises(RuntimeError) as e:
        enc.get_attentions()
    assert str(e.value) == 'no attention maps recorded: set record_attention = True and run a forward'
    batch = {'src_xyz': [torch.from_numpy(s) for s in src], 'tgt_xyz': [torch.from_numpy(t) for t in tgt]}
    enc.record_attention = True
    model.train()
    with pytest.raises(NotImplementedError, match='record_attention'):
        model(batch)
    model.eval()
    with pytest.raises(NotImplementedError, match='record'):
        next(fgreg.pipeline(model, [batch]))
