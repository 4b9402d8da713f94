"""TransformerCrossEncoder.get_attentions() on the GPU (record_attention, the recording route of
fgreg/transformer.py and fgreg/regtr.py).

1. Against the reference's own maps (tests/golden/attn_modelnet_small.npz, attn_modelnet_postnorm
   .npz: a row subset of get_attentions() of the forward_modelnet_small / _postnorm forwards,
   tests/golden/make_golden_attention.py): the forward parity bound of test_gpu_forward.py per
   map, rel_err <= 1e-4 and elem_err <= 1e-3; in the bf16 mode the bound of test_gpu_bf16.py.
   Shapes equal the reference's, padded key columns and padded query rows are 0.
2. At d_embed 256 / 8 heads (head dim 32) on seeded weights: against the fp64 attention of the
   q / k that a forward hook on every layer's in_proj_tap captured, with the kernel test's bound.
3. Recording leaves the plain forward alone: outputs of a recording forward within 1e-4 of a
   plain one, the next plain forward bit-equal to the one before, a captured graph still
   replayed, recording forwards not counted as sightings.
4. The drop-in finegrained_regtr.RegTR returns the same tensors.
"""
import numpy as np
import pytest
import torch

from _attn_weights_ref import head_mean_weights, valid_mask
from conftest import elem_err, forward_fixture, golden, rel_err

pytestmark = pytest.mark.gpu
TOL, ELEM_TOL = 1e-4, 1e-3          # test_gpu_forward.py: TOL, ELEM_TOL (floor 1e-2)
BF16_TOL = 5e-2                     # test_gpu_bf16.py: BF16_FEAT_TOL (normwise)
MAPS = ('src_satt', 'tgt_satt', 'src_xatt', 'tgt_xatt')
KEYS = ['src_feat_un', 'tgt_feat_un', 'src_feat', 'tgt_feat', 'src_kp_warped', 'tgt_kp_warped',
        'src_overlap', 'tgt_overlap']
FIXTURES = {'attn_modelnet_small': 'forward_modelnet_small',
            'attn_modelnet_postnorm': 'forward_modelnet_postnorm'}


def _model(cfg, sd, dev, cls=None):
    import fgreg
    m = (cls or fgreg.RegTR)(cfg)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith('feature_criterion') for k in missing)
    return m.to(dev).eval()


def _batch(src, tgt, dev):
    return {'src_xyz': [torch.from_numpy(np.asarray(s)).to(dev) for s in src],
            'tgt_xyz': [torch.from_numpy(np.asarray(t)).to(dev) for t in tgt]}


def _fixture_model(name, dev, cls=None):
    import fgreg
    cfg, sd, src, tgt, meta, _ = forward_fixture(FIXTURES[name])
    model = _model(cfg, sd, dev, cls)
    model.preprocessor = fgreg.FixedMetaPreprocessor({k: [t.to(dev) for t in v]
                                                      for k, v in meta.items()})
    return model, src, tgt


def _named(att):
    (src_satt, tgt_satt), (src_xatt, tgt_xatt) = att
    return dict(zip(MAPS, (src_satt, tgt_satt, src_xatt, tgt_xatt)))


def _sides(name):
    q = name[:3]
    return q, (q if 'satt' in name else ('tgt' if q == 'src' else 'src'))


def _check_padding(maps, lens):
    """Padded key columns and padded query rows of every (L, B, Nq, Nk) stack are 0."""
    B = len(lens) // 2
    n_of = {'src': lens[:B], 'tgt': lens[B:]}
    for name, t in maps.items():
        q, k = _sides(name)
        assert t.dtype == torch.float32 and t.shape[1] == B
        assert tuple(t.shape[2:]) == (max(n_of[q]), max(n_of[k]))
        for b in range(B):
            assert not bool(t[:, b, :, n_of[k][b]:].any()), (name, b, 'padded key columns')
            assert not bool(t[:, b, n_of[q][b]:].any()), (name, b, 'padded query rows')
            s = t[:, b, :n_of[q][b]].double().sum(-1)
            assert float((s - 1).abs().max()) <= n_of[k][b] * 2.0 ** -23, (name, b)


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', list(FIXTURES))
def test_maps_match_reference(gpu, name, mode):
    import fgreg
    ref = golden(name)
    old = fgreg.precision()
    fgreg.set_precision(mode)
    try:
        model, src, tgt = _fixture_model(name, gpu)
        plain = model(_batch(src, tgt, gpu))
        model.transformer_encoder.record_attention = True
        rec = model(_batch(src, tgt, gpu))
        maps = _named(model.transformer_encoder.get_attentions())
    finally:
        fgreg.set_precision(old)
    lens = [int(n) for n in ref['lens']]
    B = len(lens) // 2
    assert [t.shape[0] for t in rec['src_kp']] + [t.shape[0] for t in rec['tgt_kp']] == lens
    for nm, t in maps.items():
        assert tuple(t.shape) == tuple(int(x) for x in ref[f'shape.{nm}']), nm
    _check_padding(maps, lens)
    tol = TOL if mode == 'fp32' else BF16_TOL
    for nm, t in maps.items():
        q, _ = _sides(nm)
        for b in range(B):
            rows = torch.from_numpy(ref[f'rows.{q}.{b}']).to(gpu)
            got, want = t[:, b].index_select(1, rows), ref[f'{nm}.{b}']
            e, ee = rel_err(got, want), elem_err(got, want)
            print(f'attention-maps {name} {mode} {nm}.{b}: rel_err {e:.3e} elem_err {ee:.3e}')
            assert e <= tol, (nm, b, e)
            if mode == 'fp32':
                assert ee <= ELEM_TOL, (nm, b, ee)
    # the recording route computes what the plain forward computes, up to rounding (asserted in
    # the fp32-accurate mode; the bf16 routes round q / k / v at different points: printed)
    worst = max(rel_err(rec[k][b], plain[k][b]) for k in KEYS for b in range(B))
    print(f'attention-maps {name} {mode}: recording vs plain forward, worst rel_err {worst:.3e}')
    if mode == 'fp32':
        assert worst <= TOL
        assert float((rec['pose'] - plain['pose']).abs().max()) <= TOL


def _seeded_model(cfg, seed, dev):
    import fgreg
    torch.manual_seed(seed)
    np.random.seed(seed)
    m = fgreg.RegTR(cfg)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.75 + 0.5 * torch.rand(mod.running_var.shape, generator=g))
        m.correspondence_decoder.conf_logits_decoder.bias.fill_(4.0)
    return m.to(dev).eval()


def test_maps_head_dim_32_and_plain_forward_untouched(gpu):
    """d_embed 256 / 8 heads on a B = 2 batch of modelnet_like_pair clouds. The maps against fp64
    attention of the hooked q / k (bound of test_gpu_attention_weights.py: elem_err floor 1e-3
    over the valid columns <= max(4 x the fp32 restatement's, 1e-6)); then the plain forward is
    what it was: bit-equal outputs, the captured graph replayed, no sighting counted."""
    import fgreg.config as fc
    import fgreg.regtr as rt
    from fgreg.synthetic import make_batch
    cfg = fc.get('modelnet')
    assert cfg.d_embed == 256 and cfg.nhead == 8
    model = _seeded_model(cfg, 23, gpu)
    enc = model.transformer_encoder
    src, tgt, _ = make_batch('modelnet_like', 2)
    old = rt.GRAPHS
    rt.GRAPHS = True
    taps, hooks = [], []
    try:
        # recording forwards are no sightings: nothing is remembered, nothing captured
        enc.record_attention = True
        model(_batch(src, tgt, gpu))
        model(_batch(src, tgt, gpu))
        assert rt._GRAPHS.get(model) is None
        enc.record_attention = False
        for _ in range(2):
            model(_batch(src, tgt, gpu))
        assert len(rt._GRAPHS[model]['graphs']) == 1           # second sighting: captured
        before = model(_batch(src, tgt, gpu))                  # a replay
        graph = next(iter(rt._GRAPHS[model]['graphs'].values()))
        for layer in enc.layers:
            hooks.append(layer.in_proj_tap.register_forward_hook(
                lambda mod, args, out: taps.append(tuple(t.detach().cpu() for t in out))))
        enc.record_attention = True
        rec = model(_batch(src, tgt, gpu))
        maps = _named(enc.get_attentions())
        enc.record_attention = False
        after = model(_batch(src, tgt, gpu))
        assert len(rt._GRAPHS[model]['graphs']) == 1
        assert next(iter(rt._GRAPHS[model]['graphs'].values())) is graph
    finally:
        rt.GRAPHS = old
        enc.record_attention = False
        for h in hooks:
            h.remove()
    L = len(enc.layers)
    assert len(taps) == 2 * L                                  # self, cross of every layer; no more
    for k in KEYS:
        for b in range(2):
            assert torch.equal(after[k][b], before[k][b]), k
            assert rel_err(rec[k][b], before[k][b]) <= TOL, (k, b)
    assert torch.equal(after['pose'], before['pose'])

    lens = [t.shape[0] for t in rec['src_kp']] + [t.shape[0] for t in rec['tgt_kp']]
    _check_padding(maps, lens)
    B, start = 2, np.cumsum([0] + lens)
    scale = float(np.float32(np.sqrt(1.0 / 32)))
    for l in range(L):
        for i, kind in enumerate(('satt', 'xatt')):
            q, k = taps[2 * l + i]
            assert q.shape == (sum(lens), 256) and q.dtype == torch.float32
            kv_seg = [(c + B) % (2 * B) if kind == 'xatt' else c for c in range(2 * B)]
            w64 = head_mean_weights(q.double(), k.double(), lens, lens, kv_seg, 8, scale, max(lens))
            w32 = head_mean_weights(q, k, lens, lens, kv_seg, 8, scale, max(lens))
            m = valid_mask(lens, lens, kv_seg, max(lens))
            got = torch.zeros_like(w32)
            for c in range(2 * B):
                t = maps[('src_' if c < B else 'tgt_') + kind][l, c % B].cpu()
                got[start[c]:start[c + 1], :t.shape[1]] = t[:lens[c]]
            e = elem_err(got[m], w64[m], floor=1e-3)
            e32 = elem_err(w32[m], w64[m], floor=1e-3)
            print(f'attention-maps d256 layer {l} {kind}: kernel {e:.3e} fp32-restatement {e32:.3e}')
            assert e <= max(4 * e32, 1e-6), (l, kind, e, e32)
            assert not bool(got[~m].any())


def test_get_attentions_needs_a_recording_forward(gpu):
    import fgreg
    model, src, tgt = _fixture_model('attn_modelnet_small', gpu)
    enc = model.transformer_encoder
    assert enc.record_attention is False
    assert all(l.satt_weights is None and l.xatt_weights is None for l in enc.layers)
    model(_batch(src, tgt, gpu))                               # a plain forward records nothing
    with pytest.raises(RuntimeError, match='no attention maps recorded: set record_attention = '
                                           'True and run a forward'):
        enc.get_attentions()
    enc.record_attention = True
    with pytest.raises(NotImplementedError):
        next(fgreg.pipeline(model, [_batch(src, tgt, gpu)]))
    model.train()
    with pytest.raises(NotImplementedError):
        model(_batch(src, tgt, gpu))
    model.eval()
    model(_batch(src, tgt, gpu))
    (a, _), _ = enc.get_attentions()
    assert a.shape[0] == len(enc.layers) and a.is_cuda


def test_dropin_returns_the_same_maps(gpu):
    """model.transformer_encoder.get_attentions() through the package's finegrained_regtr.RegTR
    (it inherits the forward): bit-equal to fgreg.RegTR's on the same weights and inputs."""
    from test_gpu_dropin import _load_dropin
    mod = _load_dropin()
    outs = []
    for cls in (None, mod.RegTR):
        model, src, tgt = _fixture_model('attn_modelnet_small', gpu, cls)
        model.transformer_encoder.record_attention = True
        with torch.no_grad():
            model(_batch(src, tgt, gpu))
        outs.append(_named(model.transformer_encoder.get_attentions()))
    for nm in MAPS:
        assert torch.equal(outs[0][nm], outs[1][nm]), nm
