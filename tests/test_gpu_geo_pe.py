"""RegTR with ``pos_emb_type: geometric`` on the GPU: the reference's forward fixture, HIP-graph
replay and weight-update invalidation on a full-width model, the bf16 mode (the embedding stays
f16x3), fgreg.pipeline, the reference's training step (gradients of proj_d / proj_a included), a
module-level gradient test against fp64, the CorrespondenceDecoder head, and the refusals."""
import numpy as np
import pytest
import torch

import _geo_ref as gr
from conftest import forward_fixture, golden, is_trainable, loss_fixture, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4                 # test_gpu_learned_pe.py's
GRAD_TOL = 1e-2            # test_gpu_train.py's (see its module docstring)
KEYS = ['src_feat_un', 'tgt_feat_un', 'src_feat', 'tgt_feat', 'src_kp', 'tgt_kp',
        'src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap']
PE_KEYS = [f'pos_embed.proj_{p}.{t}' for p in 'da' for t in ('weight', 'bias')]


def _batch(src, tgt, dev):
    return {'src_xyz': [torch.from_numpy(np.asarray(s)).to(dev) for s in src],
            'tgt_xyz': [torch.from_numpy(np.asarray(t)).to(dev) for t in tgt]}


def test_forward_on_reference_meta(gpu):
    """forward_modelnet_geo_pe.npz: the reference RegTR with its structure embedding switched on
    (sigma_d 0.05, stored as geo_sigma_d), d_embed 32: the composed path."""
    import fgreg
    from fgreg.transformer import GeometricStructureEmbedding
    cfg, sd, src, tgt, meta, d = forward_fixture('forward_modelnet_geo_pe')
    assert cfg.pos_emb_type == 'geometric' and cfg.geo_sigma_d == float(d['geo_sigma_d']) == 0.05
    model = fgreg.RegTR(cfg)
    assert isinstance(model.pos_embed, GeometricStructureEmbedding)
    assert model.pos_embed.sigma_d == 0.05 and model.pos_embed.angle_k == 3
    assert torch.allclose(model.pos_embed.embedding.div_term, sd['pos_embed.embedding.div_term'],
                          rtol=1e-6, atol=0)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith('feature_criterion') for k in missing)
    model = model.to(gpu).eval()
    model.preprocessor = fgreg.FixedMetaPreprocessor(
        {k: [t.to(gpu) for t in v] for k, v in meta.items()})
    out = model(_batch(src, tgt, gpu))
    for k in KEYS:
        for b in range(len(src)):
            assert rel_err(out[k][b], d[f'out.{k}.{b}']) < TOL, (k, b)
    assert np.abs(out['pose'].cpu().numpy() - d['out.pose']).max() < TOL


def _random_model(cfg, seed):
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
    return m.eval()


def _same(a, b):
    for k in KEYS:
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x, y), k
    assert torch.equal(a['pose'], b['pose'])


def _eager(model, batch):
    import fgreg.regtr as rt
    old = rt.GRAPHS
    rt.GRAPHS = False
    try:
        return model(batch)
    finally:
        rt.GRAPHS = old


GEO = dict(pos_emb_type='geometric', geo_sigma_d=0.05)


def test_full_width_graph_update_and_bf16(gpu):
    """The ModelNet config (d_embed 256: the fused launch) with the structure embedding, B = 2:
    graph replay equals the eager forward bit for bit, a weight update leaves no stale image or
    graph, the bf16 mode runs and the embedding itself is unchanged by the mode."""
    import fgreg.config as fc
    import fgreg.regtr as rt
    from fgreg import linear as lin
    from fgreg import ops
    from fgreg.synthetic import make_batch
    model = _random_model(fc.get('modelnet', **GEO), 5).to(gpu)
    src, tgt, _ = make_batch('modelnet', 2)
    old = rt.GRAPHS
    try:
        e1 = _eager(model, _batch(src, tgt, gpu))
        rt.GRAPHS = True
        model(_batch(src, tgt, gpu))
        model(_batch(src, tgt, gpu))                  # second sighting: captured
        assert len(rt._GRAPHS[model]['graphs']) == 1
        g1 = model(_batch(src, tgt, gpu))             # third call: replay
        _same(g1, e1)
        lens = [t.shape[0] for t in g1['src_kp'] + g1['tgt_kp']]
        assert ops.geo_embed_supported(sum(lens), 256, 3)
        with torch.no_grad():
            model.pos_embed.proj_a.weight.mul_(1.5)
            model.pos_embed.proj_d.bias.add_(0.1)
        g2 = model(_batch(src, tgt, gpu))
        assert not torch.equal(g2['src_feat'][0], g1['src_feat'][0])
        fresh = _random_model(fc.get('modelnet', **GEO), 5)
        fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
        _same(g2, _eager(fresh.to(gpu), _batch(src, tgt, gpu)))
    finally:
        rt.GRAPHS = old
    xyz = torch.cat(g1['src_kp'] + g1['tgt_kp']).contiguous()
    off = ops.offsets(lens, gpu)
    with torch.no_grad():
        pe = model.pos_embed(xyz, off, lens)
        with lin.mode_scope('bf16'):
            out16 = model(_batch(src, tgt, gpu))
            pe16 = model.pos_embed(xyz, off, lens)
        composed = model.pos_embed.forward_composed(xyz, off, lens)
    assert torch.equal(pe, pe16)
    assert rel_err(pe, composed) < 4e-6
    assert all(bool(torch.isfinite(t).all()) for t in out16['src_feat'])
    # and it is the definition: fp64 on the kernel's own neighbours
    nn = ops.geo_embed_indices(xyz, off, 3, 0.05, 15)[0].cpu().numpy()
    m = model.pos_embed
    ref = gr.forward(xyz.cpu().numpy(), lens, 3, 0.05, 15, m.embedding.div_term.cpu().double(),
                     m.proj_d.weight.detach().cpu(), m.proj_d.bias.detach().cpu(),
                     m.proj_a.weight.detach().cpu(), m.proj_a.bias.detach().cpu(), 'max', nn=nn)
    assert rel_err(pe, ref) < 1e-5


def test_pipeline_equals_sequential_cold_model(gpu):
    import fgreg
    from fgreg.synthetic import make_batch
    torch.manual_seed(3)
    np.random.seed(3)
    model = fgreg.RegTR(fgreg.config.get('modelnet', **GEO)).to(gpu).eval()
    batches = []
    for start in (0, 4, 0):
        src, tgt, _ = make_batch('modelnet', 2, start=start)
        batches.append(_batch(src, tgt, gpu))
    got = list(fgreg.pipeline(model, [dict(b) for b in batches], depth=2, streams=2))
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = [model(dict(b)) for b in batches]
    assert len(got) == 3
    for a, r in zip(got, ref):
        _same(a, r)


def test_decoder_head_and_refusals(gpu):
    """The CorrespondenceDecoder head without positional embedding works (forward finite, equal
    under graph replay); with corr_decoder_has_pos_emb it is refused at construction; an n <= k
    cloud is a ValueError; a sine model still constructs."""
    import fgreg
    import fgreg.config as fc
    from fgreg.synthetic import make_batch
    from fgreg.transformer import PositionEmbeddingCoordsSine
    with pytest.raises(NotImplementedError, match='corr_decoder_has_pos_emb'):
        fgreg.RegTR(fc.get('modelnet', direct_regress_coor=False, **GEO))
    with pytest.raises(ValueError, match='Unsupported reduction mode'):
        fgreg.RegTR(fc.get('modelnet', geo_reduction_a='median', **GEO))
    assert isinstance(fgreg.RegTR(fc.get('modelnet')).pos_embed, PositionEmbeddingCoordsSine)
    m = fgreg.RegTR(fc.get('modelnet', geo_angle_k=4, geo_sigma_a=10, geo_reduction_a='mean', **GEO))
    pe = m.pos_embed
    assert (pe.angle_k, pe.sigma_a, pe.reduction_a, pe.sigma_d) == (4, 10, 'mean', 0.05)
    model = _random_model(fc.get('modelnet', direct_regress_coor=False,
                                 corr_decoder_has_pos_emb=False, **GEO), 2).to(gpu)
    src, tgt, _ = make_batch('modelnet', 1)
    e = _eager(model, _batch(src, tgt, gpu))
    assert all(bool(torch.isfinite(t).all()) for t in e['src_kp_warped'] + e['src_feat'])
    model(_batch(src, tgt, gpu))
    _same(model(_batch(src, tgt, gpu)), e)
    # a coarse cloud of <= k points: ValueError from the host lengths
    from fgreg.transformer import Segments
    xyz = torch.rand(3 + 40, 3, device=gpu)
    seg = Segments([3, 40], gpu)
    with pytest.raises(ValueError):
        model.pos_embed(xyz, seg.cloud_off, seg.lengths)


def test_train_step_vs_reference(gpu):
    """The reference's train() step on the geometric-PE model (train_modelnet_geo_pe.npz) vs
    fgreg's: losses within 1e-5, every gradient norm and every stored full gradient within
    GRAD_TOL, and the four gradients of proj_d / proj_a present and non-zero."""
    import fgreg
    import loss_oracle as lo
    cfg, sd, src, tgt, meta, _ = forward_fixture('forward_modelnet_geo_pe')
    _, _, batch, _, _, _, W, W_un = loss_fixture()
    ref = golden('train_modelnet_geo_pe')
    model = fgreg.RegTR(cfg)
    model.load_state_dict(sd, strict=False)
    model = model.to(gpu).train()
    model.preprocessor = fgreg.FixedMetaPreprocessor({k: [t.to(gpu) for t in v]
                                                      for k, v in meta.items()})
    pred = model(_batch(src, tgt, gpu))
    host = {k: ([t.cpu().double() for t in v] if isinstance(v, list) else v.cpu().double())
            for k, v in pred.items()}
    Wg = W.detach().cpu().double().requires_grad_(True)
    Wug = W_un.detach().cpu().double().requires_grad_(True)
    cv = lambda t: t.cpu().double() if t.is_floating_point() else t.cpu()      # noqa: E731
    b = {'pose': cv(batch['pose']),
         'kpconv_meta': {k: [cv(t) for t in v] for k, v in batch['kpconv_meta'].items()},
         'src_overlap': [cv(t) for t in batch['src_overlap']],
         'tgt_overlap': [cv(t) for t in batch['tgt_overlap']]}
    losses, _ = lo.compute_loss(cfg, Wg, Wug, host, b)
    losses['total'].backward()
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    grads['feature_criterion.W'] = Wg.grad
    grads['feature_criterion_un.W'] = Wug.grad
    for k in ref.files:
        if k.startswith('loss.'):
            v = float(ref[k])
            assert abs(float(losses[k[5:]]) - v) <= 1e-5 * max(1.0, abs(v)), (k, float(losses[k[5:]]), v)
    for k in PE_KEYS:
        assert grads.get(k) is not None, k
        assert float(grads[k].abs().max()) > 0.0, k
        assert 'grad.' + k in ref.files
    norms = {k[6:] for k in ref.files if k.startswith('gnorm.')}
    assert norms == {k for k in grads if is_trainable(k)}, norms ^ set(grads)
    nerr = {}
    for k in sorted(norms):
        n_ref = float(ref['gnorm.' + k])
        nerr[k] = abs(float(grads[k].double().norm()) - n_ref) / max(n_ref, 1e-12)
    ferr = {}
    for k in ref.files:
        if k.startswith('grad.'):
            a, r = grads[k[5:]].detach().double().cpu(), torch.from_numpy(ref[k]).double()
            ferr[k[5:]] = float((a - r).norm() / max(float(r.norm()), 1e-30))
    print('\nworst gradient-norm errors', sorted(((v, k) for k, v in nerr.items()), reverse=True)[:5],
          '\nfull-gradient Frobenius errors', {k[-40:]: f'{v:.1e}' for k, v in ferr.items()})
    for k, e in nerr.items():
        assert e < GRAD_TOL, (k, e)
    for k, e in ferr.items():
        assert e < GRAD_TOL, (k, e)


@pytest.mark.parametrize('reduction', ['max', 'mean'])
def test_module_gradients_vs_fp64(gpu, reduction):
    """train_forward on clouds [4, 65]: the gradients of proj_d / proj_a under a fixed random
    cotangent against an fp64 torch restatement on the kernel's own neighbours.

    The embedding is a maximum of candidates, and among 69 x 256 outputs some have two candidates
    closer than any fp32 evaluation can tell apart (smallest fp64 gap here ~3e-8); there the
    derivative is not defined and either routing is a valid sub-gradient. The cotangent is
    therefore zero on the outputs whose fp64 gap is below 1e-5 (5 x the forward's 2e-6 absolute
    error at |out| <= 2), and at most 5 % of the outputs may be such. Everywhere else both sides
    route through the same rows, and what remains is: d / a from the fp32 indices kernel (within
    1e-5 absolute, test_gpu_geo_embed.py; dE/dt <= 1), fp32 sin / cos, and the f16x3
    weight-gradient products over 69 * 12 rows (~2e-6): 2e-5 relative Frobenius."""
    from fgreg import ops
    from fgreg.transformer import GeometricStructureEmbedding
    lengths, k = [4, 65], 3
    rng = np.random.default_rng(4)
    x = rng.uniform(-1.0, 1.0, (sum(lengths), 3)).astype(np.float32)
    torch.manual_seed(4)
    m = GeometricStructureEmbedding(256, angle_k=k, reduction_a=reduction).to(gpu).train()
    X = torch.from_numpy(x).to(gpu)
    off = ops.offsets(lengths, gpu)
    out = m.train_forward(X, off, lengths)
    nn = ops.geo_embed_indices(X, off, k, m.sigma_d, m.sigma_a)[0].cpu().numpy()
    ps = [p.detach().cpu().double().requires_grad_(True)
          for p in (m.proj_d.weight, m.proj_d.bias, m.proj_a.weight, m.proj_a.bias)]
    w = m.embedding.div_term.cpu().double()
    d64, a64 = gr.indices(x, nn, m.sigma_d, m.sigma_a)
    ref = gr.embed(d64, a64, w, *ps, reduction)
    assert rel_err(out, ref) < 1e-5
    with torch.no_grad():
        clear = gr.max_gaps(d64, a64, w, *ps, reduction) >= 1e-5
    print(f'{reduction}: {int((~clear).sum())} of {clear.numel()} outputs at a tie')
    assert float((~clear).double().mean()) <= 0.05
    cot = torch.from_numpy(rng.standard_normal(tuple(out.shape))).double() * clear
    (out * cot.float().to(gpu)).sum().backward()
    (ref * cot.float().double()).sum().backward()
    for p, q, name in zip((m.proj_d.weight, m.proj_d.bias, m.proj_a.weight, m.proj_a.bias), ps,
                          PE_KEYS):
        e = float((p.grad.cpu().double() - q.grad).norm() / q.grad.norm())
        print(f'{reduction} {name}: {e:.3g}')
        assert e < 2e-5, (name, e)
