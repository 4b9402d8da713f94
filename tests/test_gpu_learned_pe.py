"""RegTR with ``pos_emb_type: learned`` on the GPU: the reference's forward fixtures (regressor
and CorrespondenceDecoder heads), HIP-graph replay and weight-update invalidation on a
full-width model, the bf16 mode (the MLP stays f16x3), the reference's training step (gradients
of the MLP's ten parameters included) and fgreg.pipeline."""
import numpy as np
import pytest
import torch

from conftest import forward_fixture, golden, is_trainable, loss_fixture, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
GRAD_TOL = 1e-2            # test_gpu_train.py's (see its module docstring)
KEYS = ['src_feat_un', 'tgt_feat_un', 'src_feat', 'tgt_feat', 'src_kp', 'tgt_kp',
        'src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap']
PE_KEYS = [f'pos_embed.mlp.{i}.{t}' for i in (0, 2, 4, 6, 8) for t in ('weight', 'bias')]


def _batch(src, tgt, dev):
    return {'src_xyz': [torch.from_numpy(np.asarray(s)).to(dev) for s in src],
            'tgt_xyz': [torch.from_numpy(np.asarray(t)).to(dev) for t in tgt]}


@pytest.mark.parametrize('name', ['forward_modelnet_learned_pe',
                                  'forward_modelnet_learned_pe_decoder'])
def test_forward_on_reference_meta(gpu, name):
    import fgreg
    cfg, sd, src, tgt, meta, d = forward_fixture(name)
    model = fgreg.RegTR(cfg)
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


def test_full_width_graph_update_and_bf16(gpu):
    """The ModelNet config (d_embed 256: the fused launch) with the learned embedding, B = 2."""
    import fgreg.config as fc
    import fgreg.regtr as rt
    from fgreg import linear as lin
    from fgreg import ops
    from fgreg.synthetic import make_batch
    model = _random_model(fc.get('modelnet', pos_emb_type='learned'), 5).to(gpu)
    src, tgt, _ = make_batch('modelnet', 2)
    n_c = None
    old = rt.GRAPHS
    try:
        e1 = _eager(model, _batch(src, tgt, gpu))
        rt.GRAPHS = True
        model(_batch(src, tgt, gpu))
        model(_batch(src, tgt, gpu))                  # second sighting: captured
        assert len(rt._GRAPHS[model]['graphs']) == 1
        g1 = model(_batch(src, tgt, gpu))             # third call: replay
        _same(g1, e1)
        n_c = sum(t.shape[0] for t in g1['src_kp'] + g1['tgt_kp'])
        assert ops.pos_mlp_supported(n_c, 256)
        # an in-place update of the MLP's last layer: no stale image or graph survives
        with torch.no_grad():
            model.pos_embed.mlp[8].weight.mul_(1.5)
        g2 = model(_batch(src, tgt, gpu))
        assert not torch.equal(g2['src_feat'][0], g1['src_feat'][0])
        fresh = _random_model(fc.get('modelnet', pos_emb_type='learned'), 5)
        fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
        _same(g2, _eager(fresh.to(gpu), _batch(src, tgt, gpu)))
        # and of an earlier layer (layer 0's raw weight is read by the kernel directly)
        with torch.no_grad():
            model.pos_embed.mlp[0].weight.mul_(0.5)
            model.pos_embed.mlp[4].bias.add_(0.1)
        g3 = model(_batch(src, tgt, gpu))
        model(_batch(src, tgt, gpu))
        g3b = model(_batch(src, tgt, gpu))            # recaptured and replayed
        fresh.load_state_dict({k: v for k, v in model.state_dict().items()})
        e3 = _eager(fresh, _batch(src, tgt, gpu))
        _same(g3, e3)
        _same(g3b, e3)
    finally:
        rt.GRAPHS = old
    # bf16 mode: the forward runs and the embedding itself is the f16x3 one, bit for bit
    xyz = torch.cat(g1['src_kp'] + g1['tgt_kp']).contiguous()
    with torch.no_grad():
        pe = model.pos_embed(xyz)
        with lin.mode_scope('bf16'):
            out16 = model(_batch(src, tgt, gpu))
            pe16 = model.pos_embed(xyz)
        chain = model.pos_embed.forward_chain(xyz)
    assert torch.equal(pe, pe16)
    assert rel_err(pe, chain) < 4e-6
    assert all(bool(torch.isfinite(t).all()) for t in out16['src_feat'])


def test_train_step_vs_reference(gpu):
    """The reference's train() step on the learned-PE model (train_modelnet_learned_pe.npz) vs
    fgreg's: losses within 1e-5, every gradient norm and every stored full gradient within
    GRAD_TOL, and all ten gradients of the MLP present and non-zero."""
    import fgreg
    import loss_oracle as lo
    cfg, sd, src, tgt, meta, _ = forward_fixture('forward_modelnet_learned_pe')
    _, _, batch, _, _, _, W, W_un = loss_fixture()
    ref = golden('train_modelnet_learned_pe')
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


def test_pipeline_equals_sequential_cold_model(gpu):
    """fgreg.pipeline over three batches on two core streams equals model(batch), starting
    from a model whose weight images do not exist yet."""
    import fgreg
    from fgreg.synthetic import make_batch
    torch.manual_seed(3)
    np.random.seed(3)
    model = fgreg.RegTR(fgreg.config.get('modelnet', pos_emb_type='learned')).to(gpu).eval()
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
