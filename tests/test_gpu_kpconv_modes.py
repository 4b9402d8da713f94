"""KP_influence gaussian / constant and aggregation_mode closest on the GPU: every forward
gather family (c1, narrow, quad-lane, wide) and the backward's scatter for the five new
(influence, aggregation) pairs against the fp64 restatement of finegrained_kpconv_blocks.py:
296-381 (tests/_kpconv_modes.py, which also states the rule for near-ties of ``closest``),
in a guarded arena, and the reference's own fixtures (tests/golden/make_golden_kpconv_modes.py).

Forward bound (test_gpu_dispatch's): the conditioned error max |wf - ref| / sum_h w_h |x_h| is
at most 4 x the torch fp32 restatement's own error + 1e-7 and never above 1e-4; nnorm is exact.
Both errors are printed before the assertion.
"""
import math

import numpy as np
import pytest
import torch

import _kpconv_modes as km
from _arena import SENTINEL, Arena, assert_both_equal, run_both
from conftest import forward_fixture, golden, is_trainable, loss_fixture, rel_err

pytestmark = pytest.mark.gpu
F32 = torch.float32
CAP, TOL, GRAD_TOL = 1e-4, 1e-4, 1e-2        # test_gpu_dispatch's, test_gpu_forward's, test_gpu_train's
EXT = km.EXT
CODES = {'linear': 0, 'gaussian': 1, 'constant': 2, 'sum': 0, 'closest': 1}
KEYS = ['src_feat_un', 'tgt_feat_un', 'src_feat', 'tgt_feat', 'src_kp', 'tgt_kp',
        'src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap']
# n_kp 15 at every width and both row lengths (H 7: the wide / quad-lane pad rows are live;
# H 70: a second 64-wide chunk); n_kp 17 / 32 (the 32-kernel-point instances) at cin 1, 64, 256
SHAPES = [(cin, H, 15) for cin in (1, 3, 12, 16, 32, 48, 64, 128, 256) for H in (7, 70)] + \
         [(1, 7, 17), (1, 70, 32), (64, 70, 17), (64, 7, 32), (256, 7, 17), (256, 70, 32)]


def _L():
    from fgreg import _lib
    return _lib.load()


def _ok(rc, name):
    from fgreg import _lib
    _lib.check(rc, name)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _hold(what, e, e32):
    print(f'kpconv-modes-error {what}: kernel {e:.3e} fp32-restatement {e32:.3e}')
    assert e <= min(4 * e32 + 1e-7, CAP), (what, e, e32)


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('influence,aggregation', km.NEW_COMBOS)
@pytest.mark.parametrize('cin,H,n_kp', SHAPES)
def test_gather_modes_vs_fp64(gpu, cin, H, n_kp, influence, aggregation):
    import fgreg.ops as ops
    q, s, idx, x, kp, cnt = km.table(cin, H, n_kp)
    ref, den, e32 = km.reference(cin, H, n_kp, influence, aggregation)
    wf, nn_ = ops.kpconv_gather(q.to(gpu), s.to(gpu), idx.to(gpu), x.to(gpu), kp.to(gpu), EXT,
                                influence, aggregation)
    _hold(f'{influence}/{aggregation} cin {cin} n_kp {n_kp} H {H}', km.cond_err(wf, ref, den), e32)
    assert torch.equal(nn_.cpu(), cnt)
    assert bool((wf[3] == 0).all()) and float(nn_[3]) == 1.0          # the all-shadow row


def _gather_abi(ar, data, cin, n_kp, H, inf, agg, old=False):
    q, s, idx, x, kp = data[:5]
    nq, ns = q.shape[0], s.shape[0]
    wf = ar.matrix(nq, n_kp * cin, n_kp * cin, F32, 'out', name='wf')
    nn_ = ar.vector(nq, F32, 'out', name='nnorm')
    a = (_p(ar.put(q, name='q')), _p(ar.put(s, name='s')), nq, ns,
         _p(ar.put(idx, name='idx')) if H else None, H, _p(ar.put(x, name='x')), cin,
         _p(ar.put(kp, name='kp')), n_kp, EXT)
    tail = (_p(wf), _p(nn_), None, 0, _st())
    rc = _L().fgr_kpconv_gather(*a, *tail) if old else _L().fgr_kpconv_gather_mode(*a, inf, agg, *tail)
    return rc, wf, nn_


@pytest.mark.parametrize('influence,aggregation', km.NEW_COMBOS)
@pytest.mark.parametrize('cin', [1, 12, 16, 64])
def test_gather_modes_width_zero(gpu, cin, influence, aggregation):
    """An empty neighbour table (width 0, idx NULL): wf all zeros and nnorm all ones from the
    stem, narrow, quad-lane and wide kernels in every mode (constant included)."""
    q, s, idx, x, kp, _ = km.table(cin, 7, 15)
    ar = Arena(gpu)
    rc, wf, nn_ = _gather_abi(ar, (q, s, idx, x, kp), cin, 15, 0, CODES[influence], CODES[aggregation])
    _ok(rc, 'fgr_kpconv_gather_mode')
    torch.cuda.synchronize()
    ar.check()
    assert bool((wf == 0).all()) and bool((nn_ == 1).all())


@pytest.mark.parametrize('cin', [1, 12, 16, 64])
def test_old_entry_point_is_mode_0_0(gpu, cin):
    """fgr_kpconv_gather and fgr_kpconv_gather_mode(.., 0, 0): bit-equal wf and nnorm, one case
    per kernel family."""
    data = km.table(cin, 70, 15)
    got = []
    for old in (True, False):
        ar = Arena(gpu)
        rc, wf, nn_ = _gather_abi(ar, data, cin, 15, 70, 0, 0, old=old)
        _ok(rc, 'fgr_kpconv_gather')
        torch.cuda.synchronize()
        ar.check()
        got.append((wf.clone(), nn_.clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


# ---------------------------------------------------------------------------------------------
# guarded arena
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cin,H,influence,aggregation', [(1, 70, 'gaussian', 'closest'),
                                                         (12, 7, 'constant', 'closest'),
                                                         (16, 7, 'constant', 'sum'),
                                                         (32, 70, 'linear', 'closest'),
                                                         (64, 7, 'constant', 'sum'),
                                                         (128, 70, 'gaussian', 'closest')])
def test_gather_modes_footprint(gpu, cin, H, influence, aggregation):
    """One new-mode case per family through ctypes: exact bytes (every wf / nnorm element
    written, nothing outside them), clean run equal to the poisoned run, and the bound. The
    H 7 / constant cases are the pad-row trap: a pad row whose weight came from the influence
    function would add x[0] to every kernel point's sum."""
    data = km.table(cin, H, 15)
    ref, den, e32 = km.reference(cin, H, 15, influence, aggregation)

    def fn(ar):
        rc, wf, nn_ = _gather_abi(ar, data, cin, 15, H, CODES[influence], CODES[aggregation])
        _ok(rc, 'fgr_kpconv_gather_mode')
        return wf, nn_
    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    _hold(f'arena {influence}/{aggregation} cin {cin} H {H}',
          km.cond_err(clean[0].reshape(ref.shape), ref, den), e32)
    assert torch.equal(clean[1].cpu(), data[5])


def _scatter_abi(ar, data, dwf, cin, n_kp, H, inf, agg):
    from fgreg import _lib
    from fgreg.autograd import nbr_inverse
    q, s, idx, x, kp = data[:5]
    nq, ns = q.shape[0], s.shape[0]
    start, pos, _ = nbr_inverse(idx.to(ar.device), ns)
    nb = _lib.ws_size('fgr_kpconv_scatter_workspace', nq, H, cin)
    dx = ar.matrix(ns, cin, cin, F32, 'out', name='dx')
    ws = ar.bytes(nb, name='ws')
    rc = _L().fgr_kpconv_scatter_mode(
        _p(ar.put(q, name='q')), _p(ar.put(s, name='s')), nq, ns, _p(ar.put(idx, name='idx')), H,
        _p(ar.put(dwf, name='dwf')), cin, _p(ar.put(kp, name='kp')), n_kp, EXT, inf, agg,
        _p(ar.put(start.cpu(), name='start')), _p(ar.put(pos.cpu().reshape(nq, H), name='pos')),
        _p(dx), _p(ws), nb, _st())
    return rc, dx


def test_scatter_modes_footprint(gpu):
    """fgr_kpconv_scatter_mode (gaussian / closest, cin 12) through ctypes with the exact
    workspace of fgr_kpconv_scatter_workspace: exact bytes, clean = poisoned, and dx equal to
    the fp64 autograd of the restatement within test_kpconv_backward's 1e-5."""
    cin, H, n_kp = 12, 70, 15
    data = km.table(cin, H, n_kp)
    q, s, idx, x, kp, _ = data
    dwf = torch.randn(q.shape[0], n_kp * cin, generator=torch.Generator().manual_seed(5))
    x64 = x.double().requires_grad_(True)
    wf64, _ = km.gather_ref(q, s, idx, x64, kp, EXT, 'gaussian', 'closest', torch.float64)
    (wf64.reshape(dwf.shape) * dwf.double()).sum().backward()

    def fn(ar):
        rc, dx = _scatter_abi(ar, data, dwf, cin, n_kp, H, 1, 1)
        _ok(rc, 'fgr_kpconv_scatter_mode')
        return dx
    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    assert rel_err(clean, x64.grad) < 1e-5, rel_err(clean, x64.grad)


@pytest.mark.parametrize('inf,agg', [(7, 0), (0, 2), (-1, 1)])
def test_unknown_mode_is_refused_before_any_launch(gpu, inf, agg):
    """FGR_E_ARG, the value named in fgr_last_error, and every sentinel of wf, nnorm, dx and the
    workspace intact."""
    data = km.table(16, 7, 15)
    ar = Arena(gpu)
    rc, _, _ = _gather_abi(ar, data, 16, 15, 7, inf, agg)
    assert rc == -1
    msg = _L().fgr_last_error().decode()
    assert 'fgr_kpconv_gather_mode' in msg and f'influence {inf}' in msg and f'aggregation {agg}' in msg
    dwf = torch.zeros(70, 15 * 16)
    rc, _ = _scatter_abi(ar, data, dwf, 16, 15, 7, inf, agg)
    assert rc == -1 and 'fgr_kpconv_scatter_mode' in _L().fgr_last_error().decode()
    torch.cuda.synchronize()
    for r in ar.regions:
        if r.role == 'out':
            assert bool((r.buf.view(torch.int32) == SENTINEL).all()), r.name
        elif r.role == 'scratch':
            assert bool((r.view == 0).all()), r.name


# ---------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('influence,aggregation', km.NEW_COMBOS)
@pytest.mark.parametrize('cin', [1, 12, 16, 64, 128])
def test_kpconv_modes_backward(gpu, cin, influence, aggregation):
    """kpconv_t (gather + weight GEMM; dx through fgr_kpconv_scatter_mode, dW through the
    regathered wf) vs fp64 autograd of the restatement on the tie-edited table:
    test_gpu_train.test_kpconv_backward's bound."""
    from fgreg.autograd import kpconv_t
    q, s, idx, x0, kp, _ = km.table(cin, 70, 15)
    g = torch.Generator().manual_seed(cin)
    W0 = torch.randn(15, cin, 24, generator=g) / math.sqrt(15 * cin)

    class Conv:
        pass
    conv = Conv()
    x, W = (t.clone().to(gpu).requires_grad_(True) for t in (x0, W0))
    x64, W64 = (t.double().requires_grad_(True) for t in (x0, W0))
    conv.weights, conv.kernel_points, conv.KP_extent = W, kp.to(gpu), EXT
    conv.KP_influence, conv.aggregation_mode = influence, aggregation
    out, nnorm = kpconv_t(conv, q.to(gpu), s.to(gpu), idx.to(gpu), x)
    y = out / nnorm.unsqueeze(1)
    y64 = km.kpconv_ref(q.double(), s.double(), idx, x64, W64, kp.double(), EXT, influence, aggregation)
    R = torch.randn(y64.shape, generator=torch.Generator().manual_seed(3))
    (y * R.to(gpu)).sum().backward()
    (y64 * R.double()).sum().backward()
    errs = rel_err(y, y64), rel_err(x.grad, x64.grad), rel_err(W.grad, W64.grad)
    print(f'kpconv-modes-backward {influence}/{aggregation} cin {cin}: y {errs[0]:.2e} dx {errs[1]:.2e} dW {errs[2]:.2e}')
    assert max(errs) < 1e-5, errs


# ---------------------------------------------------------------------------------------------
# the reference's fixtures
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('influence,aggregation', km.NEW_COMBOS)
def test_kpconv_module_vs_reference(gpu, influence, aggregation):
    """fgreg.backbone.KPConv against the reference's KPConv module (kpconv_modes.npz), within the
    forward tests' 1e-4."""
    from fgreg.backbone import KPConv
    d = golden('kpconv_modes')
    T = lambda k: torch.from_numpy(d[k])
    kp, W = T('kp'), T(f'W.{influence}.{aggregation}')
    conv = KPConv(kp.shape[0], 3, W.shape[1], W.shape[2], KP_extent=float(d['extent']),
                  radius=float(d['radius']), KP_influence=influence, aggregation_mode=aggregation)
    with torch.no_grad():
        conv.weights.copy_(W)
        conv.kernel_points.copy_(kp)
    conv = conv.to(gpu)
    with torch.no_grad():
        out = conv(T('q').to(gpu), T('s').to(gpu), T('idx').long().to(gpu), T('x').to(gpu))
    e = rel_err(out, d[f'out.{influence}.{aggregation}'])
    print(f'kpconv module {influence}/{aggregation}: rel_err {e:.3g}')
    assert e < TOL, e


def _batch(src, tgt, dev):
    return {'src_xyz': [torch.from_numpy(np.asarray(s)).to(dev) for s in src],
            'tgt_xyz': [torch.from_numpy(np.asarray(t)).to(dev) for t in tgt]}


def _fixture_model(name, gpu, **over):
    import ast
    import fgreg
    import fgreg.config as fc
    from fgreg.backbone import KPConv
    cfg, sd, src, tgt, meta, d = forward_fixture(name)
    if over:
        cfg = fc.get('modelnet', **dict(ast.literal_eval(str(d['cfg_overrides'])), **over))
    model = fgreg.RegTR(cfg)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith('feature_criterion') for k in missing)
    model = model.to(gpu).eval()
    model.preprocessor = fgreg.FixedMetaPreprocessor(
        {k: [t.to(gpu) for t in v] for k, v in meta.items()})
    convs = [m for m in model.modules() if isinstance(m, KPConv)]
    assert all((c.KP_influence, c.aggregation_mode) == (cfg.KP_influence, cfg.aggregation_mode)
               for c in convs)
    return model, src, tgt, d


@pytest.mark.parametrize('name', ['forward_modelnet_kp_gaussian', 'forward_modelnet_kp_closest'])
def test_forward_on_reference_meta(gpu, name):
    """Three calls in a row: eager, the capturing second sighting, a graph replay."""
    model, src, tgt, d = _fixture_model(name, gpu)
    for call in range(3):
        out = model(_batch(src, tgt, gpu))
        for k in KEYS:
            for b in range(len(src)):
                e = rel_err(out[k][b], d[f'out.{k}.{b}'])
                assert e < TOL, (call, k, b, e)
        pose = float(np.abs(out['pose'].cpu().numpy() - d['out.pose']).max())
        assert pose < TOL, (call, pose)


@pytest.mark.parametrize('name,over', [('forward_modelnet_kp_gaussian', dict(KP_influence='linear')),
                                       ('forward_modelnet_kp_closest', dict(aggregation_mode='sum'))])
def test_default_modes_fail_the_fixtures(gpu, name, over):
    """The options are not ignored: the same weights with linear / sum miss the bound."""
    model, src, tgt, d = _fixture_model(name, gpu, **over)
    out = model(_batch(src, tgt, gpu))
    assert min(rel_err(out['src_feat'][b], d[f'out.src_feat.{b}']) for b in range(len(src))) > TOL


def _train_step(gpu):
    """fgreg's training step on the gaussian-influence model and the loss inputs of
    loss_modelnet_small -> (losses, {parameter: gradient}, the reference's npz)."""
    import fgreg
    import loss_oracle as lo
    import ast
    from named_weights import named_state_dict
    cfg, _, src, tgt, meta, fwd = forward_fixture('forward_modelnet_kp_gaussian')
    _, _, batch, _, _, _, W, W_un = loss_fixture()
    ref = golden('train_modelnet_kp_gaussian')
    # the weights of the fixture's own seed (the generator's rule), rebuilt from (key, shape, seed)
    raw = fwd['sd_keys'].item()
    keys = ast.literal_eval(raw.decode() if isinstance(raw, bytes) else str(raw))
    stored = {k[3:]: ref[k] for k in ref.files if k.startswith('sd.')}
    assert len(stored) >= 5 and all('kernel_points' in k for k in stored)
    sd = {k: torch.from_numpy(np.array(v)) for k, v in
          named_state_dict(keys, int(ref['sd_seed']), float(fwd['bias']), stored).items()}
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
    return {k: float(v.detach()) for k, v in losses.items()}, grads, ref


def _check_train_step(losses, grads, ref, pre, what):
    """Losses within 1e-5, every gradient norm and every stored full gradient within GRAD_TOL
    (test_gpu_train.test_train_step_vs_reference's checks) against the entries ``pre`` + ..."""
    n_loss = 0
    for k in ref.files:
        if k.startswith(pre + 'loss.'):
            v, name = float(ref[k]), k[len(pre) + 5:]
            assert abs(losses[name] - v) <= 1e-5 * max(1.0, abs(v)), (k, losses[name], v)
            n_loss += 1
    assert n_loss >= 3
    norms = {k[len(pre) + 6:] for k in ref.files if k.startswith(pre + 'gnorm.')}
    assert norms == {k for k in grads if is_trainable(k)}, norms ^ set(grads)
    nerr = {}
    for k in sorted(norms):
        n_ref = float(ref[pre + 'gnorm.' + k])
        nerr[k] = abs(float(grads[k].double().norm()) - n_ref) / max(n_ref, 1e-12)
    ferr = {}
    for k in ref.files:
        if k.startswith(pre + 'grad.'):
            name = k[len(pre) + 5:]
            a, r = grads[name].detach().double().cpu(), torch.from_numpy(ref[k]).double()
            ferr[name] = float((a - r).norm() / max(float(r.norm()), 1e-30))
    assert len(ferr) >= 1
    print(f'kpconv-modes-train {what}: worst gradient-norm errors',
          sorted(((v, k) for k, v in nerr.items()), reverse=True)[:3],
          'full-gradient Frobenius errors', {k[-40:]: f'{v:.1e}' for k, v in ferr.items()})
    for k, e in nerr.items():
        assert e < GRAD_TOL, ('gnorm', k, e)
    for k, e in ferr.items():
        assert e < GRAD_TOL, ('grad', k, e)


def test_train_step_vs_reference(gpu):
    """The reference's train() step on the gaussian-influence model, make_golden.make_train's
    recipe in fp32 (train_modelnet_kp_gaussian.npz), vs fgreg's: losses within 1e-5, every
    gradient norm and every stored full gradient within test_gpu_train's GRAD_TOL = 1e-2.

    The fixture's weight seed is 1, by the generator's rule (make_golden_kpconv_modes.make_train):
    with seed 0 one activation input of the last encoder block lies 9.4e-7 from its kink, the
    reference's fp32 forward takes another branch there than its own fp64 forward, and its fp32
    encoder gradients are up to 1.2e-2 from its fp64 ones, so no implementation meets 1e-2
    against them except by landing on the same side (measured on an MI355X against that
    fixture: 1.07e-2 in one norm, 1.2e-2 in one full gradient, 5.7e-6 / 3.1e-6 against the fp64
    run). With seed 1 the reference's fp32 step is 2.9e-5 from its fp64 step."""
    losses, grads, ref = _train_step(gpu)
    _check_train_step(losses, grads, ref, '', 'vs the reference in fp32')


def test_train_step_vs_reference_fp64(gpu):
    """The same step against the same recipe run with the reference's modules in fp64 (the
    f64.* entries of the fixture): the same checks and bounds."""
    losses, grads, ref = _train_step(gpu)
    _check_train_step(losses, grads, ref, 'f64.', 'vs the reference in fp64')
