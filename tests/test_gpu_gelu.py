"""``transformer_act: gelu`` on the GPU: the elementwise kernels (fgr_gelu_fwd / fgr_gelu_bwd)
against fp64 beside torch's own fp32 F.gelu, in a guarded arena; the fused feed-forward launch
with GELU (fgr_ffn_f16x3_act) against fp64, against the three launches it replaces, its refusals
and the layer's dispatch; the reference's forward fixtures (pre- and post-norm, eager and graph
replay, fgreg.pipeline, the bf16 mode) and the reference's training step."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _arena import assert_both_equal, run_both
from conftest import forward_fixture, golden, is_trainable, loss_fixture, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4                 # test_gpu_forward.py's / test_gpu_learned_pe.py's
GRAD_TOL = 1e-2            # test_gpu_train.py's (see its module docstring)
BF16_FEAT_TOL, BF16_ROT_DEG, BF16_TRANS = 5e-2, 5.0, 0.02       # test_gpu_bf16.py's
KEYS = ['src_feat_un', 'tgt_feat_un', 'src_feat', 'tgt_feat', 'src_kp', 'tgt_kp',
        'src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap']
F32 = torch.float32
ACT_LEAKY, ACT_RELU, ACT_GELU = 1, 2, 4
FIXED = [0.0, 0.7517916, -0.7517916, 1e-30, -1e-30, 6.0, -6.0, 30.0, -30.0, -1e4, 1e4]
SIZES = [1, 3, 4, 5, 1023, 262145]


def _L():
    from fgreg import _lib
    return _lib.load()


def _ok(rc, name):
    from fgreg import _lib
    _lib.check(rc, name)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _both(fn, gpu):
    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    return clean


def _z(n, fixed):
    z = 3.0 * torch.randn(n, generator=torch.Generator().manual_seed(n))
    return torch.cat([z, torch.tensor(FIXED, dtype=F32)]) if fixed else z


# ---------------------------------------------------------------------------------------------
# the elementwise kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fixed', [False, True])
@pytest.mark.parametrize('n', SIZES)
def test_gelu_fwd_bwd_vs_fp64(gpu, n, fixed):
    """n values from N(0, 3^2) alone (the kernel's vector body / n % 4 tail at exactly n), and
    with the fixed values appended (both tails, the erf kink 0.7517916 * sqrt 2 ~ 1, denormal-
    range and huge arguments): error against fp64 within 4 x torch's own fp32 F.gelu / autograd
    error + 1e-7, outputs finite, exact 0 at -30 and exact z at +30, out of place and in place,
    in a guarded arena (exact bytes, guards untouched, clean = poisoned).

    Measured at n = 262145 (random values alone; normwise, max |ref| 13.8 forward, 4.72
    backward): forward 3.25e-8 against torch's 3.25e-8, backward 8.7e-8 against torch's 8.7e-8."""
    z = _z(n, fixed)
    nn_ = z.numel()
    dy = torch.randn(nn_, generator=torch.Generator().manual_seed(n + 1))
    zd = z.double().requires_grad_(True)
    ref = F.gelu(zd)
    ref.backward(dy.double())
    ref, dref = ref.detach(), zd.grad
    # torch fp32 on the same device (the comparison baseline only)
    zt = z.to(gpu).requires_grad_(True)
    yt = F.gelu(zt)
    yt.backward(dy.to(gpu))
    e_t, eb_t = rel_err(yt, ref), rel_err(zt.grad, dref)

    def fwd(ar):
        y = ar.vector(nn_, F32, 'out', name='y')
        _ok(_L().fgr_gelu_fwd(ar.put(z, name='z').data_ptr(), y.data_ptr(), nn_, _st()), 'fgr_gelu_fwd')
        return y

    def fwd_inplace(ar):
        y = ar.vector(nn_, F32, 'out', name='zy')
        y.copy_(z)
        _ok(_L().fgr_gelu_fwd(y.data_ptr(), y.data_ptr(), nn_, _st()), 'fgr_gelu_fwd')
        return y

    def bwd(ar):
        dz = ar.vector(nn_, F32, 'out', name='dz')
        _ok(_L().fgr_gelu_bwd(ar.put(z, name='z').data_ptr(), ar.put(dy, name='dy').data_ptr(),
                              dz.data_ptr(), nn_, _st()), 'fgr_gelu_bwd')
        return dz

    def bwd_inplace(ar):
        dz = ar.vector(nn_, F32, 'out', name='dydz')
        dz.copy_(dy)
        _ok(_L().fgr_gelu_bwd(ar.put(z, name='z').data_ptr(), dz.data_ptr(), dz.data_ptr(), nn_,
                              _st()), 'fgr_gelu_bwd')
        return dz

    y, dz = _both(fwd, gpu), _both(bwd, gpu)
    assert torch.equal(_both(fwd_inplace, gpu), y)
    assert torch.equal(_both(bwd_inplace, gpu), dz)
    e, eb = rel_err(y, ref), rel_err(dz, dref)
    print(f'\ngelu n={n} fixed={fixed}: fwd {e:.3g} (torch {e_t:.3g}) bwd {eb:.3g} (torch {eb_t:.3g}) '
          f'max|ref| {float(ref.abs().max()):.3g} / {float(dref.abs().max()):.3g}')
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dz).all())
    assert e < 4 * e_t + 1e-7, (e, e_t)
    assert eb < 4 * eb_t + 1e-7, (eb, eb_t)
    if fixed:
        yc, k = y.cpu(), n + FIXED.index(-30.0)
        assert float(yc[k]) == 0.0 and float(yc[n + FIXED.index(30.0)]) == 30.0
        assert float(yc[n + FIXED.index(-1e4)]) == 0.0 and float(yc[n + FIXED.index(1e4)]) == 1e4
        assert float(yc[n]) == 0.0                                    # gelu(0) = 0
        dc = dz.cpu()
        assert float(dc[k]) == 0.0 and float(dc[n + FIXED.index(30.0)]) == float(dy[n + FIXED.index(30.0)])


def test_gelu_refusals_and_wrappers(gpu):
    import fgreg
    from fgreg import _lib, ops
    buf = torch.zeros(64, device=gpu)
    p = buf.data_ptr()
    assert p % 16 == 0
    L, st = _L(), _st()
    with pytest.raises(fgreg.FgrError, match='aligned'):
        _lib.check(L.fgr_gelu_fwd(p + 4, p + 128, 8, st), 'fgr_gelu_fwd')        # misaligned input
    with pytest.raises(fgreg.FgrError, match='aligned'):
        _lib.check(L.fgr_gelu_bwd(p, p + 64, p + 132, 8, st), 'fgr_gelu_bwd')    # misaligned output
    with pytest.raises(fgreg.FgrError, match='overlaps'):
        _lib.check(L.fgr_gelu_fwd(p, p + 16, 8, st), 'fgr_gelu_fwd')             # partial overlap
    with pytest.raises(fgreg.FgrError, match='overlaps'):
        _lib.check(L.fgr_gelu_bwd(p, p + 64, p + 80, 8, st), 'fgr_gelu_bwd')
    with pytest.raises(fgreg.FgrError):
        _lib.check(L.fgr_gelu_fwd(None, p, 8, st), 'fgr_gelu_fwd')               # null
    with pytest.raises(fgreg.FgrError):
        _lib.check(L.fgr_gelu_fwd(p, p, -1, st), 'fgr_gelu_fwd')                 # n < 0
    assert L.fgr_gelu_fwd(None, None, 0, st) == 0 and L.fgr_gelu_bwd(None, None, None, 0, st) == 0
    torch.cuda.synchronize()
    assert not bool(buf.any())
    # the wrappers: any shape, in place, host tensors refused
    z = torch.randn(3, 5, 7, generator=torch.Generator().manual_seed(0)).to(gpu)
    y = ops.gelu(z)
    assert y.shape == z.shape and rel_err(y, F.gelu(z.double())) < 1e-6
    g = ops.gelu_backward(z, torch.ones_like(z))
    zz = z.clone().requires_grad_(True)
    F.gelu(zz.double()).sum().backward()
    assert rel_err(g, zz.grad) < 1e-6
    w = z.clone()
    assert ops.gelu_(w) is w and torch.equal(w, y)
    assert ops.gelu(torch.empty(0, 4, device=gpu)).shape == (0, 4)
    with pytest.raises(fgreg.FgrError):
        ops.gelu(torch.zeros(4))
    with pytest.raises(fgreg.FgrError):
        ops.gelu_backward(torch.zeros(4), torch.zeros(4))


# ---------------------------------------------------------------------------------------------
# the fused feed-forward with GELU (test_gpu_ffn.py's _layer / _ref64, restated with F.gelu)
# ---------------------------------------------------------------------------------------------
def _layer(d, f, seed, big_row=False, neg_bias=False):
    g = torch.Generator().manual_seed(seed)
    norm = torch.nn.LayerNorm(d)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * torch.randn(d, generator=g))
        norm.bias.copy_(0.2 * torch.randn(d, generator=g))
    w1 = torch.randn(f, d, generator=g) / math.sqrt(d)
    b1 = 0.5 * torch.randn(f, generator=g)
    w2 = torch.randn(d, f, generator=g) / math.sqrt(f)
    b2 = torch.randn(d, generator=g)
    if big_row:
        w1[3] *= 1e4                    # erf saturates on both sides of this hidden unit
    if neg_bias:
        b1 -= 3.0                       # most hidden units in GELU's negative tail (ReLU: 0)
    return norm, w1, b1, w2, b2


def _ref64(x, norm, w1, b1, w2, b2):
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    a = (xd - mu) / torch.sqrt(var + norm.eps) * norm.weight.double() + norm.bias.double()
    h = F.gelu(a @ w1.double().t() + b1.double())
    return xd + h @ w2.double().t() + b2.double()


def _run(gpu, x, norm, w1, b1, w2, b2, out=None, act=ACT_GELU):
    from fgreg import linear as fl
    from fgreg import ops
    W1, B1, W2, B2 = (t.to(gpu) for t in (w1, b1, w2, b2))
    bound = torch.stack([W1.norm(dim=1).max(), B1.abs().max()]).contiguous()
    return ops.ffn(x, norm.to(gpu), fl.weight_image(W1, mode='f16x3', cache=False), B1,
                   fl.weight_image(W2, mode='ffn2', cache=False), B2, bound, out=out, act=act)


# (12300, 1024): past 48 x 256 rows, where the ReLU dispatcher switches to 64-row blocks; the
# GELU kernel exists with 48-row blocks only and takes a second round of the CUs there
@pytest.mark.parametrize('m,f', [(1, 1024), (65, 1024), (777, 2048), (500, 128), (12300, 1024)])
@pytest.mark.parametrize('case', ['plain', 'big_row', 'neg_bias'])
def test_ffn_gelu_vs_fp64(gpu, m, f, case):
    from fgreg import ops
    d = 256
    assert ops.ffn_supported(m, d, f, ACT_GELU)
    norm, w1, b1, w2, b2 = _layer(d, f, m + f, big_row=case == 'big_row',
                                  neg_bias=case == 'neg_bias')
    g = torch.Generator().manual_seed(m)
    x = 3.0 + 2.0 * torch.randn(m, d, generator=g)
    if m > 8:
        x[7] = 0.0                      # a constant row: LayerNorm gives beta
    ref = _ref64(x, norm, w1, b1, w2, b2)
    X = x.to(gpu)
    out = _run(gpu, X, norm, w1, b1, w2, b2)
    # torch fp32 (the comparison baseline only)
    N = norm.to(gpu)
    a32 = F.layer_norm(X, (d,), N.weight, N.bias, N.eps)
    h32 = F.gelu(torch.addmm(b1.to(gpu), a32, w1.to(gpu).t()))
    y32 = X + torch.addmm(b2.to(gpu), h32, w2.to(gpu).t())
    e32, e = rel_err(y32, ref), rel_err(out, ref)
    # the update alone (y - x): its error is not hidden by the residual's magnitude
    eu = rel_err(out - X, ref - x.double())
    eu32 = rel_err(y32 - X, ref - x.double())
    print(f'\nffn gelu m={m} f={f} {case}: e {e:.3g} (torch {e32:.3g}) update {eu:.3g} (torch {eu32:.3g})')
    assert e < 1e-5 and e < 4 * e32 + 1e-6, (e, e32)
    assert eu < 1e-5 and eu < 4 * eu32 + 1e-6, (eu, eu32)
    # in place: out = x gives the out-of-place result bit for bit
    Y = X.clone()
    got = _run(gpu, Y, norm, w1, b1, w2, b2, out=Y)
    assert got.data_ptr() == Y.data_ptr() and torch.equal(got, out)


def test_ffn_act_refusals(gpu):
    import fgreg
    L = _L()
    assert L.fgr_ffn_f16x3_act_supported(100, 256, 192, ACT_GELU) == 0      # f % 128 != 0
    assert L.fgr_ffn_f16x3_act_supported(100, 256, 192, ACT_RELU) == 1      # the LDS-ring kernel
    assert L.fgr_ffn_f16x3_act_supported(100, 512, 1024, ACT_GELU) == 0     # d != 256
    assert L.fgr_ffn_f16x3_act_supported(100, 256, 1024, ACT_GELU) == 1
    assert L.fgr_ffn_f16x3_act_supported(100, 256, 1024, ACT_LEAKY) == 0
    norm, w1, b1, w2, b2 = _layer(256, 1024, 1)
    x = torch.randn(100, 256, generator=torch.Generator().manual_seed(1)).to(gpu)
    with pytest.raises(fgreg.FgrError, match='act'):
        _run(gpu, x, norm, w1, b1, w2, b2, act=ACT_LEAKY)
    norm, w1, b1, w2, b2 = _layer(256, 192, 1)
    with pytest.raises(fgreg.FgrError):
        _run(gpu, x, norm, w1, b1, w2, b2, act=ACT_GELU)                    # f = 192 with GELU
    assert _run(gpu, x, norm, w1, b1, w2, b2, act=ACT_RELU).shape == (100, 256)


def test_ffn_gelu_equals_three_launch_path(gpu):
    """ops.ffn(act=ACT_GELU) against linear_ln -> gelu_ -> linear (+ residual): the same f16x3
    products with the hidden activations in HBM."""
    from fgreg import linear as fl
    from fgreg import ops
    m, d, f = 2000, 256, 1024
    norm, w1, b1, w2, b2 = _layer(d, f, 5)
    x = (3.0 + 2.0 * torch.randn(m, d, generator=torch.Generator().manual_seed(5))).to(gpu)
    out = _run(gpu, x, norm, w1, b1, w2, b2)
    N = norm.to(gpu)
    h = ops.gelu_(fl.linear_ln(x, N, w1.to(gpu), b1.to(gpu)))
    three = fl.linear(h, w2.to(gpu), b2.to(gpu), residual=x)
    assert rel_err(out - x, three - x) < 4e-6


@pytest.mark.parametrize('f,fused', [(1024, True), (192, False)])
def test_layer_dispatch(gpu, monkeypatch, f, fused):
    """The pre-norm layer takes the fused launch where ops.ffn_supported(.., ACT_GELU) and the
    three launches elsewhere; both give the same output; no GEMM wrapper accepts ACT_GELU."""
    import fgreg
    from fgreg import linear as fl
    from fgreg import ops
    from fgreg.transformer import Segments, TransformerCrossEncoderLayer
    torch.manual_seed(f)
    layer = TransformerCrossEncoderLayer(256, 8, f, 0.0, 'gelu', normalize_before=True,
                                         sa_val_has_pos_emb=True, ca_val_has_pos_emb=True)
    layer = layer.to(gpu).eval()
    seg = Segments([37, 50, 41, 29], gpu)
    g = torch.Generator().manual_seed(f + 1)
    x = torch.randn(157, 256, generator=g).to(gpu)
    pos = torch.randn(157, 256, generator=g).to(gpu)
    calls = []
    real_ffn, real_gelu = ops.ffn, ops.gelu_

    def spy_ffn(*a, **k):
        calls.append(('ffn', k.get('act')))
        return real_ffn(*a, **k)

    def spy_gelu(*a, **k):
        calls.append(('gelu_', a[0].shape[1]))
        return real_gelu(*a, **k)

    monkeypatch.setattr(ops, 'ffn', spy_ffn)
    monkeypatch.setattr(ops, 'gelu_', spy_gelu)
    with torch.no_grad():
        y, pending = layer.forward_packed(x.clone(), pos, seg)
        assert pending is None
        assert calls == ([('ffn', ACT_GELU)] if fused else [('gelu_', f)])
        monkeypatch.setattr(ops, 'FFN_FUSE', False)
        calls.clear()
        y3, _ = layer.forward_packed(x.clone(), pos, seg)
        assert calls == [('gelu_', f)]
        assert rel_err(y, y3) < 1e-5 and (fused or torch.equal(y, y3))
        with pytest.raises(fgreg.FgrError):
            fl.linear(x, layer.linear1.weight, layer.linear1.bias, act=ACT_GELU)
        with pytest.raises(fgreg.FgrError):
            fl.linear_ln(x, layer.norm3, layer.linear1.weight, layer.linear1.bias, act=ACT_GELU)


# ---------------------------------------------------------------------------------------------
# the reference's fixtures
# ---------------------------------------------------------------------------------------------
def _batch(src, tgt, dev):
    return {'src_xyz': [torch.from_numpy(np.asarray(s)).to(dev) for s in src],
            'tgt_xyz': [torch.from_numpy(np.asarray(t)).to(dev) for t in tgt]}


def _fixture_model(name, gpu, **over):
    import fgreg
    import fgreg.config as fc
    cfg, sd, src, tgt, meta, d = forward_fixture(name)
    if over:
        cfg = fc.get('modelnet', **dict(cfg_overrides(d), **over))
    model = fgreg.RegTR(cfg)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith('feature_criterion') for k in missing)
    model = model.to(gpu).eval()
    model.preprocessor = fgreg.FixedMetaPreprocessor(
        {k: [t.to(gpu) for t in v] for k, v in meta.items()})
    return model, src, tgt, d


def cfg_overrides(d):
    import ast
    return ast.literal_eval(str(d['cfg_overrides']))


def _errors(out, d, B):
    errs = {(k, b): rel_err(out[k][b], d[f'out.{k}.{b}']) for k in KEYS for b in range(B)}
    return errs, float(np.abs(out['pose'].cpu().numpy() - d['out.pose']).max())


@pytest.mark.parametrize('name', ['forward_modelnet_gelu', 'forward_modelnet_gelu_postnorm'])
def test_forward_on_reference_meta(gpu, name):
    """Three calls in a row: eager, the capturing second sighting, a graph replay."""
    model, src, tgt, d = _fixture_model(name, gpu)
    assert all(l.act == ACT_GELU for l in model.transformer_encoder.layers)
    for call in range(3):
        out = model(_batch(src, tgt, gpu))
        errs, pose = _errors(out, d, len(src))
        for kb, e in errs.items():
            assert e < TOL, (call, kb, e)
        assert pose < TOL, (call, pose)


def test_relu_model_fails_the_gelu_fixture(gpu):
    """The option is not ignored: the same weights with transformer_act='relu' miss the bound."""
    model, src, tgt, d = _fixture_model('forward_modelnet_gelu', gpu, transformer_act='relu')
    assert all(l.act == ACT_RELU for l in model.transformer_encoder.layers)
    out = model(_batch(src, tgt, gpu))
    assert min(rel_err(out['src_feat'][b], d[f'out.src_feat.{b}']) for b in range(len(src))) > TOL


def _rot_deg(a, b):
    r = a[:, :3] @ b[:, :3].T
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(r) - 1) / 2))))


@pytest.mark.parametrize('name', ['forward_modelnet_gelu', 'forward_modelnet_gelu_postnorm'])
def test_forward_bf16(gpu, name):
    """The bf16 mode (the GELU itself stays fp32, on the GEMM's fp32 output) within the bf16
    mode's stated tolerances (test_gpu_bf16.py)."""
    import fgreg
    model, src, tgt, d = _fixture_model(name, gpu)
    old = fgreg.precision()
    fgreg.set_precision('bf16')
    try:
        out = model(_batch(src, tgt, gpu))
    finally:
        fgreg.set_precision(old)
    errs, _ = _errors(out, d, len(src))
    worst = max(errs.values())
    print(f'\nbf16 {name}: worst rel err {worst:.3g}')
    for kb, e in errs.items():
        assert e < BF16_FEAT_TOL, (kb, e)
    assert worst > TOL                      # really the bf16 mode
    pose, ref = out['pose'].cpu().numpy(), d['out.pose']
    for b in range(len(src)):
        p, pr = pose[-1, b], ref[-1, b]
        rot, trans = _rot_deg(p, pr), float(np.linalg.norm(p[:, 3] - pr[:, 3]))
        assert rot < BF16_ROT_DEG and trans < BF16_TRANS, (b, rot, trans)


def _same(a, b):
    for k in KEYS:
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x, y), k
    assert torch.equal(a['pose'], b['pose'])


def test_full_width_graph_and_pipeline(gpu, monkeypatch):
    """The ModelNet config (d_embed 256, d_feedforward 1024: the fused GELU launch in every
    layer) with random weights: graph replay equals the eager forward, fgreg.pipeline over two
    batches equals model(batch), and the fused launch really is what runs."""
    import fgreg
    import fgreg.regtr as rt
    from fgreg import ops
    from fgreg.synthetic import make_batch
    torch.manual_seed(3)
    np.random.seed(3)
    model = fgreg.RegTR(fgreg.config.get('modelnet', transformer_act='gelu')).to(gpu).eval()
    batches = []
    for start in (0, 4):
        src, tgt, _ = make_batch('modelnet', 2, start=start)
        batches.append(_batch(src, tgt, gpu))
    calls = []
    real_ffn = ops.ffn
    monkeypatch.setattr(ops, 'ffn', lambda *a, **k: (calls.append(k.get('act')), real_ffn(*a, **k))[1])
    monkeypatch.setattr(rt, 'GRAPHS', False)
    with torch.no_grad():
        eager = model(dict(batches[0]))
    n_layers = len(model.transformer_encoder.layers)
    assert calls == [ACT_GELU] * n_layers
    monkeypatch.setattr(rt, 'GRAPHS', True)
    with torch.no_grad():
        model(dict(batches[0]))
        model(dict(batches[0]))                       # second sighting: captured
        assert len(rt._GRAPHS[model]['graphs']) == 1
        _same(model(dict(batches[0])), eager)         # replay
    got = list(fgreg.pipeline(model, [dict(b) for b in batches], depth=2, streams=2))
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = [model(dict(b)) for b in batches]
    assert len(got) == 2
    for a, r in zip(got, ref):
        _same(a, r)


def test_train_step_vs_reference(gpu):
    """The reference's train() step on the GELU model (train_modelnet_gelu.npz) vs fgreg's:
    losses within 1e-5, every gradient norm and every stored full gradient (layer 0's linear1
    weight and bias included: the GELU's own backward) within GRAD_TOL."""
    import fgreg
    import loss_oracle as lo
    cfg, sd, src, tgt, meta, _ = forward_fixture('forward_modelnet_gelu')
    _, _, batch, _, _, _, W, W_un = loss_fixture()
    ref = golden('train_modelnet_gelu')
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
    for k in ('transformer_encoder.layers.0.linear1.weight', 'transformer_encoder.layers.0.linear1.bias'):
        assert 'grad.' + k in ref.files and float(grads[k].abs().max()) > 0.0, k
    norms = {k[6:] for k in ref.files if k.startswith('gnorm.')}
    assert norms == {k for k in grads if is_trainable(k)}, norms ^ set(grads)
    nerr, serr = {}, {}
    for k in sorted(norms):
        n_ref = float(ref['gnorm.' + k])
        nerr[k] = abs(float(grads[k].double().norm()) - n_ref) / max(n_ref, 1e-12)
        # the sums against the gradient's own scale (a sum of cancelling terms has no relative bound)
        serr[k] = abs(float(grads[k].double().sum()) - float(ref['gsum.' + k])) / max(
            n_ref * math.sqrt(grads[k].numel()), 1e-12)
    ferr = {}
    for k in ref.files:
        if k.startswith('grad.'):
            a, r = grads[k[5:]].detach().double().cpu(), torch.from_numpy(ref[k]).double()
            ferr[k[5:]] = float((a - r).norm() / max(float(r.norm()), 1e-30))
    print('\nworst gradient-norm errors', sorted(((v, k) for k, v in nerr.items()), reverse=True)[:5],
          '\nfull-gradient Frobenius errors', {k[-40:]: f'{v:.1e}' for k, v in ferr.items()})
    for k, e in nerr.items():
        assert e < GRAD_TOL, (k, e)
    for k, e in serr.items():
        assert e < GRAD_TOL, (k, e)
    for k, e in ferr.items():
        assert e < GRAD_TOL, (k, e)
