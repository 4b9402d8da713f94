"""Deformable / modulated KPConv on the GPU: fgr_kpconv_deform_points, fgr_kpconv_gather_deform
(narrow and wide families, 16 and 32 kernel-point instances), fgr_kpconv_scatter_deform and
fgr_kpconv_deform_grad against the fp64 restatement of finegrained_kpconv_blocks.py:270-345,
:384-399 (tests/_kpconv_deform.py, which also states the table's edit rule), in a guarded arena,
and the reference's own fixtures (tests/golden/make_golden_deform.py).

Forward bound (test_gpu_dispatch's): the conditioned error max |wf - ref| / (|mod| sum_h w_h |x_h|)
is at most 4 x the torch fp32 restatement's own error + 1e-7 and never above 1e-4; nnorm is exact.
Both errors are printed before the assertion.
"""
import ast
import math

import numpy as np
import pytest
import torch

import _kpconv_deform as kd
import _kpconv_modes as km
from _arena import SENTINEL, Arena, assert_both_equal, run_both
from conftest import forward_fixture, golden, loss_fixture, rel_err

pytestmark = pytest.mark.gpu
F32 = torch.float32
CAP, TOL = 1e-4, 1e-4                  # test_gpu_dispatch's, test_gpu_forward's
EXT = kd.EXT
CODES = {'linear': 0, 'gaussian': 1, 'constant': 2, 'sum': 0, 'closest': 1}
KEYS = ['src_feat_un', 'tgt_feat_un', 'src_feat', 'tgt_feat', 'src_kp', 'tgt_kp',
        'src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap']
# n_kp 15 at every width and both row lengths (H 7: the pad rows are live; H 70: a second
# 64-wide chunk); n_kp 17 / 32: the 32-kernel-point instances of the narrow and wide kernels
SHAPES = [(cin, H, 15) for cin in (1, 3, 12, 16, 32, 48, 64, 128, 256) for H in (7, 70)] + \
         [(1, 7, 17), (64, 70, 17), (64, 7, 32), (256, 70, 32)]
# one unmodulated case per kernel family: narrow / wide x 16 / 32 kernel points
UNMODULATED = [(12, 70, 15, 'linear', 'sum'), (3, 7, 17, 'constant', 'closest'),
               (64, 7, 15, 'constant', 'sum'), (128, 70, 15, 'gaussian', 'closest'),
               (256, 70, 32, 'linear', 'closest')]


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


def _bound(e32):
    return min(4 * e32 + 1e-7, CAP)


def _hold(what, e, e32):
    print(f'kpconv-deform-error {what}: kernel {e:.3e} fp32-restatement {e32:.3e}')
    assert e <= _bound(e32), (what, e, e32)


def _gather(gpu, t, influence, aggregation, modulated=True):
    import fgreg.ops as ops
    q, s, idx, x, kp, kp_q, mod = t[:7]
    return ops.kpconv_gather_deform(q.to(gpu), s.to(gpu), idx.to(gpu), x.to(gpu), kp_q.to(gpu),
                                    mod.to(gpu) if modulated else None, EXT, influence, aggregation)


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('influence,aggregation', kd.COMBOS)
@pytest.mark.parametrize('cin,H,n_kp', SHAPES)
def test_gather_deform_vs_fp64(gpu, cin, H, n_kp, influence, aggregation):
    t = kd.table(cin, H, n_kp)
    ref, den, e32 = kd.reference(cin, H, n_kp, influence, aggregation)
    wf, nn_ = _gather(gpu, t, influence, aggregation)
    _hold(f'{influence}/{aggregation} cin {cin} n_kp {n_kp} H {H}', km.cond_err(wf, ref, den), e32)
    assert torch.equal(nn_.cpu(), t[7])
    assert bool((wf[3] == 0).all()) and float(nn_[3]) == 1.0          # the all-shadow row


@pytest.mark.parametrize('cin,H,n_kp,influence,aggregation', UNMODULATED)
def test_gather_deform_unmodulated(gpu, cin, H, n_kp, influence, aggregation):
    """mod NULL: one case per kernel family."""
    t = kd.table(cin, H, n_kp)
    ref, den, e32 = kd.reference(cin, H, n_kp, influence, aggregation, modulated=False)
    wf, nn_ = _gather(gpu, t, influence, aggregation, modulated=False)
    _hold(f'unmodulated {influence}/{aggregation} cin {cin} n_kp {n_kp} H {H}',
          km.cond_err(wf, ref, den), e32)
    assert torch.equal(nn_.cpu(), t[7])


@pytest.mark.parametrize('cin,H', [(12, 70), (64, 7), (256, 70)])
def test_in_range_mask_changes_nnorm(gpu, cin, H):
    """The table's builder asserts that the in-range mask changes nnorm for at least one query
    (stats['nnorm_changed']): a kernel that counts every valid neighbour fails here."""
    t = kd.table(cin, H, 15)
    q, s, idx, x = t[:4]
    nx = torch.cat([x.double(), torch.zeros(1, cin, dtype=torch.float64)])[idx]
    cnt_all = torch.clamp((nx.sum(-1) > 0).sum(-1), min=1).float()
    _, nn_ = _gather(gpu, t, 'linear', 'sum')
    assert t[8]['nnorm_changed'] >= 1 and not torch.equal(t[7], cnt_all)
    assert torch.equal(nn_.cpu(), t[7])


@pytest.mark.parametrize('cin', [12, 128])
def test_ignoring_mod_fails_the_bound(gpu, cin):
    """The unmodulated result misses the modulated reference's bound: the check sees mod."""
    t = kd.table(cin, 70, 15)
    ref, den, e32 = kd.reference(cin, 70, 15, 'gaussian', 'sum')
    wf, _ = _gather(gpu, t, 'gaussian', 'sum', modulated=False)
    assert km.cond_err(wf, ref, den) > 100 * _bound(e32)
    wf, _ = _gather(gpu, t, 'gaussian', 'sum')
    assert km.cond_err(wf, ref, den) <= _bound(e32)


@pytest.mark.parametrize('influence,aggregation', [('linear', 'sum'), ('gaussian', 'closest'),
                                                   ('constant', 'sum')])
@pytest.mark.parametrize('cin', [1, 16, 48, 128])
def test_undeformed_equals_the_rigid_gather(gpu, cin, influence, aggregation):
    """kp_q = the rigid kernel points for every query and every valid entry in range (the others
    made shadows): nnorm equals fgr_kpconv_gather_mode's and both wf meet the same bound against
    the fp64 rigid restatement."""
    import fgreg.ops as ops
    q, s, idx, x, kp, _ = km.table(cin, 70, 15)
    idx = idx.clone()
    d2 = km.sq_distances(q.double(), s.double(), idx, kp.double())
    r = torch.sqrt(d2) / EXT
    # out of range, or within the 2 % boundary zone of the in-range test under any kernel point
    idx[~((r < 0.98).any(2)) & (idx < s.shape[0])] = s.shape[0]
    assert int((idx < s.shape[0]).sum()) >= 20
    ref, den = km.gather_ref(q, s, idx, x, kp, EXT, influence, aggregation, torch.float64)
    if influence == 'gaussian':
        den = den + 70 * 2.0 ** -126 * float(x.abs().max())
    e32 = km.cond_err(km.gather_ref(q, s, idx, x, kp, EXT, influence, aggregation, F32)[0], ref, den)
    dev = [a.to(gpu) for a in (q, s, idx, x)]
    kp_q = kp.to(gpu).unsqueeze(0).expand(q.shape[0], -1, -1).contiguous()
    wf_r, nn_r = ops.kpconv_gather(*dev, kp.to(gpu), EXT, influence, aggregation)
    wf_d, nn_d = ops.kpconv_gather_deform(*dev, kp_q, None, EXT, influence, aggregation)
    assert torch.equal(nn_r, nn_d)
    _hold(f'undeformed {influence}/{aggregation} cin {cin} (rigid)', km.cond_err(wf_r, ref, den), e32)
    _hold(f'undeformed {influence}/{aggregation} cin {cin} (deform)', km.cond_err(wf_d, ref, den), e32)


@pytest.mark.parametrize('modulated', [False, True])
def test_deform_points_vs_fp64(gpu, modulated):
    """fgr_kpconv_deform_points against the fp64 chain of :272-306, within 1e-6 (a division, two
    additions, a product and a sigmoid in fp32)."""
    import fgreg.ops as ops
    g = torch.Generator().manual_seed(7)
    nq, K = 70, 15
    raw = torch.randn(nq, (4 if modulated else 3) * K, generator=g) * 3
    rn = torch.randint(1, 9, (nq,), generator=g).float()
    bias = torch.randn(raw.shape[1], generator=g) * 0.3
    kp = torch.randn(K, 3, generator=g) * 0.3
    kp_q, mod = ops.kpconv_deform_points(raw.to(gpu), rn.to(gpu), bias.to(gpu), kp.to(gpu), EXT, modulated)
    f64 = raw.double() / rn.double().unsqueeze(1) + bias.double()
    r_kp, r_mod = kd.deform_points_ref(f64, kp.double(), EXT, modulated)
    assert rel_err(kp_q, r_kp) < 1e-6
    assert (mod is None) == (not modulated)
    if modulated:
        assert rel_err(mod, r_mod) < 1e-6


# ---------------------------------------------------------------------------------------------
# guarded arena
# ---------------------------------------------------------------------------------------------
def _gather_abi(ar, t, cin, n_kp, H, inf, agg, modulated=True, extent=EXT):
    q, s, idx, x, kp, kp_q, mod = t[:7]
    nq, ns = q.shape[0], s.shape[0]
    wf = ar.matrix(nq, n_kp * cin, n_kp * cin, F32, 'out', name='wf')
    nn_ = ar.vector(nq, F32, 'out', name='nnorm')
    rc = _L().fgr_kpconv_gather_deform(
        _p(ar.put(q, name='q')), _p(ar.put(s, name='s')), nq, ns,
        _p(ar.put(idx, name='idx')) if H else None, H, _p(ar.put(x, name='x')), cin,
        _p(ar.put(kp_q.reshape(nq, -1), name='kp_q')),
        _p(ar.put(mod, name='mod')) if modulated else None, n_kp, extent, inf, agg, _p(wf), _p(nn_),
        None, 0, _st())
    return rc, wf, nn_


@pytest.mark.parametrize('cin,H,n_kp,influence,aggregation,modulated', [
    (1, 70, 15, 'gaussian', 'closest', True), (12, 7, 15, 'constant', 'closest', True),
    (48, 7, 17, 'constant', 'sum', False), (64, 7, 15, 'constant', 'sum', True),
    (128, 70, 15, 'gaussian', 'closest', False), (256, 70, 32, 'linear', 'sum', True)])
def test_gather_deform_footprint(gpu, cin, H, n_kp, influence, aggregation, modulated):
    """One case per family through ctypes: exact bytes (every wf / nnorm element written, nothing
    outside them), clean run equal to the poisoned run, and the bound. The H 7 / constant cases
    are the pad-row trap: a pad row whose weight came from the influence function would add x[0]
    to every kernel point's sum."""
    t = kd.table(cin, H, n_kp)
    ref, den, e32 = kd.reference(cin, H, n_kp, influence, aggregation, modulated)

    def fn(ar):
        rc, wf, nn_ = _gather_abi(ar, t, cin, n_kp, H, CODES[influence], CODES[aggregation], modulated)
        _ok(rc, 'fgr_kpconv_gather_deform')
        return wf, nn_
    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    _hold(f'arena {influence}/{aggregation} cin {cin} H {H}',
          km.cond_err(clean[0].reshape(ref.shape), ref, den), e32)
    assert torch.equal(clean[1].cpu(), t[7])


@pytest.mark.parametrize('influence,aggregation', [('constant', 'sum'), ('gaussian', 'closest')])
@pytest.mark.parametrize('cin', [1, 12, 64, 256])
def test_gather_deform_width_zero(gpu, cin, influence, aggregation):
    """An empty neighbour table (width 0, idx NULL): wf all zeros and nnorm all ones."""
    t = kd.table(cin, 7, 15)
    ar = Arena(gpu)
    rc, wf, nn_ = _gather_abi(ar, t, cin, 15, 0, CODES[influence], CODES[aggregation])
    _ok(rc, 'fgr_kpconv_gather_deform')
    torch.cuda.synchronize()
    ar.check()
    assert bool((wf == 0).all()) and bool((nn_ == 1).all())


@pytest.mark.parametrize('modulated', [False, True])
def test_deform_points_footprint(gpu, modulated):
    g = torch.Generator().manual_seed(11)
    nq, K = 70, 15
    raw = torch.randn(nq, (4 if modulated else 3) * K, generator=g)
    rn = torch.randint(1, 9, (nq,), generator=g).float()
    bias = torch.randn(raw.shape[1], generator=g) * 0.3
    kp = torch.randn(K, 3, generator=g) * 0.3

    def fn(ar):
        kp_q = ar.matrix(nq, 3 * K, 3 * K, F32, 'out', name='kp_q')
        mod = ar.matrix(nq, K, K, F32, 'out', name='mod') if modulated else None
        _ok(_L().fgr_kpconv_deform_points(_p(ar.put(raw, name='raw')), _p(ar.put(rn, name='rn')),
                                          _p(ar.put(bias, name='bias')), _p(ar.put(kp.reshape(1, -1), name='kp')),
                                          nq, K, EXT, _p(kp_q), _p(mod), _st()), 'fgr_kpconv_deform_points')
        return (kp_q, mod) if modulated else kp_q
    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    f64 = raw.double() / rn.double().unsqueeze(1) + bias.double()
    r_kp, _ = kd.deform_points_ref(f64, kp.double(), EXT, modulated)
    assert rel_err((clean[0] if modulated else clean).reshape(nq, K, 3), r_kp) < 1e-6


def _scatter_abi(ar, t, dwf, cin, n_kp, H, inf, agg, modulated=True):
    from fgreg import _lib
    from fgreg.autograd import nbr_inverse
    q, s, idx, x, kp, kp_q, mod = t[:7]
    nq, ns = q.shape[0], s.shape[0]
    start, pos, _ = nbr_inverse(idx.to(ar.device), ns)
    nb = _lib.ws_size('fgr_kpconv_scatter_deform_workspace', nq, H, cin)
    dx = ar.matrix(ns, cin, cin, F32, 'out', name='dx')
    ws = ar.bytes(nb, name='ws')
    rc = _L().fgr_kpconv_scatter_deform(
        _p(ar.put(q, name='q')), _p(ar.put(s, name='s')), nq, ns, _p(ar.put(idx, name='idx')), H,
        _p(ar.put(dwf, name='dwf')), cin, _p(ar.put(kp_q.reshape(nq, -1), name='kp_q')),
        _p(ar.put(mod, name='mod')) if modulated else None, n_kp, EXT, inf, agg,
        _p(ar.put(start.cpu(), name='start')), _p(ar.put(pos.cpu().reshape(nq, H), name='pos')),
        _p(dx), _p(ws), nb, _st())
    return rc, dx


def _grad_abi(ar, t, dwf, cin, n_kp, H, inf, agg, modulated=True):
    q, s, idx, x, kp, kp_q, mod = t[:7]
    nq, ns = q.shape[0], s.shape[0]
    d_kp = ar.matrix(nq, 3 * n_kp, 3 * n_kp, F32, 'out', name='d_kp')
    d_mod = ar.matrix(nq, n_kp, n_kp, F32, 'out', name='d_mod') if modulated else None
    rc = _L().fgr_kpconv_deform_grad(
        _p(ar.put(q, name='q')), _p(ar.put(s, name='s')), nq, ns,
        _p(ar.put(idx, name='idx')) if H else None, H, _p(ar.put(x, name='x')), cin,
        _p(ar.put(dwf, name='dwf')), _p(ar.put(kp_q.reshape(nq, -1), name='kp_q')),
        _p(ar.put(mod, name='mod')) if modulated else None, n_kp, EXT, inf, agg, _p(d_kp), _p(d_mod),
        _st())
    return rc, d_kp, d_mod


def _ref_grads(t, dwf, influence, aggregation, modulated, dtype=torch.float64):
    """autograd of the restatement: d (wf . dwf) / d (x, kp_q, mod)."""
    q, s, idx, x, kp, kp_q, mod = t[:7]
    # copies: the cached table stays as it is
    xg, kg = x.clone().to(dtype).requires_grad_(True), kp_q.clone().to(dtype).requires_grad_(True)
    mg = mod.clone().to(dtype).requires_grad_(True) if modulated else None
    wf, _, _ = kd.gather_ref(q, s, idx, xg, kg, mg, EXT, influence, aggregation, dtype)
    (wf.reshape(dwf.shape) * dwf.to(dtype)).sum().backward()
    return xg.grad, kg.grad, (mg.grad if modulated else None)


@pytest.mark.parametrize('cin,n_kp,influence,aggregation,modulated',
                         [(12, 15, 'gaussian', 'closest', True), (128, 17, 'linear', 'sum', False)])
def test_scatter_deform_footprint(gpu, cin, n_kp, influence, aggregation, modulated):
    """fgr_kpconv_scatter_deform through ctypes with the exact workspace: exact bytes, clean =
    poisoned, dx within test_kpconv_backward's 1e-5 of the fp64 autograd of the restatement."""
    H = 70
    t = kd.table(cin, H, n_kp)
    dwf = torch.randn(t[0].shape[0], n_kp * cin, generator=torch.Generator().manual_seed(5))
    dx64, _, _ = _ref_grads(t, dwf, influence, aggregation, modulated)

    def fn(ar):
        rc, dx = _scatter_abi(ar, t, dwf, cin, n_kp, H, CODES[influence], CODES[aggregation], modulated)
        _ok(rc, 'fgr_kpconv_scatter_deform')
        return dx
    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    assert rel_err(clean, dx64) < 1e-5, rel_err(clean, dx64)


def _grad_bound(e32):
    return min(max(4 * e32, 1e-6), CAP)


@pytest.mark.parametrize('cin,n_kp,influence,aggregation,modulated',
                         [(12, 15, 'gaussian', 'closest', True), (128, 17, 'linear', 'sum', False),
                          (64, 32, 'gaussian', 'sum', True)])
def test_deform_grad_footprint(gpu, cin, n_kp, influence, aggregation, modulated):
    """fgr_kpconv_deform_grad through ctypes: exact bytes, clean = poisoned, d_kp / d_mod within
    the backward test's bound of the fp64 autograd."""
    H = 70
    t = kd.table(cin, H, n_kp)
    nq = t[0].shape[0]
    dwf = torch.randn(nq, n_kp * cin, generator=torch.Generator().manual_seed(6))
    _, dk64, dm64 = _ref_grads(t, dwf, influence, aggregation, modulated)
    _, dk32, dm32 = _ref_grads(t, dwf, influence, aggregation, modulated, F32)

    def fn(ar):
        rc, d_kp, d_mod = _grad_abi(ar, t, dwf, cin, n_kp, H, CODES[influence], CODES[aggregation], modulated)
        _ok(rc, 'fgr_kpconv_deform_grad')
        return (d_kp, d_mod) if modulated else d_kp
    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    d_kp = (clean[0] if modulated else clean).reshape(nq, n_kp, 3)
    e, e32 = rel_err(d_kp, dk64), rel_err(dk32, dk64)
    print(f'kpconv-deform-grad arena d_kp: kernel {e:.3e} fp32-restatement {e32:.3e}')
    assert e <= _grad_bound(e32)
    if modulated:
        e, e32 = rel_err(clean[1], dm64), rel_err(dm32, dm64)
        print(f'kpconv-deform-grad arena d_mod: kernel {e:.3e} fp32-restatement {e32:.3e}')
        assert e <= _grad_bound(e32)


def test_deform_grad_width_zero(gpu):
    t = kd.table(12, 7, 15)
    ar = Arena(gpu)
    rc, d_kp, d_mod = _grad_abi(ar, t, torch.ones(70, 15 * 12), 12, 15, 0, 0, 0)
    _ok(rc, 'fgr_kpconv_deform_grad')
    torch.cuda.synchronize()
    ar.check()
    assert bool((d_kp == 0).all()) and bool((d_mod == 0).all())


@pytest.mark.parametrize('bad', [dict(inf=7), dict(agg=2), dict(cin=96), dict(n_kp=33), dict(extent=0.0)])
def test_bad_argument_is_refused_before_any_launch(gpu, bad):
    """FGR_E_ARG from every entry point, the entry point and the value named in fgr_last_error,
    and every sentinel of the outputs and the workspace intact."""
    t = kd.table(16, 7, 15)
    q, s, idx, x, kp, kp_q, mod = t[:7]
    nq, ns = q.shape[0], s.shape[0]
    inf, agg = bad.get('inf', 0), bad.get('agg', 0)
    cin, n_kp, extent = bad.get('cin', 16), bad.get('n_kp', 15), bad.get('extent', EXT)
    ar = Arena(gpu)
    P = {k: _p(ar.put(v, name=k)) for k, v in dict(q=q, s=s, idx=idx, x=x, kp_q=kp_q.reshape(nq, -1),
                                                    mod=mod, kp=kp.reshape(1, -1),
                                                    dwf=torch.zeros(nq, 15 * 16),
                                                    start=torch.zeros(ns + 1, dtype=torch.int32),
                                                    pos=torch.zeros(nq, 7, dtype=torch.int32),
                                                    raw=torch.zeros(nq, 60), rn=torch.ones(nq),
                                                    bias=torch.zeros(60)).items()}
    out = {k: _p(ar.matrix(r, c, c, F32, 'out', name=k)) for k, (r, c) in dict(
        wf=(nq, 15 * 16), nnorm=(1, nq), dx=(ns, 16), d_kp=(nq, 45), d_mod=(nq, 15), o_kp=(nq, 45),
        o_mod=(nq, 15)).items()}
    ws = ar.bytes(nq * 7 * 16 * 4, name='ws')
    L = _L()
    calls = {
        'fgr_kpconv_gather_deform': lambda: L.fgr_kpconv_gather_deform(
            P['q'], P['s'], nq, ns, P['idx'], 7, P['x'], cin, P['kp_q'], P['mod'], n_kp, extent, inf,
            agg, out['wf'], out['nnorm'], None, 0, _st()),
        'fgr_kpconv_scatter_deform': lambda: L.fgr_kpconv_scatter_deform(
            P['q'], P['s'], nq, ns, P['idx'], 7, P['dwf'], cin, P['kp_q'], P['mod'], n_kp, extent,
            inf, agg, P['start'], P['pos'], out['dx'], _p(ws), ws.numel(), _st()),
        'fgr_kpconv_deform_grad': lambda: L.fgr_kpconv_deform_grad(
            P['q'], P['s'], nq, ns, P['idx'], 7, P['x'], cin, P['dwf'], P['kp_q'], P['mod'], n_kp,
            extent, inf, agg, out['d_kp'], out['d_mod'], _st()),
    }
    if 'n_kp' in bad or 'extent' in bad:
        calls['fgr_kpconv_deform_points'] = lambda: L.fgr_kpconv_deform_points(
            P['raw'], P['rn'], P['bias'], P['kp'], nq, n_kp, extent, out['o_kp'], out['o_mod'], _st())
    what = {'inf': 'influence 7', 'agg': 'aggregation 2', 'cin': 'cin 96', 'n_kp': 'n_kp 33',
            'extent': 'extent 0'}[next(iter(bad))]
    for name, call in calls.items():
        assert call() == -1, name
        msg = L.fgr_last_error().decode()
        assert name + ':' in msg and what in msg, msg
    torch.cuda.synchronize()
    for r in ar.regions:
        if r.role == 'out':
            assert bool((r.buf.view(torch.int32) == SENTINEL).all()), r.name
        elif r.role == 'scratch':
            assert bool((r.view == 0).all()), r.name


# ---------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('influence,aggregation', kd.COMBOS)
@pytest.mark.parametrize('cin', [1, 12, 16, 64, 128])
def test_kpconv_deform_backward(gpu, cin, influence, aggregation):
    """The autograd function of kpconv_deform_t (gather_deform + weight GEMM; dx through
    fgr_kpconv_scatter_deform, d_kp / d_mod through fgr_kpconv_deform_grad, dW through the
    regathered wf) vs fp64 autograd of the restatement: y, dx, dW within test_kpconv_backward's
    1e-5; d_kp, d_mod within min(max(4 x the fp32 restatement autograd's own error, 1e-6), 1e-4);
    d_kp exactly zero under constant; two runs bit-equal."""
    from fgreg.autograd import kpconv_deform_gather_t
    q, s, idx, x0, kp, kp_q0, mod0, _, _ = kd.table(cin, 70, 15)
    W0 = torch.randn(15, cin, 24, generator=torch.Generator().manual_seed(cin)) / math.sqrt(15 * cin)
    R = torch.randn(q.shape[0], 24, generator=torch.Generator().manual_seed(3))

    def ref(dtype):
        leaves = [t.clone().to(dtype).requires_grad_(True) for t in (x0, W0, kp_q0, mod0)]
        wf, _, cnt = kd.gather_ref(q, s, idx, leaves[0], leaves[2], leaves[3], EXT, influence,
                                   aggregation, dtype)
        y = torch.einsum('qkc,kco->qo', wf, leaves[1]) / cnt.unsqueeze(1)
        (y * R.to(dtype)).sum().backward()
        return [y.detach()] + [t.grad for t in leaves]

    def mine():
        leaves = [t.clone().to(gpu).requires_grad_(True) for t in (x0, W0, kp_q0, mod0)]
        out, nnorm = kpconv_deform_gather_t(leaves[0], leaves[1], leaves[2], leaves[3], q.to(gpu),
                                            s.to(gpu), idx.to(gpu), EXT, influence, aggregation)
        y = out / nnorm.unsqueeze(1)
        (y * R.to(gpu)).sum().backward()
        return [y.detach()] + [t.grad for t in leaves]

    r64, r32, got, again = ref(torch.float64), ref(F32), mine(), mine()
    for a, b in zip(got, again):
        assert torch.equal(a, b)                        # deterministic: no atomics
    errs = [rel_err(a, b) for a, b in zip(got[:3], r64[:3])]
    print(f'kpconv-deform-backward {influence}/{aggregation} cin {cin}: y {errs[0]:.2e} dx {errs[1]:.2e} '
          f'dW {errs[2]:.2e}')
    assert max(errs) < 1e-5, errs
    if influence == 'constant':
        # the restatement's kp_q has no path to the output at all (autograd: no gradient)
        assert bool((got[3] == 0).all()) and (r64[3] is None or bool((r64[3] == 0).all()))
    for i, name in ((3, 'd_kp'), (4, 'd_mod')):
        if name == 'd_kp' and influence == 'constant':
            continue
        e, e32 = rel_err(got[i], r64[i]), rel_err(r32[i], r64[i])
        print(f'kpconv-deform-backward {influence}/{aggregation} cin {cin} {name}: kernel {e:.3e} '
              f'fp32-restatement {e32:.3e}')
        assert e <= _grad_bound(e32), (name, e, e32)


# ---------------------------------------------------------------------------------------------
# the reference's fixtures
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modulated', [False, True])
@pytest.mark.parametrize('influence,aggregation', kd.COMBOS)
def test_deformable_kpconv_vs_reference(gpu, influence, aggregation, modulated):
    """fgreg.backbone.DeformableKPConv against the reference's KPConv(deformable=True)
    (kpconv_deform.npz): output and deformed_KP within the forward tests' 1e-4."""
    from fgreg.backbone import DeformableKPConv
    d = golden('kpconv_deform')
    name = f'{influence}.{aggregation}.{int(modulated)}'
    T = lambda k: torch.from_numpy(d[k])
    W = T(f'W.{name}')
    conv = DeformableKPConv(15, 3, W.shape[1], W.shape[2], KP_extent=float(d['extent']),
                            radius=float(d['radius']), KP_influence=influence,
                            aggregation_mode=aggregation, modulated=modulated)
    conv.load_state_dict({'weights': W, 'kernel_points': T('kp'), 'offset_bias': T(f'offset_bias.{name}'),
                          'offset_conv.weights': T(f'offset_W.{name}'),
                          'offset_conv.kernel_points': T('offset_kp')}, strict=True)
    conv = conv.to(gpu)
    with torch.no_grad():
        out = conv(T('q').to(gpu), T('s').to(gpu), T('idx').long().to(gpu), T('x').to(gpu))
    e, ek = rel_err(out, d[f'out.{name}']), rel_err(conv.deformed_KP, d[f'deformed_KP.{name}'])
    print(f'deformable kpconv module {name}: out {e:.3g} deformed_KP {ek:.3g}')
    assert e < TOL and ek < TOL
    assert tuple(conv.offset_features.shape) == (300, (4 if modulated else 3) * 15)


def test_offsets_do_not_depend_on_the_precision_mode(gpu):
    """The offset conv's weight product and deform_points run in the fp32-accurate f16x3 mode in
    the bf16 precision mode too: deformed_KP, offset_features and nnorm are bit-equal between
    the modes (a bf16 offset would move neighbours across the in-range boundary)."""
    import fgreg.linear as lin
    from fgreg.backbone import DeformableKPConv
    d = golden('kpconv_deform')
    name = 'linear.sum.1'
    T = lambda k: torch.from_numpy(d[k])
    conv = DeformableKPConv(15, 3, 16, 24, KP_extent=float(d['extent']), radius=float(d['radius']),
                            modulated=True)
    conv.load_state_dict({'weights': T(f'W.{name}'), 'kernel_points': T('kp'),
                          'offset_bias': T(f'offset_bias.{name}'),
                          'offset_conv.weights': T(f'offset_W.{name}'),
                          'offset_conv.kernel_points': T('offset_kp')}, strict=True)
    conv = conv.to(gpu)
    args = (T('q').to(gpu), T('s').to(gpu), T('idx').long().to(gpu), T('x').to(gpu))
    got = {}
    for mode in ('f16x3', 'bf16'):
        with torch.no_grad(), lin.mode_scope(mode):
            out, nnorm = conv.forward_unnormalized(*args)
        got[mode] = (conv.deformed_KP.clone(), conv.offset_features.clone(), nnorm.clone(), out)
    for a, b in zip(got['f16x3'][:3], got['bf16'][:3]):
        assert torch.equal(a, b)
    assert not torch.equal(got['f16x3'][3], got['bf16'][3])      # the outer product does follow the mode


def _batch(src, tgt, dev):
    return {'src_xyz': [torch.from_numpy(np.asarray(s)).to(dev) for s in src],
            'tgt_xyz': [torch.from_numpy(np.asarray(t)).to(dev) for t in tgt]}


def _fixture_model(name, gpu, fixed=True, mode='ball_query', **over):
    import fgreg
    import fgreg.config as fc
    cfg, sd, src, tgt, meta, d = forward_fixture(name)
    if over:
        cfg = fc.get('modelnet', **dict(ast.literal_eval(str(d['cfg_overrides'])), **over))
    model = fgreg.RegTR(cfg, neighbor_mode=mode)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert all(k.startswith('feature_criterion') for k in missing)
    assert bool(over) or not unexpected
    model = model.to(gpu).eval()
    if fixed:
        model.preprocessor = fgreg.FixedMetaPreprocessor(
            {k: [t.to(gpu) for t in v] for k, v in meta.items()})
    return model, src, tgt, meta, d


FIXTURES = ['forward_modelnet_deform', 'forward_modelnet_deform_mod']


@pytest.mark.parametrize('name', FIXTURES)
def test_forward_on_reference_meta(gpu, name):
    """Three calls in a row: eager, the capturing second sighting, a graph replay."""
    model, src, tgt, _, d = _fixture_model(name, gpu)
    for call in range(3):
        out = model(_batch(src, tgt, gpu))
        for k in KEYS:
            for b in range(len(src)):
                e = rel_err(out[k][b], d[f'out.{k}.{b}'])
                assert e < TOL, (call, k, b, e)
        pose = float(np.abs(out['pose'].cpu().numpy() - d['out.pose']).max())
        assert pose < TOL, (call, pose)


@pytest.mark.parametrize('name', FIXTURES)
def test_rigid_blocks_fail_the_fixtures(gpu, name):
    """The same weights with the `deformable` suffix stripped from the architecture (the offset
    parameters left unused) miss the bound."""
    rigid = ['simple', 'resnetb', 'resnetb', 'resnetb_strided', 'resnetb', 'resnetb']
    model, src, tgt, _, d = _fixture_model(name, gpu, architecture=rigid)
    out = model(_batch(src, tgt, gpu))
    assert min(rel_err(out['src_feat'][b], d[f'out.src_feat.{b}']) for b in range(len(src))) > TOL


class _FixtureEdits(torch.nn.Module):
    """PreprocessorHIP whose tables are checked against the fixture's and then given the
    generator's boundary edits. The fixture's tables are the reference preprocessor's with a few
    entries (at most 0.1 % of a table's, asserted) turned into shadows where the reference's fp64
    run found them within 1e-4 of the in-range boundary (make_golden_deform.py); which entries,
    only the fixture knows. Level 0 must be equal entry for entry. The coarse points are equal as
    a set (row permutation p, test_gpu_forward._match), so the level-1 rows are compared as sets
    through p; an entry the fixture lacks is made a shadow, anything else fails."""

    def __init__(self, inner, ref):
        super().__init__()
        self.inner, self.ref, self.edits = inner, ref, 0

    def _align(self, mine, want, shadow):
        """mine, want (rows, H) CPU tables over the same supports: equal row sets, except entries
        of ``mine`` that ``want`` lacks -> the mask of those entries."""
        assert mine.shape == want.shape
        drop = torch.zeros_like(mine, dtype=torch.bool)
        same = (torch.sort(mine, 1).values == torch.sort(want, 1).values).all(1)
        for i in torch.nonzero(~same).flatten().tolist():
            m, w = set(mine[i].tolist()) - {shadow}, set(want[i].tolist()) - {shadow}
            assert w <= m and len(m) - len(w) == int((want[i] == shadow).sum() - (mine[i] == shadow).sum()), i
            drop[i] = torch.isin(mine[i], torch.tensor(sorted(m - w)))
        assert int(drop.sum()) <= 1e-3 * int((mine != shadow).sum())
        return drop

    def forward(self, pts):
        from scipy.spatial import cKDTree
        meta, ref = self.inner(pts), self.ref
        assert torch.equal(meta['points'][0].cpu(), ref['points'][0])
        assert torch.equal(meta['neighbors'][0].cpu(), ref['neighbors'][0])
        a1, r1 = meta['points'][1].cpu(), ref['points'][1]
        dist, p = cKDTree(a1.numpy()).query(r1.numpy())
        assert dist.max() == 0.0 and len(np.unique(p)) == len(p) == len(a1)
        p = torch.from_numpy(p)
        n0, n1 = ref['points'][0].shape[0], len(p)
        pmap = torch.cat([p, torch.tensor([n1])])               # reference coarse index -> mine
        pools = meta['pools'][0].cpu()
        drop = self._align(pools[p], ref['pools'][0], n0)
        pools[p[torch.nonzero(drop)[:, 0]], torch.nonzero(drop)[:, 1]] = n0
        nb1 = meta['neighbors'][1].cpu()
        drop1 = self._align(nb1[p], pmap[ref['neighbors'][1]], n1)
        nb1[p[torch.nonzero(drop1)[:, 0]], torch.nonzero(drop1)[:, 1]] = n1
        up = meta['upsamples'][0].cpu()
        assert not bool(self._align(up, pmap[ref['upsamples'][0]], n1).any())
        self.edits = int(drop.sum() + drop1.sum())
        meta['pools'][0].copy_(pools)
        meta['neighbors'][1].copy_(nb1)
        return meta


@pytest.mark.parametrize('name', FIXTURES)
def test_forward_end_to_end_nanoflann_mode(gpu, name):
    """The full forward through PreprocessorHIP(neighbor_mode='nanoflann'): every table of the
    fixture reproduced (level 0 entry for entry; the pool, level-1 and upsample tables, which are
    searched with the deformable radius by the radius rule, as row sets) up to the generator's
    boundary edits, and the outputs within TOL: test_gpu_forward's
    test_forward_end_to_end_nanoflann_mode comparison."""
    from scipy.spatial import cKDTree
    model, src, tgt, meta, d = _fixture_model(name, gpu, fixed=False, mode='nanoflann')
    model.preprocessor = _FixtureEdits(model.preprocessor, meta)
    out = model(_batch(src, tgt, gpu))
    print(f'{name}: {model.preprocessor.edits} boundary edits of the fixture applied')
    for b in range(len(src)):
        for side in ('src', 'tgt'):
            a = out[f'{side}_kp'][b].cpu().numpy()
            dist, p = cKDTree(a).query(d[f'out.{side}_kp.{b}'])
            assert dist.max() == 0.0 and len(np.unique(p)) == len(p)
            for k in ('feat', 'kp_warped', 'overlap'):
                assert rel_err(out[f'{side}_{k}'][b][:, p], d[f'out.{side}_{k}.{b}']) < TOL, (side, k, b)
    assert np.abs(out['pose'].cpu().numpy() - d['out.pose']).max() < TOL


def test_ball_query_preprocessor_applies_the_radius_rule(gpu):
    """neighbor_mode='ball_query' searches the same radii: in every row that the limit does not
    cap, the same neighbour set as the nanoflann table (which the test above holds against the
    reference's)."""
    import fgreg
    cfg, _, src, tgt, _, _ = forward_fixture('forward_modelnet_deform')
    pts = [torch.from_numpy(np.asarray(c)).to(gpu) for c in list(src) + list(tgt)]
    got = {m: fgreg.backbone.PreprocessorHIP(cfg, neighbor_mode=m)(pts) for m in ('ball_query', 'nanoflann')}
    for m in got.values():
        assert torch.equal(m['points'][1], got['nanoflann']['points'][1])
    for key, lvl, sup in (('neighbors', 0, 0), ('pools', 0, 0), ('neighbors', 1, 1), ('upsamples', 0, 1)):
        a, b = got['ball_query'][key][lvl].cpu(), got['nanoflann'][key][lvl].cpu()
        ns, limit = got['nanoflann']['points'][sup].shape[0], cfg.neighborhood_limits[lvl]
        assert a.shape[1] == limit and b.shape[1] <= limit
        free = (b == ns).any(1) if b.shape[1] == limit else torch.ones(b.shape[0], dtype=torch.bool)
        sa, sb = torch.sort(a[free], 1).values, torch.sort(b[free], 1).values
        w = b.shape[1]
        assert int(free.sum()) > 10 and torch.equal(sa[:, :w], sb) and bool((sa[:, w:] == ns).all()), (key, lvl)


def test_pipeline_equals_model(gpu):
    """fgreg.pipeline on a deformable, modulated model: exactly model(batch) for every batch."""
    import fgreg
    from fgreg.synthetic import make_batch
    torch.manual_seed(0)
    np.random.seed(0)
    arch = ['simple', 'resnetb', 'resnetb_deformable', 'resnetb_deformable_strided',
            'resnetb_deformable', 'resnetb']
    cfg = fgreg.config.get('modelnet', architecture=arch, modulated=True, first_feats_dim=128,
                           d_embed=64, d_feedforward=128, num_encoder_layers=2, overlap_loss_on=[1],
                           feature_loss_on=[1], corr_loss_on=[1])
    model = fgreg.RegTR(cfg)
    with torch.no_grad():                              # offsets that move the kernel points
        for m in model.modules():
            if isinstance(m, fgreg.backbone.DeformableKPConv):
                m.offset_bias.normal_(0.0, 0.3)
    model = model.to(gpu).eval()
    batches = []
    for start in (0, 5) * 3:
        src, tgt, _ = make_batch('modelnet', 2, start=start)
        batches.append({'src_xyz': [torch.from_numpy(a).to(gpu) for a in src],
                        'tgt_xyz': [torch.from_numpy(a).to(gpu) for a in tgt]})
    with torch.no_grad():
        ref = [model(dict(b)) for b in batches]
    got = list(fgreg.pipeline(model, [dict(b) for b in batches], depth=2, streams=2))
    torch.cuda.synchronize()
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert torch.equal(a['pose'], b['pose'])
        for k in ('src_feat', 'tgt_feat', 'src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap'):
            for u, v in zip(a[k], b[k]):
                assert torch.equal(u, v), k


def _train_step(gpu):
    """fgreg's training step on the deformable model and the loss inputs of loss_modelnet_small
    -> (losses, {parameter: gradient}, the reference's npz)."""
    import fgreg
    import loss_oracle as lo
    from named_weights import named_state_dict
    cfg, _, src, tgt, meta, fwd = forward_fixture('forward_modelnet_deform')
    _, _, batch, _, _, _, W, W_un = loss_fixture()
    ref = golden('train_modelnet_deform')
    raw = fwd['sd_keys'].item()
    keys = ast.literal_eval(raw.decode() if isinstance(raw, bytes) else str(raw))
    stored = {k[3:]: ref[k] for k in ref.files if k.startswith('sd.')}
    assert len(stored) >= 9 and all('kernel_points' in k for k in stored)
    sd = {k: torch.from_numpy(np.array(v)) for k, v in
          named_state_dict(keys, int(ref['sd_seed']), float(fwd['bias']), stored).items()}
    model = fgreg.RegTR(cfg)
    model.load_state_dict(sd, strict=False)
    model = model.to(gpu).train()
    meta_dev = {k: [t.to(gpu) for t in v] for k, v in meta.items()}
    model.preprocessor = fgreg.FixedMetaPreprocessor(meta_dev)
    pred = model(_batch(src, tgt, gpu))
    host = {k: ([t.cpu().double() for t in v] if isinstance(v, list) else v.cpu().double())
            for k, v in pred.items()}
    Wg = W.detach().cpu().double().requires_grad_(True)
    Wug = W_un.detach().cpu().double().requires_grad_(True)
    cv = lambda t: t.cpu().double() if t.is_floating_point() else t.cpu()      # noqa: E731
    b = {'pose': cv(batch['pose']),
         'kpconv_meta': {k: [cv(t) for t in v] for k, v in meta.items()},
         'src_overlap': [cv(t) for t in batch['src_overlap']],
         'tgt_overlap': [cv(t) for t in batch['tgt_overlap']]}
    losses, _ = lo.compute_loss(cfg, Wg, Wug, host, b)
    losses['total'].backward()
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    grads['feature_criterion.W'] = Wg.grad
    grads['feature_criterion_un.W'] = Wug.grad
    return {k: float(v.detach()) for k, v in losses.items()}, grads, ref


@pytest.mark.parametrize('pre', ['', 'f64.'])
def test_train_step_vs_reference(gpu, pre):
    """The reference's train() step on the deformable model (train_modelnet_deform.npz, the
    recipe of make_golden_kpconv_modes.make_train, fixture seed by its rule) in fp32 and with its
    modules in fp64, vs fgreg's: test_gpu_kpconv_modes._check_train_step's checks (losses within
    1e-5, every gradient norm and every stored full gradient, the offset parameters' among them,
    within 1e-2)."""
    from test_gpu_kpconv_modes import _check_train_step
    losses, grads, ref = _train_step(gpu)
    assert sum('.offset_' in k for k in grads) == 6
    assert any('offset_conv.weights' in k[len(pre) + 5:] for k in ref.files if k.startswith(pre + 'grad.'))
    _check_train_step(losses, grads, ref, pre, f'deformable vs the reference ({pre or "fp32"})')
