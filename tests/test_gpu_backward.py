"""Every backward entry point outside attention (csrc/train.hip, csrc/wgrad.hip and the two GEMM
modes as fgreg/autograd.py drives them) per element against the same operation in plain fp64 on
the CPU. It follows test_gpu_dispatch.py, whose helpers it imports; the restatements live in
tests/_backward_ref.py (checked on the CPU by test_backward_ref.py).

Error and bounds. Per element, condition-aware: |got - ref64| / sum|terms| of that element
(_cond_err); an element without terms must be an exact 0. Every case prints the kernel's error,
the torch fp32 restatement's error and the bound before it asserts ("backward-error ...").
  fp32 kernels (LayerNorm, scatter, max-pool sums)   _hold: <= 4 x the fp32 restatement's error
              + 1e-7, never above CAP = 1e-4.
              Measured (largest kernel / restatement error; largest kernel / bound of a case):
              LayerNorm dx 2.3e-7 / 2.1e-7, 0.32; dgamma 1.8e-7 / 2.6e-7, 0.30; dbeta 1.1e-7 /
              1.5e-7, 0.23; scatter linear / sum 2.3e-6 / 4.0e-6, 0.43, the other five pairs
              <= 1.2e-6 / 1.2e-6, 0.30; kpconv_t dx 1.2e-6 / 1.4e-6, 0.22; max-pool 1.2e-7 /
              1.2e-7, 0.21.
  colsum, db  fp64 partials, one fp32 rounding of the result: <= 1.5 * 2^-24 = 8.9e-8 of sum|x|
              (the bias gradient is summed in fp64 in both modes: fgr_colsum in bf16, the wgrad
              kernel's own column sums in f16x3). Measured: colsum 1.2e-8, db 1.8e-8 (the torch
              fp32 sum: 4.2e-8).
  bf16 GEMMs  against the fp64 product of the SAME bf16-rounded operands (the rounding-point
              contract of DESIGN.md "bf16 mode"): (ceil(K / 32) + 8) * 2^-24, the worst case of
              an fp32 accumulation in k-steps of 32, never above 1e-5 (5.4e-7 at K <= 32 ..
              4.4e-6 at K = 2056). A doubly rounded or truncated operand costs ~2^-9, a dropped
              K tail ~1/K. Measured: y 9.8e-8, dx 1.2e-7, dW 1.3e-7 (wgrad alone 1.1e-7), kpconv
              out / d_wf / dW 9.0e-8 / 8.4e-8 / 8.8e-8; at most 0.20 of the bound; torch's fp32
              product of the same operands: 7e-8 .. 1.8e-7. Also normwise 1e-2 against the exact
              fp64 product (measured <= 3.9e-3, at K = 1).
  f16x3 GEMMs against exact fp64: 3 * 2^-22 (the per-product bound of fgreg/linear.py) +
              (ceil(K / 32) + 8) * 2^-24 (1.25e-6 at K <= 32 .. 5.1e-6 at K = 2056). Measured:
              y 1.6e-7, dx 4.6e-7, dW 2.0e-7, kpconv out / d_wf / dW 3.2e-7 / 1.8e-7 / 2.3e-7; at
              most 0.37 of the bound.
  integer outputs and gradient routing               exact.

sum|terms| per family
  y            |x| |W|^T + |b| (+ |residual|)
  dx (linear)  |dY| |W|                      dW   |dY|^T |X|            db   sum_r |dY|
  LayerNorm    dx: rstd (|dxh| + mean|dxh| + |xh| mean|dxh xh|), dxh = dy gamma;
               dgamma: sum_r |dy xh|; dbeta: sum_r |dy|
  scatter dx   sum_entries sum_k w |d_wf| (the restatement's autograd on |d_wf|: w >= 0); for
               gaussian plus entries * n_kp * 2^-126 max|d_wf| (weights a kernel may flush)
  max-pool dx  sum |dy| over the (query, channel) pairs routed to the element
  colsum       sum_r |x|
The ReLU mask of every reference is taken from the kernel's own y (a bf16 y differs from fp64
by ~1e-2 relative, so elements near the kink would flip otherwise).

bf16 GEMM dispatch restated (csrc/bf16.hip; _backward_ref.bf16_branch, asserted per case):
  bf16_tile(m, n, k): k % 8 == 0 and splitk_shape -> 'X' (k >= 2048) or 'S'; else <= 400 tiles
  of 64 x 64, k >= 512, n >= 32 -> 'S' (k >= 2048 or n <= 64), 'T' or 'W'; else m <= 4096 and
  k >= 2048 -> 'W'; else 'X' (n <= 256, k >= 1000) or 'z'. splitk_shape: k >= 1920, n <= 256,
  <= 160 tiles. bf16_ksplit: splitk_shape ? (k >= 2048 ? 4 : 2) : 1. Any letter with k % 8 != 0
  runs the register-staged gemm_bf16_kernel<64, n >= 128 ? 128 : 64, false>.

Entry point -> branch -> arguments that select it -> test
  linear_t backward, bf16 mode (fgr_gemm_bf16_ws; dW GEMM is (M = n, N = k, K = rows))
    dW 'X', 4 parts          (rows, n, k) = (2048, 64, 128)     test_linear_bf16[2048-64-128-*]
    dW 'S', 2 parts          (1928, 64, 128)                    test_linear_bf16[1928-64-128-*]
    dW <64,128,false>        (2051, 64, 128): K % 8, lda % 4 != 0   test_linear_bf16[2051-64-128-*]
    dW <64,64,false>         (2052, 64, 64): K % 8 != 0, lda % 4 == 0   test_linear_bf16[2052-64-64-*]
    dW 'S', 1 part           (2056, 256, 1024): wide N          test_linear_bf16[2056-256-1024-*]
    dW <64,64 / 128,false>   (37, 3, 32), (300, 1, 256)         test_linear_bf16[37-3-32-*], [300-1-256-*]
    dX <64,64 / 128,true>    K = n = 64 / 256 (transposed image)    the five cases above
    dX scalar, K = 3 / 1     (37, 3, 32), (300, 1, 256)         test_linear_bf16[37-3-32-*], [300-1-256-*]
  wgrad(), bf16 mode: strided views, bias_grad, rerun bit-identical, rows == 0
                                                                test_wgrad_bf16[*]
  kpconv_t, bf16 mode: out, d_wf ('flat' image, K = cout), dW (K = nq = 70: <.., false>), dx
                                                                test_kpconv_bf16[1], [16], [64]
  linear_t backward, f16x3 mode ('bwd_dx' image; fgr_gemm_f16x3_wgrad, padded at n = 3 / 1)
                                                                test_linear_f16x3[*]
  kpconv_t, f16x3 mode ('flat' image, wgrad with m = 15 padded)  test_kpconv_f16x3[1], [16], [64]
  fgr_layernorm_bwd (n in 0, 1, 15, 16, 17, 333: empty, one row, a last block of 15 / 1 rows)
    PER 1    d 32 (half filled), 64         test_layernorm_bwd[32], [64]
    PER 2    d 65, 96, 128                  test_layernorm_bwd[65], [96], [128]
    PER 4    d 200, 256                     test_layernorm_bwd[200], [256]
    PER 8    d 300, 512                     test_layernorm_bwd[300], [512]
    PER 16   d 513, 576, 1000, 1024         test_layernorm_bwd[513], [576], [1000], [1024]
    refused  d 1025                         test_layernorm_bwd_refuses_wide
  fgr_colsum: n 0, 1, 255, 256, 257, 1000 (kColRows = 256 border), ldx = c and c + 5
                                                                test_colsum[1], [63], [64], [65], [257]
  fgr_nbr_inverse
    rank loop, 44 trips      (nq 70, width 40, ns 1)            test_nbr_inverse_tables[one-row]
    rank loop, 4 trips       (300, 5, 7): > 200 entries a row   test_nbr_inverse_tables[seven-rows]
    scan, 1 / 2 / 5 rows per thread  ns 1023, 1024, 1025, 4097  test_nbr_inverse_tables[ns1023] ..
    non-entries              shadow, negative, > ns             test_nbr_inverse_tables[bad-indices]
    empty                    nq 0, width 0, ns 0                test_nbr_inverse_tables[nq0], [width0], [ns0]
  fgr_max_pool_bwd: c 1, 48, 64, 257 x width 1, 5, 40, every tie of "first maximum, shadows
    read 0" (_backward_ref.pool_case)                           test_max_pool_bwd[*]
  fgr_kpconv_scatter_mode
    dw[32] registers         n_kp 15, 17, 32 x cin 1, 12, 64, 130 x H 7, 70 (linear / sum)
                                                                test_scatter[*]
    <INF, AGG>               all six pairs at cin 12, n_kp 15, H 70   test_scatter_modes[*]

Defect found: wgrad() in bf16 mode with rows == 0 asked fgr_split_weights_bf16_bytes(n, 0) for
an image and raised; it now returns zeros like the f16x3 entry point (test_wgrad_bf16[0-64-32]).
"""
import math

import numpy as np
import pytest
import torch

import _backward_ref as br
import _kpconv_modes as km
from _arena import SENTINEL, Arena, bit_equal, run_both
from conftest import rel_err
from test_gpu_dispatch import CAP, _L, _cond_err, _hold, _ok, _p, _st

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32
COLSUM_BOUND = 1.5 * br.U


def _report(what, e, e32, bound):
    print(f'backward-error {what}: kernel {e:.3e} fp32-restatement {e32:.3e} bound {bound:.3e}')


def _within(what, e, e32, bound):
    """A fixed bound (GEMM modes, colsum): print, then assert."""
    _report(what, e, e32, bound)
    assert e <= bound, (what, e, bound)


def _fp32(what, e, e32):
    """The fp32 kernels' bound (_hold), with the bound printed too."""
    _report(what, e, e32, min(4 * e32 + 1e-7, CAP))
    _hold(what, e, e32, CAP)


@pytest.fixture
def bf16_mode(monkeypatch):
    import fgreg
    monkeypatch.delenv('FGR_GEMM_BF16_TILE', raising=False)      # the default dispatch
    monkeypatch.delenv('FGR_GEMM_KSPLIT', raising=False)
    old = fgreg.precision()
    fgreg.set_precision('bf16')
    yield
    fgreg.set_precision(old)


@pytest.fixture
def f16x3_mode():
    import fgreg
    old = fgreg.precision()
    fgreg.set_precision('fp32')              # the fp32-accurate mode: linear.MODE 'f16x3'
    from fgreg import linear as lin
    assert lin.MODE == 'f16x3'
    yield
    fgreg.set_precision(old)


# ---------------------------------------------------------------------------------------------
# 1, 2. linear_t, wgrad and kpconv_t in both GEMM modes
# ---------------------------------------------------------------------------------------------
# (rows, n, k) -> the dW GEMM's (kernel, split-K parts) in bf16 mode (module docstring)
LIN_SHAPES = {(2048, 64, 128): ('X', 4), (1928, 64, 128): ('S', 2),
              (2051, 64, 128): ('z128scalar', 1), (2052, 64, 64): ('z64scalar', 1),
              (2056, 256, 1024): ('S', 1), (37, 3, 32): ('z64scalar', 1),
              (300, 1, 256): ('z128scalar', 1)}
LIN_CASES = [s + (a,) for s in LIN_SHAPES for a in ('none', 'relu')] + [(2051, 64, 128, 'residual')]


def _mode_parts(mode):
    """(operand rounding, bound(K), restatement) of a GEMM mode."""
    if mode == 'bf16':
        return br.bf, br.bf16_bound
    return (lambda t: t.detach().cpu().double()), br.f16x3_bound


def _gemm_check(what, mode, got, A, B, K, extra=None, extra_den=None, relu=False):
    """got against A @ B (fp64 operands, already rounded for bf16) (+ extra), per element."""
    _, bound = _mode_parts(mode)
    ref, den = A @ B, A.abs() @ B.abs()
    r32 = A.float() @ B.float()
    if extra is not None:
        ref, den, r32 = ref + extra, den + extra_den, r32 + extra.float()
    if relu:
        ref, r32 = ref.clamp_min(0), r32.clamp_min(0)
    _within(what, _cond_err(got, ref, den), _cond_err(r32, ref, den), bound(K))


def _linear_case(gpu, mode, rows, n, k, act):
    from fgreg import ops
    from fgreg.autograd import linear_t
    op, _ = _mode_parts(mode)
    g = torch.Generator().manual_seed(rows + n + k)
    x0 = torch.randn(rows, k, generator=g)
    w0 = torch.randn(n, k, generator=g) / math.sqrt(k)
    b0 = torch.randn(n, generator=g)
    r0 = torch.randn(rows, n, generator=g)
    R = torch.randn(rows, n, generator=g)
    x, w, b, r = (t.clone().to(gpu).requires_grad_(True) for t in (x0, w0, b0, r0))
    if act == 'relu':
        y = linear_t(x, w, b, act=ops.ACT_RELU)
    elif act == 'residual':
        y = linear_t(x, w, b, residual=r)
    else:
        y = linear_t(x, w, b)
    (y * R.to(gpu)).sum().backward()
    what = f'linear {mode} ({rows}, {n}, {k}) {act}'
    X, W = op(x0), op(w0)
    extra, eden = b0.double().expand(rows, n), b0.double().abs().expand(rows, n)
    if act == 'residual':
        extra, eden = extra + r0.double(), eden + r0.double().abs()
    _gemm_check(what + ' y', mode, y, X, W.t(), k, extra, eden, relu=act == 'relu')
    dy = R * (y.detach().cpu() > 0) if act == 'relu' else R          # the kernel's own mask
    if act == 'relu':
        assert 0.2 < float((dy != 0).float().mean()) < 0.8
    DY = op(dy)
    _gemm_check(what + ' dx', mode, x.grad, DY, W, n)
    _gemm_check(what + ' dw', mode, w.grad, DY.t(), X, rows)
    db64, dbden = dy.double().sum(0), dy.double().abs().sum(0)
    _within(what + ' db', _cond_err(b.grad, db64, dbden), _cond_err(dy.sum(0), db64, dbden),
            COLSUM_BOUND)
    if act == 'residual':
        assert torch.equal(r.grad.cpu(), R)
    if mode == 'bf16':                       # and the exact product at the bf16 level, normwise
        x64, w64, dy64 = x0.double(), w0.double(), dy.double()
        y64 = x64 @ w64.t() + extra
        for name, got, want in (('y', y, y64.clamp_min(0) if act == 'relu' else y64),
                                ('dx', x.grad, dy64 @ w64), ('dw', w.grad, dy64.t() @ x64)):
            e = rel_err(got, want)
            print(f'backward-error {what} {name} vs exact fp64, normwise: {e:.3e} bound 1.000e-02')
            assert e < 1e-2, (what, name, e)


@pytest.mark.parametrize('rows,n,k,act', LIN_CASES)
def test_linear_bf16(gpu, bf16_mode, rows, n, k, act):
    """linear_t forward and backward in bf16 mode at each branch of the dW GEMM (K = rows: split-K
    'X' / 'S', the scalar kernel for K % 8 != 0 at both tile widths, the wide unsplit 'S') and
    of the dX GEMM on the transposed image (K = n, down to 3 and 1)."""
    assert br.bf16_branch(n, k, rows) == LIN_SHAPES[(rows, n, k)]
    assert br.bf16_branch(rows, k, n)[0] == ('z128' if k >= 128 else 'z64') + ('' if n % 8 == 0 else 'scalar')
    _linear_case(gpu, 'bf16', rows, n, k, act)


@pytest.mark.parametrize('rows,n,k,act', LIN_CASES)
def test_linear_f16x3(gpu, f16x3_mode, rows, n, k, act):
    """The same shapes in f16x3 mode against exact fp64: the 'bwd_dx' image and
    fgr_gemm_f16x3_wgrad (its m % 4 / n % 4 padding path at n = 3 and n = 1)."""
    _linear_case(gpu, 'f16x3', rows, n, k, act)


@pytest.mark.parametrize('rows,m,n', [(0, 64, 32), (37, 12, 20), (1928, 20, 132), (2048, 64, 128),
                                      (2051, 64, 128)])
def test_wgrad_bf16(gpu, bf16_mode, rows, m, n):
    """wgrad() alone in bf16 mode on views into wider buffers (ld > cols), with and without
    bias_grad, bit-identical on a rerun; rows == 0 gives zeros of shape (m, n) and (m,)."""
    from fgreg import autograd as ag
    g = torch.Generator().manual_seed(rows + m + n)
    a, b = torch.randn(rows, m, generator=g), torch.randn(rows, n, generator=g)
    ab, bb = torch.zeros(rows, m + 12, device=gpu), torch.zeros(rows, n + 8, device=gpu)
    ab[:, 8:8 + m] = a.to(gpu)
    bb[:, 4:4 + n] = b.to(gpu)
    ad, bd = ab[:, 8:8 + m], bb[:, 4:4 + n]
    got = ag.wgrad(ad, bd)
    got2, db = ag.wgrad(ad, bd, bias_grad=True)
    assert got.shape == (m, n) and db.shape == (m,)
    assert bit_equal(got, ag.wgrad(ad, bd)) and bit_equal(got, got2)
    assert bit_equal(db, ag.wgrad(ad, bd, bias_grad=True)[1])
    if rows == 0:
        assert bool((got == 0).all()) and bool((db == 0).all())
        return
    what = f'wgrad bf16 ({rows}, {m}, {n})'
    _gemm_check(what + ' dw', 'bf16', got, br.bf(a).t(), br.bf(b), rows)
    db64, den = a.double().sum(0), a.double().abs().sum(0)
    _within(what + ' db', _cond_err(db, db64, den), _cond_err(a.sum(0), db64, den), COLSUM_BOUND)
    assert rel_err(got, a.double().t() @ b.double()) < 1e-2


def _scatter_check(what, got, q, s, idx, kp, dwf, cin, influence, aggregation):
    """dx of the scatter per element against fp64 autograd of the restatement, _hold."""
    args = (q, s, idx, kp, dwf, cin, influence, aggregation)
    ref = br.scatter(*args, torch.float64)
    den = br.scatter(*args, torch.float64, absolute=True)
    if influence == 'gaussian':
        ns = s.shape[0]
        cnt = torch.bincount(idx[idx < ns].reshape(-1), minlength=ns).double()
        den = den + (cnt * kp.shape[0] * 2.0 ** -126 * float(dwf.abs().max())).unsqueeze(1)
    assert int((den > 0).sum()) > 10                            # the case has live elements
    _fp32(what, _cond_err(got, ref, den), _cond_err(br.scatter(*args, torch.float32), ref, den))


def _kpconv_case(gpu, mode, cin):
    from fgreg import linear as lin
    from fgreg import ops
    from fgreg.autograd import kpconv_t
    op, _ = _mode_parts(mode)
    n_kp, cout = 15, 24
    q, s, idx, x0, kp, _ = km.table(cin, 70, n_kp)
    nq = q.shape[0]
    g = torch.Generator().manual_seed(cin)
    W0 = torch.randn(n_kp, cin, cout, generator=g) / math.sqrt(n_kp * cin)
    dout = torch.randn(nq, cout, generator=g)

    class Conv:
        pass
    conv = Conv()
    x, W = (t.clone().to(gpu).requires_grad_(True) for t in (x0, W0))
    conv.weights, conv.kernel_points, conv.KP_extent = W, kp.to(gpu), km.EXT
    Q, S, IDX = q.to(gpu), s.to(gpu), idx.to(gpu)
    out, _ = kpconv_t(conv, Q, S, IDX, x)
    (out * dout.to(gpu)).sum().backward()
    what = f'kpconv {mode} cin {cin}'
    # the operands the GEMMs see: the kernel's own fp32 gather (pinned by the gather tests) and
    # the kernel's own d_wf, recomputed by the call the backward makes
    wf = ops.kpconv_gather(Q, S, IDX, x.detach(), conv.kernel_points, km.EXT)[0].reshape(nq, -1)
    dwf = lin.linear(dout.to(gpu), W.detach(), transpose='flat', tag='bwd_dwf',
                     cache=False)
    W2 = op(W0.reshape(n_kp * cin, cout))
    _gemm_check(what + ' out', mode, out, op(wf), W2, n_kp * cin)
    _gemm_check(what + ' d_wf', mode, dwf, op(dout), W2.t(), cout)
    _gemm_check(what + ' dW', mode, W.grad.reshape(n_kp * cin, cout), op(wf).t(), op(dout), nq)
    _scatter_check(what + ' dx', x.grad, q, s, idx, kp, dwf, cin, 'linear', 'sum')
    if mode == 'bf16':
        assert rel_err(W.grad.reshape(n_kp * cin, cout), wf.double().cpu().t() @ dout.double()) < 1e-2
        assert rel_err(dwf, dout.double() @ W0.double().reshape(n_kp * cin, cout).t()) < 1e-2


@pytest.mark.parametrize('cin', [1, 16, 64])
def test_kpconv_bf16(gpu, bf16_mode, cin):
    """kpconv_t in bf16 mode: out, d_wf (the 'flat' image) and dW = wf^T dout (K = 70 queries:
    the scalar kernel) against the rounded-operand product; dx (the scatter stays fp32) with the
    fp32 convention given the kernel's d_wf."""
    _kpconv_case(gpu, 'bf16', cin)


@pytest.mark.parametrize('cin', [1, 16, 64])
def test_kpconv_f16x3(gpu, f16x3_mode, cin):
    """The same in f16x3 mode against exact fp64 (wgrad with m = 15 at cin 1: the padded path)."""
    _kpconv_case(gpu, 'f16x3', cin)


# ---------------------------------------------------------------------------------------------
# 3. fgr_layernorm_bwd
# ---------------------------------------------------------------------------------------------
LN_N = (0, 1, 15, 16, 17, 333)


def _ln_abi(ar, x, gamma, dy, n, d):
    from fgreg import _lib
    nb = _lib.ws_size('fgr_layernorm_bwd_workspace', n, d)
    ws = ar.bytes(nb, name='ws')
    dgb = ar.vector(2 * d, F32, 'out', name='dgamma_dbeta')
    dx = ar.matrix(max(n, 1), d, d, F32, 'out', name='dx', full=n > 0)
    X = ar.put(x, name='x') if n else None
    DY = ar.put(dy, name='dy') if n else None
    rc = _L().fgr_layernorm_bwd(_p(X), n, d, _p(ar.put(gamma, name='gamma')), br.EPS, _p(DY), _p(dx),
                                _p(dgb), _p(ws), nb, _st())
    return rc, dx, dgb


@pytest.mark.parametrize('d', [32, 64, 65, 96, 128, 200, 256, 300, 512, 513, 576, 1000, 1024])
def test_layernorm_bwd(gpu, d):
    """fgr_layernorm_bwd through the C ABI with its exact workspace: every PER with whole and
    partly filled lanes, n = 0 (zero dgamma / dbeta, dx untouched), 1, and last blocks of 15, 1
    and 13 rows; a row of mean 1e3 and a constant row (rstd = eps^-1/2); dx, dgamma, dbeta."""
    g = torch.Generator().manual_seed(d)
    gamma = 1 + 0.2 * torch.randn(d, generator=g)
    for n in LN_N:
        x = br.ln_rows(n, d, 1000 * d + n)
        dy = torch.randn(n, d, generator=g)
        ar = Arena(gpu)
        rc, dx, dgb = _ln_abi(ar, x, gamma, dy, n, d)
        _ok(rc, 'fgr_layernorm_bwd')
        torch.cuda.synchronize()
        ar.check()
        if n == 0:
            assert bool((dgb == 0).all())
            assert bool((dx.view(I32) == SENTINEL).all())
            continue
        ref, den = br.layernorm_bwd(x, gamma, dy, torch.float64)
        r32, _ = br.layernorm_bwd(x, gamma, dy, torch.float32)
        for i, (name, got) in enumerate((('dx', dx), ('dgamma', dgb[:d]), ('dbeta', dgb[d:]))):
            _fp32(f'layernorm_bwd d {d} n {n} {name}', _cond_err(got, ref[i], den[i]),
                  _cond_err(r32[i], ref[i], den[i]))


def test_layernorm_bwd_refuses_wide(gpu):
    """d = 1025 is refused (FGR_E_ARG) with every output sentinel and the workspace in place."""
    n, d = 17, 1025
    g = torch.Generator().manual_seed(d)
    ar = Arena(gpu)
    rc, _, _ = _ln_abi(ar, torch.randn(n, d, generator=g), torch.ones(d), torch.randn(n, d, generator=g), n, d)
    torch.cuda.synchronize()
    assert rc == -1 and '1024' in _L().fgr_last_error().decode()
    for r in ar.regions:
        if r.role == 'out':
            assert bool((r.buf.view(I32) == SENTINEL).all()), r.name
        elif r.role == 'scratch':
            assert bool((r.view == 0).all()), r.name


# ---------------------------------------------------------------------------------------------
# 4. fgr_colsum
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 63, 64, 65, 257])
def test_colsum(gpu, c):
    """fgr_colsum through the C ABI with its exact workspace: no rows, one row, each side of the
    kColRows = 256 border, four parts; dense and padded rows (ldx = c + 5); one, partial and
    several 64-channel blocks. fp64 partials: the error is the fp32 rounding of the result."""
    from fgreg import _lib
    g = torch.Generator().manual_seed(c)
    for n in (0, 1, 255, 256, 257, 1000):
        x = torch.randn(n, c, generator=g) * 10.0 ** torch.empty(c).uniform_(-3, 3, generator=g)
        for ldx in (c, c + 5):
            ar = Arena(gpu)
            nb = _lib.ws_size('fgr_colsum_workspace', n, c)
            ws = ar.bytes(nb, name='ws')
            out = ar.vector(c, F32, 'out', name='out')
            X = ar.put(x, ld=ldx, name='x') if n else None
            _ok(_L().fgr_colsum(_p(X), n, c, ldx, _p(out), _p(ws), nb, _st()), 'fgr_colsum')
            torch.cuda.synchronize()
            ar.check()
            ref, den = x.double().sum(0), x.double().abs().sum(0)
            _within(f'colsum n {n} c {c} ldx {ldx}', _cond_err(out, ref, den),
                    _cond_err(x.sum(0), ref, den), COLSUM_BOUND)


# ---------------------------------------------------------------------------------------------
# 5. fgr_nbr_inverse
# ---------------------------------------------------------------------------------------------
def _sparse_table(ns, nq=200, width=9):
    rng = np.random.default_rng(ns)
    idx = rng.integers(0, ns, (nq, width))
    idx[rng.uniform(size=idx.shape) < 0.5] = ns
    return idx, ns


def _bad_table():
    ns = 50
    rng = np.random.default_rng(50)
    idx = rng.integers(0, ns, (70, 12))
    bad = np.array([ns, -1, -7, ns + 1, ns + 1000, 1 << 40, -(1 << 40)])
    m = rng.uniform(size=idx.shape) < 0.4
    idx[m] = rng.choice(bad, int(m.sum()))
    return idx, ns


NBR_TABLES = {
    'one-row': lambda: (np.zeros((70, 40), np.int64), 1),
    'seven-rows': lambda: (np.random.default_rng(7).permutation(np.arange(1500) % 7).reshape(300, 5), 7),
    'ns1023': lambda: _sparse_table(1023), 'ns1024': lambda: _sparse_table(1024),
    'ns1025': lambda: _sparse_table(1025), 'ns4097': lambda: _sparse_table(4097),
    'bad-indices': _bad_table,
    'nq0': lambda: (np.zeros((0, 5), np.int64), 9), 'width0': lambda: (np.zeros((9, 0), np.int64), 9),
    'ns0': lambda: (np.zeros((6, 4), np.int64), 0),
}


@pytest.mark.parametrize('table', list(NBR_TABLES))
def test_nbr_inverse_tables(gpu, table):
    """fgr_nbr_inverse through the C ABI with its exact workspace, on a clean and a poisoned
    arena, equal to the host's stable inverse: start, ent (and nothing written behind the valid
    entries), pos with -1 for every non-entry."""
    from fgreg import _lib
    idx, ns = NBR_TABLES[table]()
    idx = np.ascontiguousarray(idx, np.int64)
    nq, width = idx.shape
    n_ent = nq * width
    start, ent, pos = br.nbr_inverse_host(idx, ns)
    if table in ('one-row', 'seven-rows'):
        assert int(np.diff(start).min()) > 200                   # the rank loop's later trips
    if table.startswith('ns1') or table == 'ns4097':
        assert int((np.diff(start) == 0).sum()) > 100            # rows that nobody names
    if table == 'bad-indices':
        assert len(ent) < n_ent - 300 and bool((idx < 0).any()) and bool((idx > ns).any())

    def fn(ar):
        nb = _lib._sz(0)
        _ok(_L().fgr_nbr_inverse_workspace(nq, width, ns, nb), 'fgr_nbr_inverse_workspace')
        ws = ar.bytes(nb.value, name='ws')
        S = ar.vector(ns + 1, I32, 'out', name='start')
        P = ar.vector(max(n_ent, 1), I32, 'out', name='pos', full=n_ent > 0)
        E = ar.vector(max(n_ent, 1), I32, 'out', name='ent', full=False)
        IDX = ar.put(torch.from_numpy(idx), name='idx') if n_ent else None
        _ok(_L().fgr_nbr_inverse(_p(IDX), nq, width, ns, _p(S), _p(P), _p(E), _p(ws), nb.value,
                                 _st()), 'fgr_nbr_inverse')
        return S, P, E
    for S, P, E in run_both(fn, gpu):
        S, P, E = (t.cpu().numpy() for t in (S, P, E))
        assert np.array_equal(S, start)
        assert np.array_equal(E[:len(ent)], ent) and bool((E[len(ent):] == SENTINEL).all())
        if n_ent:
            assert np.array_equal(P, pos)
        else:
            assert bool((P == SENTINEL).all())
    print(f'backward-error nbr_inverse {table}: exact ({len(ent)} entries of {n_ent}, {ns} rows, '
          f'longest row {int(np.diff(start).max()) if ns else 0})')


# ---------------------------------------------------------------------------------------------
# 6. fgr_max_pool_bwd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', [1, 5, 40])
@pytest.mark.parametrize('c', [1, 48, 64, 257])
def test_max_pool_bwd(gpu, c, width):
    """fgr_max_pool_bwd through the C ABI on the host's inverse with its exact workspace: the
    gradient goes to the row's FIRST maximum with shadows reading 0 (pool_case: a shadow's zero
    before / after a real 0.0 and -0.0, equal supports, a support named twice, negative
    channels, an all-shadow row); dx is the sum of the routed dy in ascending entry order, and
    an exact 0 where nobody routes."""
    from fgreg import _lib
    x, idx = br.pool_case(c, width)
    ns, (nq, _) = x.shape[0], idx.shape
    dy = np.random.default_rng(c + width).normal(size=(nq, c)).astype(np.float32)
    ref, den, r32, routed = br.max_pool_bwd(x, idx, dy)
    assert 0 < routed < nq * c and bool((den[7] > 0).any() or width == 1)
    start, ent, _ = br.nbr_inverse_host(idx, ns)
    ar = Arena(gpu)
    nb = _lib.ws_size('fgr_max_pool_bwd_workspace', nq, c)
    ws = ar.bytes(nb, name='ws')
    dx = ar.matrix(ns, c, c, F32, 'out', name='dx')
    T = torch.from_numpy
    ent_t = T(ent) if len(ent) else torch.zeros(1, dtype=I32)
    _ok(_L().fgr_max_pool_bwd(_p(ar.put(T(x), name='x')), ns, c, _p(ar.put(T(idx), name='idx')), nq,
                              width, _p(ar.put(T(dy), name='dy')), _p(ar.put(T(start), name='start')),
                              _p(ar.put(ent_t, name='ent')), _p(dx), _p(ws), nb, _st()),
        'fgr_max_pool_bwd')
    torch.cuda.synchronize()
    ar.check()
    assert bool((dx.cpu()[T(den == 0)] == 0).all())
    _fp32(f'max_pool_bwd c {c} width {width}', _cond_err(dx, T(ref), T(den)),
          _cond_err(T(r32), T(ref), T(den)))


# ---------------------------------------------------------------------------------------------
# 7. fgr_kpconv_scatter_mode
# ---------------------------------------------------------------------------------------------
def _scatter_case(gpu, cin, n_kp, H, influence, aggregation):
    from fgreg.autograd import kpconv_scatter
    q, s, idx, _, kp, _ = km.table(cin, H, n_kp)
    dwf = torch.randn(q.shape[0], n_kp * cin, generator=torch.Generator().manual_seed(cin + n_kp + H))
    dx = kpconv_scatter(q.to(gpu), s.to(gpu), idx.to(gpu), dwf.to(gpu), kp.to(gpu), km.EXT,
                        influence, aggregation)
    _scatter_check(f'scatter {influence}/{aggregation} cin {cin} n_kp {n_kp} H {H}', dx, q, s, idx,
                   kp, dwf, cin, influence, aggregation)


@pytest.mark.parametrize('H', [7, 70])
@pytest.mark.parametrize('cin', [1, 12, 64, 130])
@pytest.mark.parametrize('n_kp', [15, 17, 32])
def test_scatter(gpu, n_kp, cin, H):
    """fgr_kpconv_scatter_mode (linear / sum) per element: n_kp 15, 17 (a partly used dw[32])
    and 32 (kMaxKpT); one lane, partial, whole and two-and-a-bit 64-channel slices (cin 130);
    one chunk of 7 and two chunks of 70 neighbours."""
    _scatter_case(gpu, cin, n_kp, H, 'linear', 'sum')


@pytest.mark.parametrize('influence', km.INFLUENCES)
@pytest.mark.parametrize('aggregation', km.AGGREGATIONS)
def test_scatter_modes(gpu, influence, aggregation):
    """All six influence x aggregation instances at cin 12, n_kp 15, H 70."""
    _scatter_case(gpu, 12, 15, 70, influence, aggregation)
