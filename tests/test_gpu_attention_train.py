"""The training attention pair through the C ABI, per element against fp64: fgr_attention_f16x3_
train / _drop (forward, o and lse) and fgr_attention_bwd_train / _drop (dq, dk, dv) on every
kernel route they dispatch to. Reference, denominators, regimes, segmentations and the seeded
cases: tests/_attn_ref.py (pinned on the CPU by test_attn_ref.py).

Every case: operands in a guarded Arena (tests/_arena.py) with row stride d + 4, outputs of role
'out', the lse a guarded vector, the workspace exactly the bytes the matching _workspace call
returns; run on a clean and on a poisoned arena (run_both): sentinels and pad columns intact,
both outputs bit-identical. nhead 2 (7 segments x 2 heads = 14 is no multiple of the 8-way
block swizzle). The backward takes o and lse2 from the fp64 reference rounded once to fp32, so
it is judged on its own.

Routes
  F1  fgr_attention_f16x3_train, p = 0    dh 32 / 64   attn_f16x3_v2_kernel<DH, false> + lse
  F2  the same, p > 0                     dh 32 / 64   <DH, true> + lse (of the undropped softmax)
  F3  fgr_attention_f16x3_drop            dh 32 / 64   <DH, true>
  R1  fgr_attention_bwd_train, ws of _train_workspace, p = 0   dh 32 / 64   f16x3 <DH, false>
  R2  the same, p > 0                                          dh 32 / 64   f16x3 <DH, true>
  R3  fgr_attention_bwd_train, ws of fgr_attention_bwd_workspace bytes, p = 0
                                          dh 16 / 32 / 64   attn_bwd_*_mfma_kernel<DH> with lse_in
  R4  the same, p > 0                     dh 16 / 32 / 64   <DH, true> with lse_in
  R5  fgr_attention_bwd_drop (no lse)     dh 16 / 32 / 64   <DH, true> with its own pass 1
  R6  fgr_attention_bwd_train, p = 0, dh 8, and dh 32 with ld = d + 1 and operands 4 B off a
      16-B boundary                       the scalar attn_bwd_dq / dkdv_kernel (lse recomputed)
  refused  p > 0 at dh 8 and at dh 32 misaligned, _train and _drop: non-zero code, the reason
      in fgr_last_error, every output sentinel in place.

Error and bound. Per element |got - ref64| / sum|terms| (_attn_ref.cond_err); an element with
denominator 0 must be exactly 0. The bound is never taken from the kernel's own error:
  R3 - R6 (exact fp32 products)   err <= 4 x e32 + 1e-7, e32 the fp32 restatement's error on the
                                  same inputs (the rule of test_gpu_dispatch.py);
  F1 - F3, R1, R2 (f16x3)         the same 4 x e32 + 1e-7 (test_attention_split_is_fp32_accurate);
                                  the header of attention16.hip derives 3 x 2^-22 per product
                                  against fp32's 2^-24, which would allow 12 x e32 + 1e-7 in a
                                  peaked or blocks case; none needs it (largest ratio 1.7);
  unit cases                      also never above 1e-5 (the attention family's cap; in peaked
                                  the reference alone reaches 4e-6, so the cap binds unit only);
  lse                             |got - ref| <= 4 x (restatement's error) + one fp32 ulp of the
                                  case's largest |lse2|.

test_backward_reads_the_forward_lse hands R1 - R4 lse2 + 1: P, dS and the three gradients
must come out halved, which only a kernel that takes P from the lse it is given does.

Measured on an MI355X: largest kernel error, largest fp32 restatement error, largest ratio of
the two within one case (o / dq / dk / dv; lse: absolute). Information, not bounds.
  route  regime   kernel    fp32      ratio      route  regime   kernel    fp32      ratio
  F1 o   unit     5.2e-7    7.5e-7    1.21       R1     unit     7.6e-7    5.8e-7    1.72
  F1 o   peaked   1.4e-6    4.1e-6    0.64       R1     peaked   1.8e-6    3.0e-6    1.10
  F1 o   blocks   1.2e-6    1.7e-6    1.18       R1     blocks   1.2e-6    1.6e-6    1.39
  F2 o   unit     9.3e-7    9.1e-7    1.43       R2     unit     7.3e-7    7.7e-7    2.61
  F2 o   peaked   1.8e-6    4.0e-6    0.69       R2     peaked   2.0e-6    3.3e-6    0.75
  F2 o   blocks   1.1e-6    1.8e-6    1.04       R2     blocks   1.1e-6    1.9e-6    1.60
  F3 o   (the kernel of F2: the same figures)    R3     unit     9.3e-7    5.0e-7    1.93
  lse    unit     3.0e-6    1.3e-6    2.97       R3     blocks   2.9e-6    9.2e-7    3.09
  lse    peaked   4.2e-6    5.8e-6    0.81       R4     unit     1.2e-6    7.7e-7    1.97
  lse    blocks   3.3e-6    2.2e-6    1.69       R4     blocks   3.2e-6    1.1e-6    3.00
  R6     unit     5.0e-7    3.4e-7    1.49       R5     unit     1.2e-6    7.7e-7    3.22
                                                 R5     blocks   1.5e-6    1.1e-6    1.74
(lse: one fp32 ulp of |lse2| up to 16 is 9.5e-7 and part of its bound.)
"""
import math
import types

import numpy as np
import pytest
import torch

import _attn_ref as ref
from _arena import SENTINEL, Arena, assert_both_equal, bit_equal, run_both

pytestmark = pytest.mark.gpu
F32, I64, I32 = torch.float32, torch.int64, torch.int32
CAP_ATTN = 1e-5


def _L():
    from fgreg import _lib
    return _lib.load()


def _ok(rc, name):
    from fgreg import _lib
    _lib.check(rc, name)


def _ws(name, *args):
    from fgreg import _lib
    return _lib.ws_size(name, *args)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _id(c):
    regime, seg, drop = c
    return f'{regime}-{seg}-' + ('p0' if drop is None else f'{drop[0]}-{drop[1]}')


def _hold(route, c, name, got):
    """Prints the kernel's and the restatement's error, then asserts the module's bound."""
    den, want = c.dens[name], c.ref[name]
    e, e32 = ref.cond_err(got, want, den), c.e32[name]
    what = f'{route} {c.regime} {c.seg} nhead {c.nhead} dh {c.dh} drop {c.drop} {name}'
    print(f'attn-train-error {what}: kernel {e:.3e} fp32-restatement {e32:.3e} '
          f'ratio {e / e32:.2f}')
    zero = den == 0
    if bool(zero.any()):
        assert bool((got.detach().cpu()[zero] == 0).all()), (what, 'zero-denominator elements')
    bound = 4 * e32 + 1e-7
    if c.regime == 'unit':
        bound = min(bound, CAP_ATTN)
    assert e <= bound, (what, e, e32, bound)


def _hold_lse(route, c, got):
    want = c.ref['lse']
    e = float((got.detach().double().cpu().reshape(want.shape) - want).abs().max())
    ulp = 2.0 ** (math.floor(math.log2(float(want.abs().max()))) - 23)
    print(f'attn-train-error {route} {c.regime} {c.seg} dh {c.dh} drop {c.drop} lse: kernel '
          f'{e:.3e} fp32-restatement {c.e32["lse"]:.3e} ulp {ulp:.3e}')
    assert e <= 4 * c.e32['lse'] + ulp, (route, e, c.e32['lse'], ulp)


def _tables(ar, c):
    qo = ar.put(torch.tensor(np.cumsum([0] + c.qlens), dtype=I64), name='q_off')
    ko = ar.put(torch.tensor(np.cumsum([0] + c.klens), dtype=I64), name='kv_off')
    sg = ar.put(torch.tensor(c.kv_seg, dtype=I32), name='kv_seg')
    return qo, ko, sg


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
def _forward(ar, c, entry):
    """fgr_attention_f16x3_train ('train') or _drop ('drop') on arena operands -> (o[, lse])."""
    d, ld = c.nhead * c.dh, c.nhead * c.dh + 4
    nq, nk = sum(c.qlens), sum(c.klens)
    Q, K, V = (ar.put(t, ld=ld, name=n) for t, n in ((c.q, 'q'), (c.k, 'k'), (c.v, 'v')))
    O = ar.matrix(nq, d, ld, F32, 'out', name='o')
    nb = _ws('fgr_attention_f16x3_workspace', nk, len(c.klens), c.nhead)
    ws = ar.bytes(nb, name='ws')
    qo, ko, sg = _tables(ar, c)
    seed, p = c.drop if c.drop is not None else (0, 0.0)
    args = (_p(Q), ld, _p(K), ld, _p(V), ld, _p(O), ld, _p(qo), _p(ko), _p(sg), len(c.qlens),
            len(c.klens), nk, max(c.qlens), max(c.klens), c.nhead, c.dh, c.scale, _p(ws), nb,
            seed, p)
    if entry == 'train':
        lse = ar.vector(nq * c.nhead, F32, 'out', name='lse')
        _ok(_L().fgr_attention_f16x3_train(*args, _p(lse), _st()), 'fgr_attention_f16x3_train')
        return O, lse
    _ok(_L().fgr_attention_f16x3_drop(*args, _st()), 'fgr_attention_f16x3_drop')
    return (O,)


def _forward_case(gpu, route, entry, regime, seg, drop, dh):
    c = ref.case(regime, seg, 2, dh, drop)
    clean, poisoned = run_both(lambda ar: _forward(ar, c, entry), gpu)
    assert_both_equal(clean, poisoned)
    _hold(route, c, 'o', clean[0])
    if entry == 'train':
        _hold_lse(route, c, clean[1])


@pytest.mark.parametrize('dh', [32, 64])
@pytest.mark.parametrize('case', ref.FWD_P0, ids=_id)
def test_forward_train(gpu, case, dh):
    """F1: o and lse of fgr_attention_f16x3_train without dropout."""
    _forward_case(gpu, 'F1', 'train', *case, dh)


@pytest.mark.parametrize('dh', [32, 64])
@pytest.mark.parametrize('case', ref.FWD_DROP, ids=_id)
def test_forward_train_dropout(gpu, case, dh):
    """F2: o under the mask; the lse is still that of the undropped softmax. (0, 0.9) and
    (0xFFFFFFFF, 0.9) on 'self' drop every weight of row 130: o = 0 there."""
    _forward_case(gpu, 'F2', 'train', *case, dh)


@pytest.mark.parametrize('dh', [32, 64])
@pytest.mark.parametrize('case', ref.FWD_DROP, ids=_id)
def test_forward_drop(gpu, case, dh):
    """F3: fgr_attention_f16x3_drop (no lse)."""
    _forward_case(gpu, 'F3', 'drop', *case, dh)


# ---------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------
def _backward(ar, c, entry, ws_from, ld_pad=4, misalign=0, calls=1):
    """fgr_attention_bwd_train ('train') or _drop ('drop') with the workspace size of
    fgr_attention_bwd_train_workspace ('train') or fgr_attention_bwd_workspace ('plain').
    -> (rc, [(dq, dk, dv) of each call])."""
    d = c.nhead * c.dh
    ld = d + ld_pad
    nq, nk = sum(c.qlens), sum(c.klens)
    put = lambda t, name: ar.put(t, ld=ld, name=name, misalign=misalign)
    Q, K, V = put(c.q, 'q'), put(c.k, 'k'), put(c.v, 'v')
    O, DO = put(c.ref['o'].float(), 'o'), put(c.R, 'dout')
    outs = [ar.matrix(n, d, ld, F32, 'out', name=name, misalign=misalign)
            for n, name in ((nq, 'dq'), (nk, 'dk'), (nk, 'dv'))]
    if ws_from == 'train':
        nb = _ws('fgr_attention_bwd_train_workspace', nq, len(c.qlens), nk, len(c.klens), c.nhead,
                 c.dh)
    else:
        nb = _ws('fgr_attention_bwd_workspace', nq, c.nhead)
    ws = ar.bytes(nb, name='ws')
    qo, ko, sg = _tables(ar, c)
    seed, p = c.drop if c.drop is not None else (0, 0.0)
    args = (_p(Q), ld, _p(K), ld, _p(V), ld, _p(O), ld, _p(DO), ld, _p(outs[0]), ld, _p(outs[1]),
            ld, _p(outs[2]), ld, _p(qo), _p(ko), _p(sg), len(c.qlens), len(c.klens), nq,
            max(c.qlens), max(c.klens), c.nhead, c.dh, c.scale, _p(ws), nb, seed, p)
    lse = ar.put(c.ref['lse'].float().reshape(-1), name='lse') if entry == 'train' else None
    got, rc = [], 0
    for _ in range(calls):
        if entry == 'train':
            rc = _L().fgr_attention_bwd_train(*args, _p(lse), nk, _st())
        else:
            rc = _L().fgr_attention_bwd_drop(*args, _st())
        if rc != 0:
            break
        got.append(tuple(t.clone() for t in outs) if calls > 1 else tuple(outs))
    return rc, got


def _backward_case(gpu, route, entry, ws_from, regime, seg, drop, dh, nhead=2, ld_pad=4,
                   misalign=0, lse_shift=0):
    c = ref.case(regime, seg, nhead, dh, drop)
    if lse_shift:
        # P = exp2(s - lse2): a kernel that reads the lse it is given scales P, hence dS and all
        # three gradients (D = dO . O comes from o), by exactly 2^-shift
        f = 2.0 ** -lse_shift
        c = types.SimpleNamespace(**vars(c))
        c.ref = {n: (t + lse_shift if n == 'lse' else t if n == 'o' else t * f)
                 for n, t in c.ref.items()}
        c.dens = {n: t * f for n, t in c.dens.items()}

    def fn(ar):
        rc, got = _backward(ar, c, entry, ws_from, ld_pad, misalign)
        _ok(rc, f'fgr_attention_bwd_{entry}')
        return got[0]
    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    for name, got in zip(('dq', 'dk', 'dv'), clean):
        _hold(route, c, name, got)


@pytest.mark.parametrize('dh', [32, 64])
@pytest.mark.parametrize('case', ref.BWD_P0, ids=_id)
def test_backward_f16x3(gpu, case, dh):
    """R1: attn_bwd_dq / dkdv_f16x3_kernel<DH, false>. 'mixed': two query segments share a key
    segment (the dK / dV kernel's DMA restarts per query segment), 129 key rows are attended by
    nobody (dk = dv = 0 exactly)."""
    _backward_case(gpu, 'R1', 'train', 'train', *case, dh)


@pytest.mark.parametrize('dh', [32, 64])
@pytest.mark.parametrize('case', ref.BWD_DROP, ids=_id)
def test_backward_f16x3_dropout(gpu, case, dh):
    """R2: <DH, true>: the mask replayed by the dQ and by the dK / dV kernel. (0, 0.9) and
    (0xFFFFFFFF, 0.9) on 'self': row 130 loses every weight, its dq, dk and dv are exactly 0."""
    _backward_case(gpu, 'R2', 'train', 'train', *case, dh)


@pytest.mark.parametrize('nhead,dh', ref.HEADS)
@pytest.mark.parametrize('drop', [None, ref.DROPS[0]], ids=['p0', 'drop'])
def test_backward_f16x3_head_stride(gpu, drop, nhead, dh):
    """R1 / R2 at nhead 3 (d 96) and nhead 8 (d 256, the shipped width): the per-(tile, head)
    exponent and lse / D tile indices stride by n_head."""
    _backward_case(gpu, 'R2' if drop else 'R1', 'train', 'train', 'unit', 'mixed', drop, dh,
                   nhead=nhead)


@pytest.mark.parametrize('dh', [16, 32, 64])
@pytest.mark.parametrize('case', ref.MFMA_P0, ids=_id)
def test_backward_mfma_lse(gpu, case, dh):
    """R3: a workspace of only fgr_attention_bwd_workspace bytes runs attn_bwd_*_mfma_kernel<DH>
    with the forward's lse (pass 1 skipped)."""
    _backward_case(gpu, 'R3', 'train', 'plain', *case, dh)


@pytest.mark.parametrize('dh', [16, 32, 64])
@pytest.mark.parametrize('case', ref.MFMA_DROP, ids=_id)
def test_backward_mfma_lse_dropout(gpu, case, dh):
    """R4: attn_bwd_*_mfma_kernel<DH, true> with the forward's lse; dh 16 is <16, true>."""
    _backward_case(gpu, 'R4', 'train', 'plain', *case, dh)


@pytest.mark.parametrize('dh', [16, 32, 64])
@pytest.mark.parametrize('case', ref.MFMA_DROP, ids=_id)
def test_backward_drop(gpu, case, dh):
    """R5: fgr_attention_bwd_drop, <DH, true> with its own max / sum pass."""
    _backward_case(gpu, 'R5', 'drop', 'plain', *case, dh)


@pytest.mark.parametrize('ws_from,dh', [('train', 32), ('train', 64), ('plain', 16), ('plain', 32),
                                        ('plain', 64)])
@pytest.mark.parametrize('drop', [None, ref.DROPS[0]], ids=['p0', 'drop'])
def test_backward_reads_the_forward_lse(gpu, drop, ws_from, dh):
    """R1 - R4 take P from the lse they are handed, not from a pass of their own: with lse2 + 1
    every gradient is the reference's halved (same per-element bound)."""
    route = {('train', False): 'R1', ('train', True): 'R2', ('plain', False): 'R3',
             ('plain', True): 'R4'}[(ws_from, drop is not None)]
    _backward_case(gpu, route + ' lse+1', 'train', ws_from, 'unit', 'mixed', drop, dh, lse_shift=1)


@pytest.mark.parametrize('dh,ld_pad,misalign', [(8, 4, 0), (32, 1, 4)],
                         ids=['dh8', 'dh32-misaligned'])
def test_backward_scalar(gpu, dh, ld_pad, misalign):
    """R6: fgr_attention_bwd_train where neither matrix-core route applies (head dim 8; row
    stride d + 1 and operands 4 B past a 16-B boundary): the scalar kernels, which recompute
    the lse, give the same gradients."""
    _backward_case(gpu, 'R6', 'train', 'train', 'unit', 'mixed', None, dh, ld_pad=ld_pad,
                   misalign=misalign)


@pytest.mark.parametrize('entry', ['train', 'drop'])
@pytest.mark.parametrize('dh,ld_pad,misalign', [(8, 4, 0), (32, 1, 4)],
                         ids=['dh8', 'dh32-misaligned'])
def test_backward_dropout_refused(gpu, dh, ld_pad, misalign, entry):
    """Dropout where no kernel replays the mask (head dim 8, misaligned rows): a non-zero code,
    the reason in fgr_last_error, and every output sentinel still in place."""
    c = ref.case('unit', 'mixed', 2, dh, ref.DROPS[0])
    ar = Arena(gpu)
    rc, _ = _backward(ar, c, entry, 'train' if entry == 'train' else 'plain', ld_pad, misalign)
    torch.cuda.synchronize()
    assert rc != 0
    msg = _L().fgr_last_error().decode()
    assert 'dropout needs head dim 16 / 32 / 64 and 16-B aligned rows' in msg, msg
    for r in ar.regions:
        if r.role == 'out':
            assert bool((r.buf.view(torch.int32) == SENTINEL).all()), r.name


@pytest.mark.parametrize('dh', [32, 64])
@pytest.mark.parametrize('drop', [None, ref.DROPS[0]], ids=['p0', 'drop'])
def test_backward_f16x3_deterministic(gpu, drop, dh):
    """R1 / R2 on 'mixed': two calls on one arena (the second over the first's workspace) give
    bit-identical dq, dk and dv."""
    c = ref.case('unit', 'mixed', 2, dh, drop)
    ar = Arena(gpu)
    rc, got = _backward(ar, c, 'train', 'train', calls=2)
    _ok(rc, 'fgr_attention_bwd_train')
    torch.cuda.synchronize()
    ar.check()
    for a, b, name in zip(got[0], got[1], ('dq', 'dk', 'dv')):
        assert bit_equal(a, b), name
