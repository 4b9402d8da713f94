"""fgr_attention_weights / fgreg.ops.attention_weights (the head-averaged attention maps) on the
GPU against tests/_attn_weights_ref.py, on the seeded segment sets of tests/_attn_ref.py: an empty
segment, a one-key segment, 64 and 65 rows, five tiles with a partial last one, shared and
unattended key segments, keys of their own row space.

Accuracy. Per element against the fp64 reference over the valid columns, conftest.elem_err with
floor 1e-3 (of the largest weight of the case); the bound is max(4 x the same error of the fp32
restatement on the CPU, 1e-6): the yardstick is the restatement, never the kernel, and the 1e-6
floor (about 8 ulp) covers cases where the restatement happens to land exact. Every case prints
both errors before it asserts.

Exact. Columns past a row's key segment are bit-zero; a one-key row is exactly 1.0 (n_head a
power of two); every valid row sums to 1 within n 2^-23; two runs give the same bits.

Footprint. Through ctypes on operands carved out of tests/_arena.py: only [0, max_kv_len) of
every query row is written (all of it), nothing in the pad columns, before the first or beyond
the last row; the result does not depend on pad columns or on what the output held.
"""
import math

import numpy as np
import pytest
import torch

from _arena import SENTINEL, Arena, assert_both_equal, bit_equal, run_both
from _attn_weights_ref import case
from conftest import elem_err

pytestmark = pytest.mark.gpu
F32, I64, I32 = torch.float32, torch.int64, torch.int32
BASE = [(r, s) for r in ('unit', 'peaked') for s in ('self', 'mixed')] + [('unit', 'separate')]
HEADS = [(8, 4), (2, 8), (2, 32), (8, 32), (8, 64), (1, 128)]
# every (regime, segments) at ModelNet's head dim, every (n_head, dh) on the shared-key case and
# on the peaked one
CASES = sorted(set([(r, s, 2, 32) for r, s in BASE] + [('unit', 'mixed', h, dh) for h, dh in HEADS]
                   + [('peaked', 'self', h, dh) for h, dh in HEADS]))


def _tables(cs, dev):
    off = lambda lens: torch.tensor(np.cumsum([0] + list(lens)), dtype=I64, device=dev)
    return off(cs.qlens), off(cs.klens), torch.tensor(cs.kv_seg, dtype=I32, device=dev)


def _check(got, cs, what):
    """The accuracy bound and the exact properties of one result (rows, max_kv) on the host."""
    got = got.detach().cpu()
    assert got.shape == cs.w64.shape and got.dtype == F32
    assert bool(torch.isfinite(got).all())
    m = cs.mask
    e = elem_err(got[m], cs.w64[m], floor=1e-3)
    e32 = elem_err(cs.w32[m], cs.w64[m], floor=1e-3)
    print(f'attention-weights {what}: kernel {e:.3e} fp32-restatement {e32:.3e}')
    assert e <= max(4 * e32, 1e-6), (what, e, e32)
    assert bool((got[~m].view(torch.int32) == 0).all()), 'padded columns must be bit-zero'
    n = m.sum(-1)
    live = n > 0
    s = got.double().sum(-1)
    assert bool(((s - 1).abs()[live] <= n[live].double() * 2.0 ** -23).all()), \
        float(((s - 1).abs()[live] / n[live]).max())
    if cs.nhead & (cs.nhead - 1) == 0:
        assert bool((got[n == 1][:, 0] == 1.0).all())
    return e, e32


@pytest.mark.parametrize('regime,seg,nhead,dh', CASES)
def test_weights_vs_fp64(gpu, regime, seg, nhead, dh):
    from fgreg import ops
    cs = case(regime, seg, nhead, dh)
    if seg != 'mixed':                                           # these have one-key rows
        assert int((cs.mask.sum(-1) == 1).sum()) >= 1
    q_off, kv_off, kv_seg = _tables(cs, gpu)
    q, k = cs.q.to(gpu), cs.k.to(gpu)
    w = ops.attention_weights(q, k, q_off, kv_off, kv_seg, cs.max_q, nhead, max_kv_len=cs.max_kv)
    _check(w, cs, f'{regime}-{seg}-{nhead}x{dh}')
    w2 = ops.attention_weights(q, k, q_off, kv_off, kv_seg, cs.max_q, nhead, max_kv_len=cs.max_kv)
    assert bit_equal(w, w2)


@pytest.mark.parametrize('nhead,dh', [(8, 4), (8, 32), (8, 64)])
def test_weights_strided_operands(gpu, nhead, dh):
    """q and k as column slices of one [q | k | v] tensor (row stride 3 d) and an output wider
    than max_kv_len (an odd row stride: the 4-byte store path): same values as the dense call's
    bound, and the columns past max_kv_len keep what they held."""
    from fgreg import ops
    cs = case('unit', 'mixed', nhead, dh)
    d = nhead * dh
    q_off, kv_off, kv_seg = _tables(cs, gpu)
    qkv = torch.cat([cs.q, cs.k, torch.full_like(cs.q, float('nan'))], 1).to(gpu)
    out = torch.full((cs.q.shape[0], cs.max_kv + 5), -7.0, device=gpu)
    w = ops.attention_weights(qkv[:, :d], qkv[:, d:2 * d], q_off, kv_off, kv_seg, cs.max_q, nhead,
                              max_kv_len=cs.max_kv, out=out)
    assert w.data_ptr() == out.data_ptr() and w.shape == (cs.q.shape[0], cs.max_kv)
    _check(w, cs, f'strided-{nhead}x{dh}')
    assert bool((out[:, cs.max_kv:] == -7.0).all())
    dense = ops.attention_weights(cs.q.to(gpu), cs.k.to(gpu), q_off, kv_off, kv_seg, cs.max_q,
                                  nhead, max_kv_len=cs.max_kv)
    assert bit_equal(w.contiguous(), dense)                      # one arithmetic, whatever the layout


def _p(t):
    return t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _abi(ar, cs, ld_in, misalign, max_kv, ld_w, head_dim=None):
    from fgreg import _lib
    Q = ar.put(cs.q, ld=ld_in, name='q', misalign=misalign)
    K = ar.put(cs.k, ld=ld_in, name='k', misalign=misalign)
    W = ar.matrix(cs.q.shape[0], max_kv, max(ld_w, max_kv), F32, 'out', name='w',
                  misalign=misalign)
    off = lambda lens: torch.tensor(np.cumsum([0] + list(lens)), dtype=I64)
    qo, ko = ar.put(off(cs.qlens), name='q_off'), ar.put(off(cs.klens), name='kv_off')
    sg = ar.put(torch.tensor(cs.kv_seg, dtype=I32), name='kv_seg')
    rc = _lib.load().fgr_attention_weights(
        _p(Q), ld_in, _p(K), ld_in, _p(W), ld_w, _p(qo), _p(ko), _p(sg), len(cs.qlens), cs.max_q,
        max_kv, cs.nhead, cs.dh if head_dim is None else head_dim, cs.scale, _st())
    return rc, W


# (segments, n_head, dh, input pad, misalign, extra zero columns, output pad): 16-B operands with
# a last partial 16-B store (301 columns in rows of 304), 4-B operands and odd strides, keys of
# their own row space at head dim 64
FOOT = [('self', 8, 32, 4, 0, 1, 3), ('self', 8, 32, 3, 4, 0, 3), ('mixed', 8, 4, 4, 0, 2, 2),
        ('separate', 8, 64, 4, 0, 0, 4), ('separate', 2, 8, 1, 8, 3, 0)]


@pytest.mark.parametrize('seg,nhead,dh,pad_in,misalign,extra,pad_w', FOOT)
def test_weights_footprint(gpu, seg, nhead, dh, pad_in, misalign, extra, pad_w):
    from fgreg import _lib
    cs = case('unit', seg, nhead, dh)
    max_kv = cs.max_kv + extra

    def run(ar):
        rc, W = _abi(ar, cs, nhead * dh + pad_in, misalign, max_kv, max_kv + pad_w)
        _lib.check(rc, 'fgr_attention_weights')
        return W
    clean, poisoned = run_both(run, gpu)
    assert_both_equal(clean, poisoned)
    assert bool((clean[:, cs.max_kv:].view(torch.int32) == 0).all())
    _check(clean[:, :cs.max_kv], cs, f'footprint-{seg}-{nhead}x{dh}')


@pytest.mark.parametrize('head_dim,ld_short', [(6, 0), (260, 0), (0, 0), (32, 1)])
def test_weights_refused(gpu, head_dim, ld_short):
    """head_dim not a multiple of 4 or above 256, or ld_w < max_kv_len: a status, a message, no
    launch (the output keeps its sentinel everywhere)."""
    from fgreg import _lib
    cs = case('unit', 'self', 8, 32)
    ar = Arena(gpu, poison=True)
    rc, W = _abi(ar, cs, 8 * 32 + 4, 0, cs.max_kv, cs.max_kv - ld_short, head_dim=head_dim)
    torch.cuda.synchronize()
    assert rc != 0 and b'fgr_attention_weights' in _lib.load().fgr_last_error()
    for r in ar.regions:
        r.full = False
    ar.check()
    assert bool((W.view(torch.int32) == SENTINEL).all())
