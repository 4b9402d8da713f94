"""Every run-time dispatch branch of the non-GEMM entry points of include/fgreg.h against the
same operation in plain torch fp64 on the CPU.

The GEMM dispatchers are pinned by test_gemm_f16x3_tiles / test_gemm_bf16_rounding_points and
the footprint suite. Every other entry point also picks a kernel instantiation at run time
(channel count, head dim, width, row count, pointer alignment); this module runs the
instantiations the shipped configurations never produce. Branches that Python can select go
through fgreg.ops; alignment fallbacks and refusals go through ctypes with operands carved out
of tests/_arena.py (an overreach becomes an assertion, a refused call must leave every output
sentinel in place).

Error and bound. Per element, condition-aware: |got - ref64| / sum|terms| of that element
(_cond_err), so a wrong small element cannot hide behind the tensor's largest one. The bound is
the convention of test_gemm_split_vs_fp64 / test_attention_split_is_fp32_accurate: no worse
than 4x the same error of the torch fp32 restatement of the op plus 1e-7, and never above the
family's existing bound (1e-4; 1e-5 for attention). Counts, max-pool bits, copied columns and
the sentinels of refused calls are exact. Every case prints both errors before it asserts.

sum|terms| per family
  gather      sum_h w_h |x_h|. w = 1 - r / extent cancels at the influence boundary, where any
              fp32 evaluation has only absolute accuracy 2^-24 (1 + r / extent) and the weighted
              sum stops being a condition number, so neighbours within 2 % of the boundary of
              any kernel point are made shadows (_gather_data); every remaining weight is 0 in
              both or >= 0.02.
  attention   out: softmax |v|. Gradients: dS = P o (dP - D) with dP = dO V^T, D = rowsum(P o
              dP); G = P o (|dO| |V|^T + rowsum(P o |dO| |V|^T)) bounds |dS| term by term, so
              dq: scale G |K|, dk: scale G^T |Q|, dv: P^T |dO|. (corr_attention: v = xyz.)
              The reference and these denominators live in tests/_attn_ref.py (mha), which
              also carries the dropout mask of the training pair.
  layernorm   (|x| + |mean|) rstd |gamma| + |beta| + |add|.
  res2net     E_0 = |W_0| |h_0| + |b_0|, E_i = |W_i| (E_{i-1} + |h_i|) + |b_i| (ReLU is
              1-Lipschitz, so the error of step i - 1 reaches step i through |W_i|).

Entry point -> branch -> arguments that select it -> test
  fgr_kpconv_gather
    c1<16>              cin 1, n_kp <= 16           test_gpu_kernels::test_kpconv_gather_vs_torch[1-50], [1-7]
    c1<32>              cin 1, n_kp 17 / 32         test_gather_branches[1-17-7], [1-32-70]
    quads<4,1>          cin 16, n_kp <= 16, aligned test_kpconv_gather_vs_torch[16-50], [16-70]
    quads<8,2>          cin 32, n_kp <= 16, aligned test_kpconv_gather_vs_torch[32-50], [32-130], [32-5]
    narrow<8>           cin 2..8                    test_kpconv_gather_vs_torch[3-50]
    narrow<16>          cin 9..15                   test_gather_branches[12-15-7], [12-15-70]
    narrow<16>          cin 16, n_kp > 16           test_gather_branches[16-17-7]
    narrow<16>          cin 16, x misaligned        test_gather_quads_fallback[16-x]
    narrow<32>          cin 17..31                  test_gather_branches[24-15-7], [24-15-70]
    narrow<32>          cin 32, n_kp > 16           test_gather_branches[32-17-70]
    narrow<32>          cin 32, wf misaligned       test_gather_quads_fallback[32-wf]
    narrow<64>          cin 33..63                  test_gather_branches[48-15-7], [48-15-70]
    wide<1/2/4,16>      cin 64 / 128 / 256          test_kpconv_gather_vs_torch[64-50] .. [256-70]
    wide<1,32>          cin 64, n_kp 17 / 32        test_gather_branches[64-17-7], [64-32-70]
    wide<2,32>          cin 128, n_kp 17 / 32       test_gather_branches[128-17-70], [128-32-7]
    wide<4,32>          cin 256, n_kp 17 / 32       test_gather_branches[256-17-7], [256-32-70]
    refused             cin 96, 192 (was: 192 ran the 256-wide kernel)
                                                    test_gather_refuses_unsupported_width[96], [192]
    width == 0          any cin, idx NULL           test_gather_width_zero[1], [12], [16], [64]
  fgr_max_pool
    max_pool_wave<1>    c 64                        test_gpu_footprint::test_max_pool_footprint[64]
    max_pool_wave<2/4/8> c 128 / 256 / 512          test_max_pool_branches[128-*], [256-*], [512-*]
    max_pool_kernel     any other c                 test_max_pool_branches[1-*], [96-*]
  fgr_attention
    launch<4>, <8>      head dim 4, 8               test_attention_every_head_dim[4], [8]
    launch_v2<16,2>     head dim 16                 test_attention_every_head_dim[16]
    launch_v2<32/64,2>  head dim 32, 64             test_attention_every_head_dim[32], [64]
    launch<128>, <256>  head dim 128, 256           test_attention_every_head_dim[128], [256]
  fgr_attention_bwd
    scalar <4>          dh 4                        test_gpu_train::test_attention_backward[*-32-8]
    scalar <8>          dh 8                        test_gpu_train::test_attention_backward[*-64-8]
    mfma <16>           dh 16, aligned              test_gpu_train::test_attention_backward[*-128-8]
    mfma <32>, <64>     dh 32 / 64, aligned, no lse test_attention_bwd_aligned_mfma[32], [64]
    scalar <16/32/64>   ld % 4 != 0, rows misaligned test_attention_bwd_misaligned[16], [32], [64]
    f16x3 (lse)         dh 32 / 64 from attention_t test_gpu_train::test_attention_backward[*-256-8], [*-512-8]
  fgr_attention_f16x3_train, fgr_attention_f16x3_drop (test_gpu_attention_train.py, routes F1 - F3)
    v2<32/64, false> + lse   p = 0                  test_forward_train[*-32], [*-64]
    v2<32/64, true> + lse    p > 0                  test_forward_train_dropout[*-32], [*-64]
    v2<32/64, true>          _drop                  test_forward_drop[*-32], [*-64]
  fgr_attention_bwd_train, fgr_attention_bwd_drop (test_gpu_attention_train.py, routes R1 - R6)
    f16x3 <32/64, false>     ws of _train_workspace, p = 0   test_backward_f16x3[*], _head_stride[p0-*]
    f16x3 <32/64, true>      the same, p > 0        test_backward_f16x3_dropout[*], _head_stride[drop-*]
    mfma <16/32/64> lse_in   ws of fgr_attention_bwd_workspace bytes, p = 0
                                                    test_backward_mfma_lse[*-16], [*-32], [*-64]
    mfma <16/32/64, true> lse_in  the same, p > 0   test_backward_mfma_lse_dropout[*-16], [*-32], [*-64]
    mfma <16/32/64, true>    _drop (own pass 1)     test_backward_drop[*-16], [*-32], [*-64]
    scalar <8>, <32>         dh 8; ld % 4 != 0, rows misaligned (lse recomputed)
                                                    test_backward_scalar[dh8], [dh32-misaligned]
    refused                  p > 0 at dh 8 / misaligned  test_backward_dropout_refused[*]
  fgr_corr_attention, fgr_corr_attention_bwd
    <64>, <256>                                     test_gpu_train::test_corr_attention_backward[64], [256]
    <32>, <128>, <512>                              test_corr_attention_widths[32], [128], [512]
  fgr_layernorm, fgr_layernorm_dual
    lpr<32,1/2/4>, lpr<64,4> full (d 128, 256, 512, 1024), kernel<1> (d 32), kernel<4> (d 96, 192)
                                                    test_gpu_kernels::test_layernorm_vs_torch
    kernel<8>           d 300                       test_layernorm_branches[300]
    kernel<16>          d 600, 1000                 test_layernorm_branches[600], [1000]
    lpr<32,4> partly filled  d 320, 448             test_layernorm_branches[320], [448]
    lpr<64,4> partly filled  d 576, 960             test_layernorm_branches[576], [960]
    kernel<4/8/16>      d 256 / 512 / 1024, misaligned pointers
                                                    test_layernorm_misaligned[256], [512], [1024]
    dual lpr<32,*,true> d % 64 == 0, d <= 512       test_layernorm_branches[320], [448] (dual half)
    dual = two passes   any other d or misaligned   test_layernorm_branches[300] .. [1000],
                                                    test_layernorm_misaligned[*] (dual half)
  fgr_res2net_chain_h3
    <2>, <4>, <7>, <14> whole tiles (w 28, 56, 112, 224 via FGREG_R2N224=h3)
                                                    test_gpu_kernels::test_res2net_block_vs_oracle,
                                                    test_res2net_block_h3_width224
    <2> ragged tile     w 20                        test_res2net_h3_ragged_width[20]
    <4> ragged tile     w 52 (test_res2net_block_vs_oracle has 28, 56, 112, 224, 7 only)
                                                    test_res2net_h3_ragged_width[52]
    <7> ragged tile     w 100                       test_res2net_h3_ragged_width[100]
    <14> ragged tile    w 212                       test_res2net_h3_ragged_width[212]
    <14>                w 224, n 8192 (32-row blocks win)  test_res2net_h3_r48_rule[8192]
    <14,48>             w 224, n 8193 (48-row blocks win)  test_res2net_h3_r48_rule[8193]
  fgr_res2net_chain6
    <7>                 w 112                       test_gpu_kernels::test_res2net_block_vs_oracle[128-512]
    <14,16>, <14,48>    w 224, n 1500 / 9544        test_gpu_kernels::test_res2net_chain6_rows_bitexact
    <14> (32 rows)      w 224, 4096 < n <= 8192     test_res2net_chain6_32_rows
  fgr_instnorm (confirmed from norm.hip against the existing cases, no new test)
    seg16<1>            segments <= 1024 rows       test_gpu_kernels::test_instnorm_fusions_vs_torch[lens0-72-2.0], [lens1-72-2.0]
    seg16<2>            the same, c >= 512          test_instnorm_fusions_vs_torch[lens7-1024-2.0], [lens8-576--20.0]
    ls (3 launches)     longer, 256 % (c / 4) == 0  test_instnorm_fusions_vs_torch[lens3-64-2.0] .. [lens6-1024--30.0],
                                                    test_instnorm_long_repeat_and_graph
    chunk<1> + chunk<2> longer, any other c         test_instnorm_fusions_vs_torch[lens2-72-2.0]
    chunk<0>            unreachable: it needs a longest segment of at most kChunk = 768 rows,
                        and every segment of up to kSegRows = 1024 rows takes seg16 first
  fgr_add
    add4_kernel         n % 4 == 0, 16-B aligned    test_gpu_forward (forward_modelnet_postnorm: ops.add)
    add1_kernel         otherwise                   test_gpu_footprint::test_add_footprint (n 1027)
  geometry (fgr_radius_search modes, grid path, fgr_grid_subsample_*)
                                                    test_gpu_geometry (both modes, both paths)

Branches without a meaningful reference (named, not tested)
  instnorm_chunk_kernel<0>           unreachable from fgr_instnorm (above).
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _arena import SENTINEL, Arena
from _attn_ref import mha as _mha
from conftest import rel_err

pytestmark = pytest.mark.gpu
F32, I64, I32 = torch.float32, torch.int64, torch.int32
CAP, CAP_ATTN = 1e-4, 1e-5


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


def _cond_err(got, ref, den):
    """max_i |got_i - ref_i| / den_i, den_i = sum|terms| of element i (fp64). An element whose
    terms are all zero has den 0 and ref 0: anything but an exact 0 there is an error."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == den.shape, (got.shape, ref.shape, den.shape)
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / den.clamp_min(1e-300)).max())


def _hold(what, e, e32, cap):
    """The bound: <= 4 x the torch fp32 restatement's error + 1e-7, never above the family's."""
    print(f'dispatch-error {what}: kernel {e:.3e} fp32-restatement {e32:.3e}')
    assert e <= min(4 * e32 + 1e-7, cap), (what, e, e32)


# ---------------------------------------------------------------------------------------------
# fgr_kpconv_gather
# ---------------------------------------------------------------------------------------------
EXT = 0.5


def _gather_ref(q, s, idx, x, kp, dtype):
    """(wf, sum_h w_h |x_h|) of the gather in ``dtype`` on the CPU (blocks:296-381)."""
    q, s, x, kp = q.to(dtype), s.to(dtype), x.to(dtype), kp.to(dtype)
    sp = torch.cat([s, torch.full((1, 3), 1e6, dtype=dtype)])
    nb = sp[idx] - q.unsqueeze(1)
    d2 = ((nb.unsqueeze(2) - kp) ** 2).sum(3)
    w = torch.clamp(1 - torch.sqrt(d2) / EXT, min=0).transpose(1, 2)           # (nq, K, H)
    nx = torch.cat([x, torch.zeros(1, x.shape[1], dtype=dtype)])[idx]           # (nq, H, cin)
    return torch.matmul(w, nx), torch.matmul(w, nx.abs())


@functools.lru_cache(maxsize=None)
def _gather_data(cin, H, n_kp, nq=70, ns=90):
    """The table of test_gpu_kernels._gather_case (60 % shadows, query 3 all shadow) at 70
    queries over 90 supports; neighbours within 2 % of a kernel point's influence boundary
    become shadows (module docstring) and every feature row sums to at least 1e-3 in
    magnitude, so the normaliser's "row sum > 0" does not depend on the summation order."""
    rng = np.random.default_rng(1000 * cin + 10 * H + n_kp)
    s = rng.uniform(-1, 1, (ns, 3)).astype(np.float32)
    q = (s[rng.choice(ns, nq, replace=False)] + rng.normal(0, 0.01, (nq, 3))).astype(np.float32)
    idx = rng.integers(0, ns, (nq, H))
    idx[rng.uniform(size=(nq, H)) < 0.6] = ns
    idx[3] = ns
    x = rng.normal(size=(ns, cin)).astype(np.float32)
    rs = x.astype(np.float64).sum(1)
    x[np.abs(rs) < 1e-3, 0] += np.float32(0.5)
    kp = (rng.normal(size=(n_kp, 3)) * 0.3).astype(np.float32)
    q, s, x, kp, idx = (torch.from_numpy(a) for a in (q, s, x, kp, idx))
    sp = torch.cat([s.double(), torch.full((1, 3), 1e6, dtype=torch.float64)])
    r = torch.sqrt((((sp[idx] - q.double().unsqueeze(1)).unsqueeze(2) - kp.double()) ** 2).sum(3))
    idx[((1 - r / EXT).abs() < 0.02).any(2)] = ns
    assert int((idx[:, :] < ns).sum()) > nq and bool((idx[3] == ns).all())
    ref, den = _gather_ref(q, s, idx, x, kp, torch.float64)
    assert int((den > 0).sum()) > 50                       # the case has live elements
    e32 = _cond_err(_gather_ref(q, s, idx, x, kp, torch.float32)[0], ref, den)
    nx = torch.cat([x.double(), torch.zeros(1, cin, dtype=torch.float64)])[idx]
    cnt = torch.clamp((nx.sum(-1) > 0).sum(-1), min=1).float()
    return q, s, idx, x, kp, ref, den, e32, cnt


def _check_gather(what, wf, nn_, data):
    ref, den, e32, cnt = data[5:]
    _hold(what, _cond_err(wf.reshape(ref.shape), ref, den), e32, CAP)
    assert torch.equal(nn_.cpu(), cnt)


@pytest.mark.parametrize('cin,n_kp,H', [(12, 15, 7), (12, 15, 70), (24, 15, 7), (24, 15, 70),
                                        (48, 15, 7), (48, 15, 70), (16, 17, 7), (32, 17, 70),
                                        (1, 17, 7), (1, 32, 70), (64, 17, 7), (64, 32, 70),
                                        (128, 17, 70), (128, 32, 7), (256, 17, 7),
                                        (256, 32, 70)])
def test_gather_branches(gpu, cin, n_kp, H):
    """The narrow kernels at widths between the configs' (12, 24, 48), the quad-lane kernel's
    n_kp > 16 fallback (cin 16 / 32 -> narrow<16 / 32>), and the 32-kernel-point instances of
    the stem and wide kernels (n_kp 17: a partly filled second half; 32: kMaxKp)."""
    import fgreg.ops as ops
    data = _gather_data(cin, H, n_kp)
    q, s, idx, x, kp = (t.to(gpu) for t in data[:5])
    wf, nn_ = ops.kpconv_gather(q, s, idx, x, kp, EXT)
    _check_gather(f'gather cin {cin} n_kp {n_kp} H {H}', wf, nn_, data)


def _gather_abi(ar, data, cin, n_kp, H, mis_x=0, mis_wf=0):
    q, s, idx, x, kp = data[:5]
    nq, ns = q.shape[0], s.shape[0]
    wf = ar.matrix(nq, n_kp * cin, n_kp * cin, F32, 'out', name='wf', misalign=mis_wf)
    nn_ = ar.vector(nq, F32, 'out', name='nnorm')
    rc = _L().fgr_kpconv_gather(_p(ar.put(q, name='q')), _p(ar.put(s, name='s')), nq, ns,
                                _p(ar.put(idx, name='idx')), H,
                                _p(ar.put(x, name='x', misalign=mis_x)), cin,
                                _p(ar.put(kp, name='kp')), n_kp, EXT, _p(wf), _p(nn_), None, 0,
                                _st())
    return rc, wf, nn_


@pytest.mark.parametrize('cin,which', [(16, 'x'), (32, 'wf')])
def test_gather_quads_fallback(gpu, cin, which):
    """cin 16 / 32 with x or wf 4 bytes past a 16-B boundary: the quad-lane kernel's 16-B loads
    and stores do not apply and the dispatcher falls back to narrow<16> / narrow<32>."""
    data = _gather_data(cin, 70, 15)
    ar = Arena(gpu)
    rc, wf, nn_ = _gather_abi(ar, data, cin, 15, 70, mis_x=4 * (which == 'x'),
                              mis_wf=4 * (which == 'wf'))
    _ok(rc, 'fgr_kpconv_gather')
    torch.cuda.synchronize()
    ar.check()
    _check_gather(f'gather cin {cin} misaligned {which}', wf, nn_, data)


@pytest.mark.parametrize('cin', [96, 192])
def test_gather_refuses_unsupported_width(gpu, cin):
    """cin 96 and 192 are refused with FGR_E_ARG before any launch: the message lists the
    supported widths and every sentinel of wf and nnorm, payload and guards, is intact. (192
    used to run the 256-wide kernel on 192-wide rows.)"""
    data = _gather_data(cin, 7, 15)
    ar = Arena(gpu)
    rc, wf, nn_ = _gather_abi(ar, data, cin, 15, 7)
    torch.cuda.synchronize()
    assert rc == -1
    msg = _L().fgr_last_error().decode()
    assert f'cin {cin}' in msg and '128' in msg and '256' in msg and '64' in msg, msg
    for r in ar.regions:
        if r.role == 'out':
            assert bool((r.buf.view(torch.int32) == SENTINEL).all()), r.name


@pytest.mark.parametrize('cin', [1, 12, 16, 64])
def test_gather_width_zero(gpu, cin):
    """An empty neighbour table (width 0, idx NULL): wf is all zeros and nnorm all ones, from
    the stem, narrow, quad-lane and wide kernels."""
    nq, ns, n_kp = 70, 90, 15
    g = torch.Generator().manual_seed(cin)
    q, s = torch.randn(nq, 3, generator=g), torch.randn(ns, 3, generator=g)
    x, kp = torch.randn(ns, cin, generator=g), torch.randn(n_kp, 3, generator=g) * 0.3
    ar = Arena(gpu)
    wf = ar.matrix(nq, n_kp * cin, n_kp * cin, F32, 'out', name='wf')
    nn_ = ar.vector(nq, F32, 'out', name='nnorm')
    _ok(_L().fgr_kpconv_gather(_p(ar.put(q, name='q')), _p(ar.put(s, name='s')), nq, ns, None, 0,
                               _p(ar.put(x, name='x')), cin, _p(ar.put(kp, name='kp')), n_kp, EXT,
                               _p(wf), _p(nn_), None, 0, _st()), 'fgr_kpconv_gather')
    torch.cuda.synchronize()
    ar.check()
    assert bool((wf == 0).all()) and bool((nn_ == 1).all())


# ---------------------------------------------------------------------------------------------
# fgr_max_pool
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', [5, 40])
@pytest.mark.parametrize('c', [1, 96, 128, 256, 512])
def test_max_pool_branches(gpu, c, width):
    """max_pool_wave<2 / 4 / 8> (c 128 / 256 / 512) and the per-element kernel (c 1, 96):
    bit-equal to gather-and-max over the appended zero row; 70 queries (the last block of four
    is partial), a row of shadows only, channels whose values are all negative (the zero of a
    shadow entry wins) and rows without a shadow (it must not)."""
    import fgreg.ops as ops
    nq, ns = 70, 90
    rng = np.random.default_rng(c + width)
    idx = rng.integers(0, ns, (nq, width))
    idx[rng.uniform(size=(nq, width)) < 0.3] = ns
    idx[5] = ns
    idx[6] = rng.integers(0, ns, width)                      # no shadow at all
    x = rng.normal(size=(ns, c)).astype(np.float32)
    x[:, ::3] = -np.abs(x[:, ::3])
    x, idx = torch.from_numpy(x), torch.from_numpy(idx)
    ref = torch.cat([x, torch.zeros(1, c)])[idx].max(1).values
    out = ops.max_pool(x.to(gpu), idx.to(gpu)).cpu()
    assert torch.equal(out.view(I32), ref.view(I32))
    assert bool((ref[5] == 0).all()) and bool((ref[6, ::3] < 0).all())


# ---------------------------------------------------------------------------------------------
# attention: forward, backward, the correspondence head's
# ---------------------------------------------------------------------------------------------
QLENS, KLENS, KV_SEG = [130, 1, 64, 65], [65, 200, 1, 64], [1, 0, 3, 2]


@pytest.mark.parametrize('dh', [4, 8, 16, 32, 64, 128, 256])
def test_attention_every_head_dim(gpu, dh):
    """fgr_attention through the C ABI at each of its seven head dims (16 and 128 run nowhere
    else), two heads, key segmentation of its own (1-key and 200-key segments, a 1-row query
    segment, 64 / 65 / 130 rows: full, one-past and partial 64-row tiles)."""
    import fgreg.ops as ops
    from test_gpu_kernels import _attention_fp32
    nhead = 2
    d = nhead * dh
    g = torch.Generator().manual_seed(dh)
    q = torch.randn(sum(QLENS), d, generator=g)
    kv = torch.randn(sum(KLENS), 2 * d, generator=g)
    k, v = kv[:, :d], kv[:, d:]
    scale = math.sqrt(1.0 / dh)
    dens = {}
    ref = _mha(q.double(), k.double(), v.double(), QLENS, KLENS, KV_SEG, nhead, scale, dens=dens)
    e32 = _cond_err(_mha(q, k, v, QLENS, KLENS, KV_SEG, nhead, scale), ref, dens['o'])
    qg, kvg = q.to(gpu), kv.to(gpu)
    seg = torch.tensor(KV_SEG, dtype=I32, device=gpu)
    out = _attention_fp32(qg, kvg[:, :d], kvg[:, d:], ops.offsets(QLENS, gpu),
                          ops.offsets(KLENS, gpu), seg, max(QLENS), nhead)
    _hold(f'attention head dim {dh}', _cond_err(out, ref, dens['o']), e32, CAP_ATTN)


def _attention_bwd_case(gpu, dh, ld_pad, misalign):
    """fgr_attention_bwd through the C ABI on arena operands with row stride d + ld_pad, each
    ``misalign`` bytes past a 16-B boundary; q / k / v separate (own key segmentation)."""
    nhead = 2
    d = nhead * dh
    scale = math.sqrt(1.0 / dh)
    g = torch.Generator().manual_seed(100 + dh)
    q = torch.randn(sum(QLENS), d, generator=g)
    k = torch.randn(sum(KLENS), d, generator=g)
    v = torch.randn(sum(KLENS), d, generator=g)
    R = torch.randn(sum(QLENS), d, generator=g)

    def grads(dtype, dens=None):
        ql, kl, vl = (t.to(dtype).clone().requires_grad_(True) for t in (q, k, v))
        o = _mha(ql, kl, vl, QLENS, KLENS, KV_SEG, nhead, scale, R=R.to(dtype), dens=dens)
        (o * R.to(dtype)).sum().backward()
        return o.detach(), ql.grad, kl.grad, vl.grad
    dens = {}
    o64, *ref = grads(torch.float64, dens)
    e32 = [_cond_err(a, b, dens[n]) for a, b, n in zip(grads(torch.float32)[1:], ref,
                                                       ('dq', 'dk', 'dv'))]
    nq, nk, ld = q.shape[0], k.shape[0], d + ld_pad
    ar = Arena(gpu)
    put = lambda t, name: ar.put(t, ld=ld, name=name, misalign=misalign)
    Q, K, V, O, DO = put(q, 'q'), put(k, 'k'), put(v, 'v'), put(o64.float(), 'o'), put(R, 'dout')
    DQ = ar.matrix(nq, d, ld, F32, 'out', name='dq', misalign=misalign)
    DK = ar.matrix(nk, d, ld, F32, 'out', name='dk', misalign=misalign)
    DV = ar.matrix(nk, d, ld, F32, 'out', name='dv', misalign=misalign)
    from fgreg import _lib
    nb = _lib.ws_size('fgr_attention_bwd_workspace', nq, nhead)
    ws = ar.bytes(nb, name='ws')
    qo = ar.put(torch.tensor(np.cumsum([0] + QLENS), dtype=I64), name='q_off')
    ko = ar.put(torch.tensor(np.cumsum([0] + KLENS), dtype=I64), name='kv_off')
    sg = ar.put(torch.tensor(KV_SEG, dtype=I32), name='kv_seg')
    _ok(_L().fgr_attention_bwd(_p(Q), ld, _p(K), ld, _p(V), ld, _p(O), ld, _p(DO), ld, _p(DQ), ld,
                               _p(DK), ld, _p(DV), ld, _p(qo), _p(ko), _p(sg), len(QLENS),
                               len(KLENS), nq, max(QLENS), max(KLENS), nhead, dh, scale, _p(ws),
                               nb, _st()), 'fgr_attention_bwd')
    torch.cuda.synchronize()
    ar.check()
    for got, want, name, e in zip((DQ, DK, DV), ref, ('dq', 'dk', 'dv'), e32):
        _hold(f'attention_bwd head dim {dh} ld +{ld_pad} {name}', _cond_err(got, want, dens[name]),
              e, CAP_ATTN)


@pytest.mark.parametrize('dh', [16, 32, 64])
def test_attention_bwd_misaligned(gpu, dh):
    """Row stride d + 1 (ld % 4 != 0) and every operand 4 bytes past a 16-B boundary: the
    fp32-MFMA backward's 16-B row loads do not apply and fgr_attention_bwd runs the scalar
    attn_bwd_dq / dkdv_kernel<16 / 32 / 64>, which no aligned caller reaches."""
    _attention_bwd_case(gpu, dh, 1, 4)


@pytest.mark.parametrize('dh', [32, 64])
def test_attention_bwd_aligned_mfma(gpu, dh):
    """fgr_attention_bwd without the forward's lse at head dim 32 / 64 (attention_t always has
    the lse there and takes the f16x3 kernels): attn_bwd_*_mfma_kernel<32 / 64> on padded rows
    (ld = d + 4)."""
    _attention_bwd_case(gpu, dh, 4, 0)


CLOUDS = [33, 1, 70, 32]


@pytest.mark.parametrize('d', [32, 128, 512])
def test_corr_attention_widths(gpu, d):
    """fgr_corr_attention / _bwd at the widths the existing tests (64, 256) leave out, through
    corr_attention_t: 2 layers over clouds of 33, 1, 70 and 32 rows (cloud c attends to cloud
    (c + 2) % 4 of its layer; a 1-key segment, partial 32-row tiles), forward and dq / dk."""
    from fgreg.autograd import corr_attention_t
    from fgreg.transformer import Segments
    n_layers, N = 2, sum(CLOUDS)
    lens = CLOUDS * n_layers
    kv_seg = [l * 4 + (c + 2) % 4 for l in range(n_layers) for c in range(4)]
    scale = 1.0 / math.sqrt(d)
    g = torch.Generator().manual_seed(d)
    q = torch.randn(n_layers * N, d, generator=g)
    k = torch.randn(n_layers * N, d, generator=g)
    xyz = torch.randn(N, 3, generator=g)
    R = torch.randn(n_layers * N, 3, generator=g)

    def run(dtype, dens=None):
        ql, kl = (t.to(dtype).clone().requires_grad_(True) for t in (q, k))
        o = _mha(ql, kl, xyz.to(dtype).repeat(n_layers, 1), lens, lens, kv_seg, 1, scale,
                 R=R.to(dtype), dens=dens)
        (o * R.to(dtype)).sum().backward()
        return o.detach(), ql.grad, kl.grad
    dens = {}
    ref = run(torch.float64, dens)
    e32 = [_cond_err(a, b, dens[n]) for a, b, n in zip(run(torch.float32), ref, ('o', 'dq', 'dk'))]
    Q, K = q.to(gpu).requires_grad_(True), k.to(gpu).requires_grad_(True)
    corr = corr_attention_t(Q, K, xyz.to(gpu), Segments(CLOUDS, gpu, n_layers=n_layers), scale)
    (corr * R.to(gpu)).sum().backward()
    for got, want, name, e in zip((corr, Q.grad, K.grad), ref, ('o', 'dq', 'dk'), e32):
        _hold(f'corr_attention d {d} {name}', _cond_err(got, want, dens[name]), e, CAP_ATTN)


# ---------------------------------------------------------------------------------------------
# fgr_layernorm, fgr_layernorm_dual
# ---------------------------------------------------------------------------------------------
LN_ROWS = (1, 7, 9, 333)


@functools.lru_cache(maxsize=None)
def _ln_data(d, n=333):
    g = torch.Generator().manual_seed(d)
    x = torch.randn(n, d, generator=g) * 2 + 1
    w = torch.randn(2, d, generator=g) * 0.1 + 1
    b = torch.randn(2, d, generator=g) * 0.1
    a = torch.randn(2, n, d, generator=g)
    pb = torch.randn(d, generator=g)
    return x, w, b, a, pb


def _ln_ref(x, w, b, a, dtype):
    """(LN(x) w + b + a, its sum|terms|) in ``dtype``."""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    y = F.layer_norm(x, (x.shape[1],), w, b, 1e-5)
    mean = x.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)
    den = (x.abs() + mean.abs()) * rstd * w.abs() + b.abs()
    if a is not None:
        y, den = y + a.to(dtype), den + a.to(dtype).abs()
    return y, den


def _ln_check(what, got, x, w, b, a):
    ref, den = _ln_ref(x, w, b, a, torch.float64)
    e32 = _cond_err(_ln_ref(x, w, b, a, torch.float32)[0], ref, den)
    _hold(what, _cond_err(got, ref, den), e32, CAP)


@pytest.mark.parametrize('d', [300, 320, 448, 576, 600, 960, 1000])
def test_layernorm_branches(gpu, d):
    """layernorm_kernel<8> (d 300) and <16> (600, 1000); the vector kernels with a partly filled
    last chunk, lpr<32,4> (320, 448) and lpr<64,4> (576, 960); 1, 7, 9 and 333 rows (a single
    row, partial blocks of 4 and of 8). Each with `add`, with `pre_bias` (x rewritten in place)
    and as fgr_layernorm_dual (d <= 512 and d % 64 == 0: one pass; else two of the above)."""
    import fgreg.ops as ops
    x, w, b, a, pb = _ln_data(d)
    G = lambda t: t.to(gpu).contiguous()
    for n in LN_ROWS:
        out = ops.layernorm(G(x[:n]), G(w[0]), G(b[0]), 1e-5, add=G(a[0, :n]))
        _ln_check(f'layernorm d {d} n {n} add', out, x[:n], w[0], b[0], a[0, :n])
        X = G(x[:n])
        out = ops.layernorm(X, G(w[0]), G(b[0]), 1e-5, pre_bias=G(pb))
        xb = (x[:n].double() + pb.double())
        assert rel_err(X, xb) < 1e-7
        _ln_check(f'layernorm d {d} n {n} pre_bias', out, X.cpu(), w[0], b[0], None)
        na, nb_ = torch.nn.LayerNorm(d), torch.nn.LayerNorm(d)
        with torch.no_grad():
            for m, i in ((na, 0), (nb_, 1)):
                m.weight.copy_(w[i])
                m.bias.copy_(b[i])
        oa, ob = ops.layernorm_dual(G(x[:n]), na.to(gpu), nb_.to(gpu), add_b=G(a[1, :n]))
        _ln_check(f'layernorm_dual d {d} n {n} a', oa, x[:n], w[0], b[0], None)
        _ln_check(f'layernorm_dual d {d} n {n} b', ob, x[:n], w[1], b[1], a[1, :n])


@pytest.mark.parametrize('d', [256, 512, 1024])
def test_layernorm_misaligned(gpu, d):
    """Every operand 4 bytes past a 16-B boundary at widths the vector kernels own: the
    dispatcher must take the scalar layernorm_kernel<4 / 8 / 16> (fgr_layernorm with add and
    pre_bias; fgr_layernorm_dual as two such passes), not 16-B loads on those pointers."""
    x, w, b, a, pb = _ln_data(d)
    for n in LN_ROWS:
        ar = Arena(gpu)
        put = lambda t, name: ar.put(t.contiguous(), name=name, misalign=4)
        X = put(x[:n], 'x')
        out = ar.matrix(n, d, d, F32, 'out', name='out', misalign=4)
        _ok(_L().fgr_layernorm(_p(X), n, d, _p(put(w[0], 'g')), _p(put(b[0], 'b')), 1e-5,
                               _p(put(a[0, :n], 'add')), _p(put(pb, 'pb')), _p(out), _st()),
            'fgr_layernorm')
        o1 = ar.matrix(n, d, d, F32, 'out', name='out1', misalign=4)
        o2 = ar.matrix(n, d, d, F32, 'out', name='out2', misalign=4)
        X2 = put(x[:n], 'x2')
        _ok(_L().fgr_layernorm_dual(_p(X2), n, d, _p(put(w[0], 'g1')), _p(put(b[0], 'b1')), None,
                                    _p(o1), _p(put(w[1], 'g2')), _p(put(b[1], 'b2')),
                                    _p(put(a[1, :n], 'add2')), _p(o2), 1e-5, _st()),
            'fgr_layernorm_dual')
        torch.cuda.synchronize()
        ar.check()
        assert rel_err(X, x[:n].double() + pb.double()) < 1e-7
        assert torch.equal(X2.cpu(), x[:n])
        _ln_check(f'layernorm misaligned d {d} n {n}', out, X.cpu(), w[0], b[0], a[0, :n])
        _ln_check(f'layernorm_dual misaligned d {d} n {n} a', o1, x[:n], w[0], b[0], None)
        _ln_check(f'layernorm_dual misaligned d {d} n {n} b', o2, x[:n], w[1], b[1], a[1, :n])


# ---------------------------------------------------------------------------------------------
# fgr_res2net_chain_h3, fgr_res2net_chain6
# ---------------------------------------------------------------------------------------------
def _chain_ref(h, W, b, x, w, scale, dtype):
    """(cat, sum|terms|) of the Res2Net hierarchy (res2net.py:126-159, BatchNorm folded into
    (W_i, b_i)): sp_i = relu(W_i (sp_{i-1} + h_i) + b_i), cat = [sp_0 .. sp_{scale-2} |
    h_{scale-1} | x]. The copied columns carry sum|terms| = |value| (they must be exact)."""
    h, W, b, x = h.to(dtype), W.to(dtype), b.to(dtype), x.to(dtype)
    cols, dens = [], []
    sp = E = None
    for i in range(scale - 1):
        hi = h[:, i * w:(i + 1) * w]
        a = hi if i == 0 else sp + hi
        ea = hi.abs() if i == 0 else E + hi.abs()
        sp = torch.relu(a @ W[i].t() + b[i])
        E = ea @ W[i].abs().t() + b[i].abs()
        cols.append(sp)
        dens.append(E)
    tail = [h[:, (scale - 1) * w:], x]
    return torch.cat(cols + tail, 1), torch.cat(dens + [t.abs() for t in tail], 1)


def _chain_case(gpu, what, n, w, scale, cin, h3):
    import fgreg.ops as ops
    g = torch.Generator().manual_seed(n + w)
    h = torch.relu(torch.randn(n, scale * w, generator=g))       # conv1 -> bn1 -> relu output
    W = torch.randn(scale - 1, w, w, generator=g) / math.sqrt(w)
    b = torch.randn(scale - 1, w, generator=g) * 0.1
    x = torch.randn(n, cin, generator=g)
    ref, den = _chain_ref(h, W, b, x, w, scale, torch.float64)
    e32 = _cond_err(_chain_ref(h, W, b, x, w, scale, torch.float32)[0], ref, den)
    Wg = W.to(gpu)
    cat = torch.full((n, scale * w + cin), float('nan'), device=gpu)
    if h3:
        assert ops.res2net_chain_supported(w, True)
        img, wsc = ops.res2net_fragments_h3(Wg)
        ops.res2net_chain(h.to(gpu), w, scale, img, b.to(gpu), x.to(gpu), cat, w_scale=wsc)
    else:
        ops.res2net_chain(h.to(gpu), w, scale, ops.res2net_fragments3(Wg), b.to(gpu), x.to(gpu), cat)
    nw = (scale - 1) * w
    assert torch.equal(cat[:, nw:].cpu(), torch.cat([h[:, nw:], x], 1))      # copies are exact
    _hold(what, _cond_err(cat, ref, den), e32, CAP)


@pytest.mark.parametrize('w', [20, 52, 100, 212])
def test_res2net_h3_ragged_width(gpu, w):
    """fgr_res2net_chain_h3 at widths that end inside a 16-column tile (kernel <2>, <4>, <7>,
    <14> with zero-padded weight rows and a last tile that stores 4 / 4 / 4 / 4 of 16 columns):
    the full 7-step hierarchy of scale 8 over 70 rows (two full 32-row blocks and 6 rows)."""
    _chain_case(gpu, f'res2net_h3 w {w}', 70, w, 8, 12, True)


@pytest.mark.parametrize('n', [8192, 8193])
def test_res2net_h3_r48_rule(gpu, n):
    """Width 224 on each side of the row-block rule: 8192 rows fill one round of 256 32-row
    blocks (kernel <14>), 8193 need a second round and go to the 48-row blocks (<14, 48>,
    171 blocks, the last with 33 rows). Scale 3 (two chained steps) keeps the case small."""
    _chain_case(gpu, f'res2net_h3 w 224 n {n}', n, 224, 3, 8, True)


def test_res2net_chain6_32_rows(gpu):
    """fgr_res2net_chain6 at width 224 picks 32-row blocks only for 4096 < n <= 8192 (16 rows
    below: more CUs; 48 above: fewer rounds); 4097 rows: 129 blocks, the last with one row."""
    _chain_case(gpu, 'res2net_chain6 w 224 n 4097', 4097, 224, 3, 8, False)
