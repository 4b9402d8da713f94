"""Plain restatements of the training backward's non-attention ops for test_gpu_backward.py, in
any dtype on the CPU (fp64: the checker; fp32: the yardstick of the project's error bound), with
the sum|terms| of every output element, plus the bf16 GEMM dispatcher restated from
csrc/bf16.hip. Not a conftest: imported by the tests that use it (test_backward_ref.py checks
it on the CPU).
"""
import math

import numpy as np
import torch

import _kpconv_modes as km

U = 2.0 ** -24                             # unit roundoff of fp32
EPS = float(np.float32(1e-5))              # the float the kernels receive as eps


# ---------------------------------------------------------------------------------------------
# GEMM bounds and the bf16 dispatcher
# ---------------------------------------------------------------------------------------------
def bf(t):
    """The bf16 rounding point of DESIGN.md "bf16 mode": round to nearest even, as fp64."""
    return t.detach().cpu().float().to(torch.bfloat16).double()


def accum_bound(K):
    """Worst case of an fp32 accumulation in k-steps of 32 per unit of sum|terms|: one rounding
    per step, 8 more for the epilogue (bias, residual, split-K merge, the output)."""
    return (math.ceil(K / 32) + 8) * U


def bf16_bound(K):
    return min(accum_bound(K), 1e-5)       # never above the documented 1e-5


def f16x3_bound(K):
    return 3 * 2.0 ** -22 + accum_bound(K)  # fgreg/linear.py's per-product bound + accumulation


def splitk_shape(m, n, k):
    return k >= 1920 and n <= 256 and ((m + 63) // 64) * ((n + 63) // 64) <= 160


def bf16_tile(m, n, k):
    """bf16_tile of csrc/bf16.hip without the FGR_GEMM_BF16_TILE override."""
    tiles64 = ((m + 63) // 64) * ((n + 63) // 64)
    if k % 8 == 0 and splitk_shape(m, n, k):
        return 'X' if k >= 2048 else 'S'
    if tiles64 <= 400 and k >= 512 and n >= 32:
        if k >= 2048 or n <= 64:
            return 'S'
        return 'T' if (n <= 128 and k >= 1024 and tiles64 > 256) else 'W'
    if m <= 4096 and k >= 2048:
        return 'W'
    return 'X' if (n <= 256 and k >= 1000) else 'z'


def bf16_branch(m, n, k):
    """-> (kernel, split-K parts) that fgr_gemm_bf16_ws runs for an (m, n, k) product with room
    for the parts: a g5 letter, or 'z64' / 'z128' + ('' | 'scalar') for the register-staged
    gemm_bf16_kernel<64, 64 | 128, k % 8 == 0> (every letter falls to it when k % 8 != 0)."""
    cfg = bf16_tile(m, n, k)
    if cfg != 'z' and k % 8 == 0:
        return cfg, ((4 if k >= 2048 else 2) if splitk_shape(m, n, k) else 1)
    return ('z128' if n >= 128 else 'z64') + ('' if k % 8 == 0 else 'scalar'), 1


# ---------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------
def ln_rows(n, d, seed):
    """(n, d) input rows randn * 2 + 3. Row 0 has mean 1e3: multiples of 1/4 that sum to 1000 d
    exactly, so its mean, centred values and sum of squares are exact in fp32 in any order and
    the row tests the formula (a one-pass variance loses every digit here), not one rounding
    of a mean that the sum|terms| of the backward do not carry. Row n // 2 (n >= 2) is the
    constant 3: variance 0, rstd = eps^-1/2."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(max(n, 1), d, generator=g) * 2 + 3
    zi = np.clip(np.rint(np.random.default_rng(seed).normal(size=d) * 8), -28, 28).astype(np.int64)
    t = int(zi.sum())                      # in quarters; removed by unit steps spread over the row
    np.subtract.at(zi, np.arange(abs(t)) % d, int(np.sign(t)))
    assert zi.sum() == 0 and np.abs(zi).max() <= 36
    x[0] = torch.from_numpy(1000 + zi / 4.0).float()
    if n >= 2:
        x[n // 2] = 3.0
    return x[:n]


def layernorm_bwd(x, gamma, dy, dtype, eps=EPS):
    """-> ((dx, dgamma, dbeta), (their sum|terms|)) of nn.LayerNorm's backward in ``dtype``:
    dxh = dy gamma, dx = rstd (dxh - mean dxh - xh mean(dxh xh))."""
    x, gamma, dy = x.to(dtype), gamma.to(dtype), dy.to(dtype)
    xc = x - x.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps)
    xh, dxh = xc * rstd, dy * gamma
    m2 = (dxh * xh).mean(1, keepdim=True)
    dx = rstd * (dxh - dxh.mean(1, keepdim=True) - xh * m2)
    den = rstd * (dxh.abs() + dxh.abs().mean(1, keepdim=True)
                  + xh.abs() * (dxh * xh).abs().mean(1, keepdim=True))
    return ((dx, (dy * xh).sum(0), dy.sum(0)),
            (den, (dy * xh).abs().sum(0), dy.abs().sum(0)))


# ---------------------------------------------------------------------------------------------
# neighbour-table inverse, max-pool routing
# ---------------------------------------------------------------------------------------------
def nbr_inverse_host(idx, ns):
    """The host's stable inverse of an (nq, width) table (test_gpu_train.test_nbr_inverse):
    -> (start (ns + 1,), ent (valid entries,), pos (nq * width,), -1 for a non-entry), int32.
    An entry is valid when 0 <= idx < ns: the shadow ns, negatives and larger values are not."""
    flat = np.asarray(idx, np.int64).reshape(-1)
    e = np.nonzero((flat >= 0) & (flat < ns))[0]
    order = e[np.argsort(flat[e], kind='stable')]
    cnt = np.bincount(flat[e], minlength=ns)[:ns] if ns else np.zeros(0, np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)])
    pos = np.full(flat.shape, -1)
    pos[order] = np.arange(len(order))
    return start.astype(np.int32), order.astype(np.int32), pos.astype(np.int32)


def max_pool_bwd(x, idx, dy):
    """max_pool's backward restated: the gradient of (query, channel) goes to the row's FIRST
    maximum over x[idx[q, h], c] with shadow entries reading 0; when that first maximum is a
    shadow it goes nowhere. numpy arrays in -> (dx fp64, sum|dy| routed there, dx fp32 summed in
    ascending entry order, number of routed (query, channel) pairs)."""
    ns, c = x.shape
    real = (idx >= 0) & (idx < ns)
    v = np.concatenate([x, np.zeros((1, c), x.dtype)])[np.where(real, idx, ns)]     # (nq, w, c)
    arg = v.argmax(1)                                        # first maximum, (nq, c)
    tgt = np.take_along_axis(idx, arg, 1)
    routed = np.take_along_axis(real, arg, 1)
    qs, chs = np.nonzero(routed)                             # ascending query = ascending entry
    where = (tgt[qs, chs], chs)
    dx64, den, dx32 = np.zeros((ns, c)), np.zeros((ns, c)), np.zeros((ns, c), np.float32)
    np.add.at(dx64, where, dy[qs, chs].astype(np.float64))
    np.add.at(den, where, np.abs(dy[qs, chs]).astype(np.float64))
    np.add.at(dx32, where, dy[qs, chs].astype(np.float32))
    return dx64, den, dx32, len(qs)


def pool_case(c, width, nq=70, ns=90, seed=0):
    """(x (ns, c), idx (nq, width)) holding every tie of the routing rule. Support 7 is exactly
    0.0, support 8 exactly -0.0, supports 9 and 10 are equal and larger than every other row;
    channels 0, 3, 6, .. of every other support are negative. Rows (cut to ``width``):
      0  all shadow                       1  [shadow, 7, 7, ..]: the shadow's 0 comes first
      2  [7, shadow, ..]: the real 0.0 comes first, the gradient flows to 7
      3  [8, shadow, 7, ..]: -0.0 == 0.0, the first entry keeps it
      4  [10, 9, random ..] and 5 [9, 10, random ..]: equal values, the first wins
      6  [11, 12, 11, 12, ..]: the same support named more than once
      7  no shadow at all (negative channels route to a real row)
    the rest random with 30 % shadows."""
    rng = np.random.default_rng(1000 * c + 10 * width + seed)
    x = rng.normal(size=(ns, c)).astype(np.float32)
    x[:, ::3] = -np.abs(x[:, ::3])
    x[7], x[8] = 0.0, -0.0
    x[9] = np.abs(x[9]) + 8
    x[10] = x[9]
    idx = rng.integers(11, ns, (nq, width))
    idx[rng.uniform(size=(nq, width)) < 0.3] = ns
    special = [[ns] * width, [ns] + [7] * width, [7] + [ns] * width, [8, ns] + [7] * width,
               [10, 9] + list(idx[4]), [9, 10] + list(idx[5]), [11, 12] * width,
               list(rng.integers(11, ns, width))]
    for r, row in enumerate(special):
        idx[r] = row[:width]
    return x, idx.astype(np.int64)


# ---------------------------------------------------------------------------------------------
# KPConv scatter
# ---------------------------------------------------------------------------------------------
def scatter(q, s, idx, kp, dwf, cin, influence, aggregation, dtype, absolute=False):
    """dx (ns, cin) of the KPConv gather from d_wf (nq, K * cin): autograd of the restatement
    of tests/_kpconv_modes.py in ``dtype``. absolute: the same code on |d_wf| -- the weights
    are >= 0, so that is sum_entries sum_k w |d_wf|, the sum|terms| of every dx element."""
    x = torch.zeros(s.shape[0], cin, dtype=dtype, requires_grad=True)
    wf, _ = km.gather_ref(q, s, idx, x, kp, km.EXT, influence, aggregation, dtype)
    cot = dwf.detach().cpu().to(dtype)
    (wf.reshape(cot.shape) * (cot.abs() if absolute else cot)).sum().backward()
    return x.grad
