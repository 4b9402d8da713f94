"""tests/_backward_ref.py on the CPU: each restatement that test_gpu_backward.py checks the
kernels with against an independent statement of the same operation (torch fp64 autograd, a
hand-worked table), and the restated bf16 dispatcher against the table of branches that test_gpu_backward.py
relies on."""
import numpy as np
import torch
import torch.nn.functional as F

import _backward_ref as br
import _kpconv_modes as km
import model_oracle as mo


def test_layernorm_bwd_is_autograd():
    for n, d in ((1, 32), (17, 65), (5, 300)):
        x = br.ln_rows(n, d, d).double().requires_grad_(True)
        g = torch.Generator().manual_seed(d)
        gamma = (1 + 0.2 * torch.randn(d, generator=g)).double().requires_grad_(True)
        beta = torch.zeros(d, dtype=torch.float64, requires_grad=True)
        dy = torch.randn(n, d, generator=g).double()
        (F.layer_norm(x, (d,), gamma, beta, br.EPS) * dy).sum().backward()
        (dx, dg, db), (ex, eg, eb) = br.layernorm_bwd(x.detach(), gamma.detach(), dy, torch.float64)
        for got, want, den in ((dx, x.grad, ex), (dg, gamma.grad, eg), (db, beta.grad, eb)):
            # autograd's own fp64 error on the mean-1e3 row is ~1e3 * 2^-53 in xh, also where an
            # exactly centred entry has xh = 0 and therefore no dgamma term at all
            assert bool(((got - want).abs() <= 1e-10 * den + 1e-12).all())
            assert bool((den * (1 + 1e-12) >= got.abs()).all())


def test_ln_rows_special_rows_are_exact_in_fp32():
    for d in (32, 65, 300, 1000, 1024):
        x = br.ln_rows(17, d, d)
        row = x[0]
        sums = [row.sum(), row.flip(0).sum(), row.cumsum(0)[-1], row[::2].sum() + row[1::2].sum()]
        assert all(float(s) == 1000.0 * d for s in sums)          # any order: the mean is exact
        xc = row - 1000
        assert float((xc * xc).sum()) == float((xc.double() ** 2).sum())
        assert 1.0 < float(xc.std()) < 3.0 and float(xc.abs().max()) <= 9
        assert bool((x[8] == 3).all())
        assert abs(float(x[1:8].mean()) - 3) < 0.5
    assert br.ln_rows(0, 64, 1).shape == (0, 64) and br.ln_rows(1, 64, 1).shape == (1, 64)


def test_nbr_inverse_host_by_hand():
    idx = np.array([[2, 0, 3], [0, 0, 7], [-1, 2, 3]])           # ns = 3: 3, 7 and -1 name no row
    start, ent, pos = br.nbr_inverse_host(idx, 3)
    assert start.tolist() == [0, 3, 3, 5]
    assert ent.tolist() == [1, 3, 4, 0, 7]
    assert pos.tolist() == [3, 0, -1, 1, 2, -1, -1, 4, -1]
    start, ent, pos = br.nbr_inverse_host(np.zeros((2, 2), np.int64), 0)
    assert start.tolist() == [0] and len(ent) == 0 and pos.tolist() == [-1] * 4
    start, ent, pos = br.nbr_inverse_host(np.zeros((0, 4), np.int64), 5)
    assert start.tolist() == [0] * 6 and len(ent) == 0 and len(pos) == 0


def test_max_pool_bwd_ties_by_hand():
    x = np.array([[0.0], [-1.0], [5.0], [5.0]], np.float32)      # ns = 4, shadow = 4
    idx = np.array([[4, 0], [0, 4], [1, 4], [0, 0], [3, 2], [2, 3], [4, 4]])
    dy = np.array([[1], [2], [4], [8], [16], [32], [64]], np.float32)
    dx, den, dx32, routed = br.max_pool_bwd(x, idx, dy)
    # row 0: the shadow's 0 first, nothing flows; 1: the real 0.0 first; 2: the shadow beats -1;
    # 3: one support twice, counted once; 4, 5: equal values, the first wins; 6: all shadow
    assert dx[:, 0].tolist() == [10.0, 0.0, 32.0, 16.0] and routed == 4
    assert np.array_equal(dx, den) and np.array_equal(dx32, dx.astype(np.float32))


def test_max_pool_bwd_is_autograd_without_ties():
    rng = np.random.default_rng(3)
    ns, nq, c, w = 40, 30, 5, 6
    x = rng.normal(size=(ns, c)).astype(np.float32)
    idx = rng.integers(0, ns + 1, (nq, w))
    idx[2] = ns
    for r in range(nq):                                          # no support twice in a row
        real = idx[r][idx[r] < ns]
        idx[r][idx[r] < ns] = rng.choice(ns, len(real), replace=False)
    dy = rng.normal(size=(nq, c)).astype(np.float32)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    (mo.max_pool(x64, torch.from_numpy(idx)) * torch.from_numpy(dy).double()).sum().backward()
    dx, den, dx32, _ = br.max_pool_bwd(x, idx, dy)
    assert np.allclose(dx, x64.grad.numpy(), rtol=0, atol=1e-12)
    assert bool((den >= np.abs(dx) - 1e-12).all()) and np.allclose(dx32, dx, atol=1e-5)


def test_pool_case_holds_every_tie():
    for c, width in ((1, 1), (48, 5), (257, 40)):
        x, idx = br.pool_case(c, width)
        ns = x.shape[0]
        assert bool((idx[0] == ns).all()) and idx[1][0] == ns and idx[2][0] == 7 and idx[3][0] == 8
        assert bool((x[7] == 0).all()) and bool(np.signbit(x[8]).all()) and np.array_equal(x[9], x[10])
        assert bool((idx[7] < ns).all())
        if width >= 2:
            assert idx[1][1] == 7 and idx[2][1] == ns and idx[4][:2].tolist() == [10, 9]
            assert idx[5][:2].tolist() == [9, 10] and idx[6][:2].tolist() == [11, 12]
            dy = np.ones((idx.shape[0], c), np.float32)
            dx = br.max_pool_bwd(x, idx, dy)[0]
            # 7 gets row 2 only (never row 1), 8 gets row 3, 10 row 4 and 9 row 5, everywhere
            assert bool((dx[7] == 1).all()) and bool((dx[8] == 1).all())
            assert bool((dx[9] == 1).all()) and bool((dx[10] == 1).all())
        if width >= 4:
            assert idx[6][:4].tolist() == [11, 12, 11, 12]


def test_scatter_is_the_weighted_sum():
    for influence in km.INFLUENCES:
        for aggregation in km.AGGREGATIONS:
            cin, H, n_kp = 3, 7, 15
            q, s, idx, _, kp, _ = km.table(cin, H, n_kp)
            nq, ns = q.shape[0], s.shape[0]
            dwf = torch.randn(nq, n_kp * cin, generator=torch.Generator().manual_seed(1)).double()
            w = km.influences(km.sq_distances(q.double(), s.double(), idx, kp.double()), km.EXT,
                              influence, aggregation)                          # (nq, K, H)
            for absolute in (False, True):
                d3 = (dwf.abs() if absolute else dwf).view(nq, n_kp, cin)
                per = torch.einsum('qkh,qkc->qhc', w, d3).reshape(nq * H, cin)
                want = torch.zeros(ns + 1, cin, dtype=torch.float64).index_add_(0, idx.reshape(-1), per)[:ns]
                got = br.scatter(q, s, idx, kp, dwf, cin, influence, aggregation, torch.float64, absolute)
                assert float((got - want).abs().max()) < 1e-12 * max(1.0, float(want.abs().max()))
            assert bool((got >= br.scatter(q, s, idx, kp, dwf, cin, influence, aggregation,
                                           torch.float64).abs() - 1e-12).all())


def test_bf16_dispatch_and_bounds():
    # the dW GEMM (M = n, N = k, K = rows) of the issue's (rows, n, k) table
    want = {(2048, 64, 128): ('X', 4), (1928, 64, 128): ('S', 2), (2051, 64, 128): ('z128scalar', 1),
            (2052, 64, 64): ('z64scalar', 1), (2056, 256, 1024): ('S', 1),
            (37, 3, 32): ('z64scalar', 1), (300, 1, 256): ('z128scalar', 1)}
    for (rows, n, k), branch in want.items():
        assert br.bf16_branch(n, k, rows) == branch, (rows, n, k)
    assert br.bf16_tile(64, 128, 2051) == 'S' and br.bf16_tile(3, 32, 37) == 'z'
    assert br.bf16_branch(2048, 128, 64) == ('z128', 1) and br.bf16_branch(37, 32, 3) == ('z64scalar', 1)
    assert br.bf16_bound(2056) == (65 + 8) * 2.0 ** -24 < 1e-5 and br.bf16_bound(10 ** 5) == 1e-5
    assert br.f16x3_bound(1) == 3 * 2.0 ** -22 + 9 * 2.0 ** -24
    # round to nearest even at the bf16 rounding point (8 significant bits)
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -7])
    assert br.bf(t).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7]
