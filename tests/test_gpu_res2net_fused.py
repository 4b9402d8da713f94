"""fgr_res2net_block_h3 / fgr_res2net_block6: the Res2Net bottleneck front (conv1 + hierarchy +
concat) in one launch.

Error convention of test_gpu_dispatch.py: per element |got - ref64| / sum|terms|, held to
<= 4 x the torch fp32 restatement's error + 1e-7 and never above 1e-4. The propagation term of
the hierarchy is extended by conv1:
    Eh_j = |W1_j| |x| + |b1_j|
    E_i  = |W_i| (E_{i-1} + Eh_i) + |b_i|
(ReLU is 1-Lipschitz). The h_{scale-1} columns are held against Eh, the x columns are exact.

Instances (res2net.hip): res2net_block_h3_kernel<2, 1>, <4, 2>, <7, 4> = (w, cin) (28, 32),
(56, 64), (112, 128), all with 32-row blocks; n = 70 is two full blocks and one of 6 rows.
res2net_block6_kernel<14, 8, R> = (224, 256) with R = 16 / 32 / 48 rows per block by
fgr_res2net_chain6's rule: n = 70 -> 16 (4 blocks and one of 6 rows), 4097 -> 32 (the last
block has one row), 8193 -> 48 (171 blocks, the last with 33 rows); the two large cases run
scale 3 (two chained steps) to stay small, as test_gpu_dispatch's do. The f16x3 hierarchy at
width 224 (FGREG_R2N224=h3) has no fused instance and keeps its two launches.
"""
import functools
import math

import pytest
import torch

import model_oracle as mo
from _arena import SENTINEL, Arena, bit_equal
from conftest import rel_err

pytestmark = pytest.mark.gpu
F32 = torch.float32
CAP = 1e-4
TOL = 1e-4                                  # test_gpu_kernels.TOL (module level, vs the oracle)
SCALE = 8
INSTANCES = [(28, 32), (56, 64), (112, 128), (224, 256)]       # 224: block6, else block_h3


def _L():
    from fgreg import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _cond_err(got, ref, den):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == den.shape, (got.shape, ref.shape, den.shape)
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / den.clamp_min(1e-300)).max())


def _hold(what, e, e32):
    print(f'fused-error {what}: kernel {e:.3e} fp32-restatement {e32:.3e}')
    assert e <= min(4 * e32 + 1e-7, CAP), (what, e, e32)


def _block_ref(x, W1, b1, W, b, w, scale, dtype):
    """(cat, sum|terms|) of h = relu(x W1^T + b1), sp_i = relu(W_i (sp_{i-1} + h_i) + b_i),
    cat = [sp_0 .. sp_{scale-2} | h_{scale-1} | x]."""
    x, W1, b1, W, b = (t.to(dtype) for t in (x, W1, b1, W, b))
    h = torch.relu(x @ W1.t() + b1)
    Eh = x.abs() @ W1.abs().t() + b1.abs()
    cols, dens = [], []
    sp = E = None
    for i in range(scale - 1):
        hi, ehi = h[:, i * w:(i + 1) * w], Eh[:, i * w:(i + 1) * w]
        a = hi if i == 0 else sp + hi
        ea = ehi if i == 0 else E + ehi
        sp = torch.relu(a @ W[i].t() + b[i])
        E = ea @ W[i].abs().t() + b[i].abs()
        cols.append(sp)
        dens.append(E)
    lo = (scale - 1) * w
    return torch.cat(cols + [h[:, lo:], x], 1), torch.cat(dens + [Eh[:, lo:], x.abs()], 1)


@functools.lru_cache(maxsize=None)
def _params(w, cin, adversarial=False, scale=SCALE):
    g = torch.Generator().manual_seed(1000 * w + cin)
    W1 = torch.randn(scale * w, cin, generator=g) / math.sqrt(cin)
    b1 = torch.randn(scale * w, generator=g) * 0.1
    W = torch.randn(scale - 1, w, w, generator=g) / math.sqrt(w)
    b = torch.randn(scale - 1, w, generator=g) * 0.1
    if adversarial:                 # input column 0 pushes every pre-activation down
        W1[:, 0] = -W1[:, 0].abs() - 0.5
    return W1, b1, W, b


def _call(gpu, x, params, w, n=None, ld=None, misalign_x=0, expect_ok=True, x6=None,
          poison=False):
    """One ctypes call on arena operands -> (rc, cat view, arena). x6 (default: w == 224)
    selects fgr_res2net_block6; the scale is that of ``params``."""
    import fgreg.ops as ops
    W1, b1, W, b = params
    scale = W.shape[0] + 1
    x6 = (w == 224) if x6 is None else x6
    cin = x.shape[1]
    n = x.shape[0] if n is None else n
    cols = scale * w + cin
    ld = cols if ld is None else ld
    A = Arena(gpu, poison)
    img1, sc1 = ops.res2net_conv1_fragments(W1.to(gpu), scale)
    img, sc = (ops.res2net_fragments3(W.to(gpu)), None) if x6 else ops.res2net_fragments_h3(W.to(gpu))
    X = A.put(x.to(gpu), name='x', misalign=misalign_x)
    I1 = A.bytes(img1.numel() * 2, name='w1_img')
    I1.copy_(img1.reshape(-1).view(torch.uint8))
    I = A.bytes(img.numel() * 2, name='w_img')
    I.copy_(img.reshape(-1).view(torch.uint8))
    S1, B1 = A.put(sc1, name='w1_scale'), A.put(b1.to(gpu), name='b1')
    Bi = A.put(b.reshape(-1).to(gpu), name='bias')
    cat = A.matrix(max(x.shape[0], 1), min(cols, ld), ld, F32, 'out', name='cat',
                   full=expect_ok and n == x.shape[0] and n > 0)
    if x6:
        rc = _L().fgr_res2net_block6(X.data_ptr(), n, w, cin, scale, I1.data_ptr(), S1.data_ptr(),
                                     B1.data_ptr(), I.data_ptr(), Bi.data_ptr(), cat.data_ptr(),
                                     ld, _st())
    else:
        S = A.put(sc.reshape(-1), name='w_scale')
        rc = _L().fgr_res2net_block_h3(X.data_ptr(), n, w, cin, scale, I1.data_ptr(),
                                       S1.data_ptr(), B1.data_ptr(), I.data_ptr(), S.data_ptr(),
                                       Bi.data_ptr(), cat.data_ptr(), ld, _st())
    torch.cuda.synchronize()
    return rc, cat, A


def _untouched(cat):
    return bool((cat.contiguous().view(torch.int32) == SENTINEL).all())


def _check_vs_fp64(gpu, what, x, params, w):
    scale = params[2].shape[0] + 1
    ref, den = _block_ref(x, *params, w, scale, torch.float64)
    e32 = _cond_err(_block_ref(x, *params, w, scale, F32)[0], ref, den)
    rc, cat, A = _call(gpu, x, params, w)
    assert rc == 0, _L().fgr_last_error()
    A.check()
    got = cat.cpu()
    assert torch.equal(got[:, scale * w:].view(torch.int32), x.view(torch.int32))   # x: bit-exact
    lo = (scale - 1) * w
    _hold(what + ' h_last', _cond_err(got[:, lo:lo + w], ref[:, lo:lo + w], den[:, lo:lo + w]), e32)
    _hold(what, _cond_err(got, ref, den), e32)


@pytest.mark.parametrize('w,cin,n,scale', [(28, 32, 70, 8), (56, 64, 70, 8), (112, 128, 70, 8),
                                          (224, 256, 70, 8), (224, 256, 4097, 3),
                                          (224, 256, 8193, 3)])
def test_block_vs_fp64(gpu, w, cin, n, scale):
    """Every shipped instantiation at the smallest n that selects it with a ragged last block
    (module docstring)."""
    import fgreg.ops as ops
    assert ops.res2net_block_supported(w, cin, w != 224)
    g = torch.Generator().manual_seed(w + cin + n)
    x = torch.randn(n, cin, generator=g)
    _check_vs_fp64(gpu, f'block w {w} cin {cin} n {n}', x, _params(w, cin, False, scale), w)


def test_block_h3_adversarial_rows(gpu):
    """(112, 128), n = 70: an all-zero row, a row spanning 1e-30 .. 1e4, a row whose
    pre-activations are all negative (h = 0), a row of denormals."""
    w, cin = 112, 128
    params = _params(w, cin, True)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(70, cin, generator=g)
    x[3] = 0
    sign = torch.where(torch.rand(cin, generator=g) < 0.5, -1.0, 1.0)
    x[40] = sign * 10.0 ** torch.linspace(-30, 4, cin)
    x[41] = 0
    x[41, 0] = 1000.0
    x[69] = sign * torch.linspace(1, 9, cin) * 1e-40
    W1, b1 = params[0], params[1]
    assert bool(((x[41:42].double() @ W1.double().t() + b1.double()) < 0).all())
    assert float(x[69].abs().max()) < 1.2e-38 and float(x[69].abs().min()) > 0
    _check_vs_fp64(gpu, 'block_h3 adversarial', x, params, w)


@pytest.mark.parametrize('w,cin', INSTANCES)
def test_block_footprint(gpu, w, cin):
    """Only cat[:, :scale w + cin] of rows < n is written: with ld_cat larger than needed the
    padding columns and the arena guards keep their sentinels, rows past n too; a poisoned
    arena (NaN around every input) gives the same bits; n = 0 writes nothing."""
    g = torch.Generator().manual_seed(w)
    x = torch.randn(70, cin, generator=g)
    params = _params(w, cin)
    cols = SCALE * w + cin
    rc, cat, A = _call(gpu, x, params, w, ld=cols + 8)
    assert rc == 0
    A.check()
    rc, catp, Ap = _call(gpu, x, params, w, ld=cols + 8, poison=True)    # NaN in every input guard
    assert rc == 0
    Ap.check()
    assert bit_equal(cat, catp)
    rc, cat, A = _call(gpu, x, params, w, n=37, ld=cols + 8)
    assert rc == 0
    A.check()
    assert _untouched(cat[37:]) and not bool(torch.isnan(cat[:37]).any())
    rc, cat, A = _call(gpu, x, params, w, n=0)
    assert rc == 0
    A.check()
    assert _untouched(cat)


def test_block_refusals(gpu):
    """An unsupported (w, cin), a misaligned x and an ld_cat one too small each return
    FGR_E_ARG, write nothing and name the offending value."""
    g = torch.Generator().manual_seed(5)

    def refused(rc, cat, A, *names):
        assert rc == -1, rc                                   # FGR_E_ARG
        A.check()
        assert _untouched(cat)
        msg = _L().fgr_last_error().decode()
        for s in names:
            assert s in msg, (s, msg)

    x = torch.randn(70, 64, generator=g)
    refused(*_call(gpu, x, _params(112, 64), 112, expect_ok=False), 'width 112', 'cin 64')
    x = torch.randn(70, 128, generator=g)
    rc, cat, A = _call(gpu, x, _params(112, 128), 112, misalign_x=4, expect_ok=False)
    xr = [r for r in A.regions if r.name == 'x'][0]
    refused(rc, cat, A, 'x 0x%x' % xr.view.data_ptr())
    need = SCALE * 112 + 128
    refused(*_call(gpu, x, _params(112, 128), 112, ld=need - 1, expect_ok=False),
            f'ld_cat {need - 1}')
    # block6: the same three
    refused(*_call(gpu, x, _params(112, 128), 112, expect_ok=False, x6=True),
            'fgr_res2net_block6', 'width 112', 'cin 128')
    x = torch.randn(20, 256, generator=g)
    p224 = _params(224, 256, False, 3)
    rc, cat, A = _call(gpu, x, p224, 224, misalign_x=8, expect_ok=False)
    xr = [r for r in A.regions if r.name == 'x'][0]
    refused(rc, cat, A, 'fgr_res2net_block6', 'x 0x%x' % xr.view.data_ptr())
    need = 3 * 224 + 256
    refused(*_call(gpu, x, p224, 224, ld=need - 1, expect_ok=False), f'ld_cat {need - 1}')


@functools.lru_cache(maxsize=None)
def _module_case(cin, cout, n):
    from fgreg.backbone import my_Bottle2neck, my_res2Net
    torch.manual_seed(cout)
    m = my_res2Net(my_Bottle2neck, cin, cout, baseWidth=14, scale=8)
    g = torch.Generator().manual_seed(cin)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.75 + 0.5 * torch.rand(mod.running_var.shape, generator=g))
                mod.weight.copy_(1 + 0.1 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = torch.randn(n, cin, generator=g)
    ref = mo.res2net({f'r.{k}': v for k, v in sd.items()}, 'r', x)
    return m, x, ref


@pytest.mark.parametrize('n', [1500, 1501])
@pytest.mark.parametrize('cin,cout', [(128, 512), (256, 1024)])
def test_module_fused_vs_two_launches(gpu, cin, cout, n, monkeypatch):
    """my_res2Net with backbone.R2N_FUSED True and False (randomised BatchNorm state of
    test_gpu_kernels._res2net_case): each path within TOL of the oracle, and the two within
    the sum of their measured errors. (128, 512) runs fgr_res2net_block_h3 (width 112),
    (256, 1024) fgr_res2net_block6 (width 224, 16-row blocks at these row counts)."""
    import fgreg.backbone as bb
    m, x, ref = _module_case(cin, cout, n)
    m = m.to(gpu).eval()
    outs = {}
    with torch.no_grad():
        for fused in (True, False):
            monkeypatch.setattr(bb, 'R2N_FUSED', fused)
            outs[fused] = m(x.to(gpu)).clone()
    ef, eu = rel_err(outs[True], ref), rel_err(outs[False], ref)
    d = rel_err(outs[True], outs[False])
    print(f'fused-module cin {cin} n {n}: fused {ef:.3e} two-launch {eu:.3e} between {d:.3e}')
    assert ef < TOL and eu < TOL
    scale = float(outs[False].abs().max()) / max(float(ref.abs().max()), 1e-30)
    assert d * scale <= ef + eu
