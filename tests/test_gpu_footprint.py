"""Memory footprint of the C ABI (include/fgreg.h), called directly through ctypes with every
operand carved out of a guarded arena (tests/_arena.py):

* outputs are strided (ld = cols + 4) with sentinel-filled pad columns and 64 KiB guards: a
  store into column n, row m or past the end is reported; so is an element left unwritten;
* inputs have their pad columns, the rows past the end (x[ns], the neighbour tables' "shadow"
  row) and the guards poisoned with NaN / an out-of-range index;
* workspaces and weight / K-V images are exactly the bytes the library's own size function
  reports, prefilled with 0x00 and with 0xFF (NaN in fp32 / fp16 / bf16).
Each case runs twice (clean and poisoned, run_both) and the two outputs must be bit-identical;
the clean output is then held to the bound of the family's existing value test (2e-6 f16x3
GEMM / FFN, 1e-5 split attention and bf16-vs-rounded-operands, TOL = 1e-4 for the rest).
Undersized workspaces are passed as a smaller NUMBER over a full-size buffer.
"""
import functools
import math

import numpy as np
import pytest
import torch

from _arena import Arena, assert_both_equal, bit_equal, run_both
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
F32, I64, I32 = torch.float32, torch.int64, torch.int32
ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_RELU_RES_LEAKY = 0, 1, 2, 3


def _L():
    from fgreg import _lib
    return _lib.load()


def _ok(rc, name):
    from fgreg import _lib
    _lib.check(rc, name)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _size(fn, *args):
    from fgreg import _lib
    nb = _lib._sz(0)
    _ok(getattr(_L(), fn)(*args, nb), fn)
    return nb.value


def _p(t):
    return None if t is None else t.data_ptr()


def _refused(rc):
    """A refused call: non-zero status and a message in fgr_last_error()."""
    assert rc != 0
    assert len(_L().fgr_last_error()) > 0


def _both(fn, gpu):
    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    return clean


# ---------------------------------------------------------------------------------------------
# a / b / j. dense layers: weight image (exact bytes) -> GEMM (strided, guarded output)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gemm_data(m, n, k):
    g = torch.Generator().manual_seed(m + n + k)
    x = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / math.sqrt(k)
    b = torch.randn(n, generator=g)
    r = torch.randn(m, n, generator=g)
    return x, w, b, r


def _gemm_ref(m, n, k, act, res, bf16=False):
    x, w, b, r = _gemm_data(m, n, k)
    if bf16:
        p = x.bfloat16().double() @ w.bfloat16().double().t() + b.double()
    else:
        p = x.double() @ w.double().t() + b.double()
    if act == ACT_RELU:
        p = p.clamp_min(0)
    if act == ACT_RELU_RES_LEAKY:
        return torch.nn.functional.leaky_relu(p.clamp_min(0) + r.double(), 0.1)
    return p + r.double() if res else p


def _image(arena, w, split='fgr_split_weights_h3', colmajor=False):
    """The split image of w (n, k) in an exact-size scratch view. colmajor: w is stored (k, n),
    element (i, j) at w[j * n + i] (stride_n 1, the KPConv / transposed-activation layout)."""
    n, k = w.shape
    img = arena.bytes(_size(split + '_bytes', n, k), name='w_img')
    if colmajor:
        wd, sn, sk = arena.put(w.t().contiguous(), name='w'), 1, n
    else:
        wd, sn, sk = arena.put(w, name='w'), k, 1
    _ok(getattr(_L(), split)(_p(wd), n, k, sn, sk, _p(img), _st()), split)
    return img


def _gemm(arena, m, n, k, act, res, mode='f16x3', unaligned=False, ws=None, colmajor=False):
    """One fgr_gemm_<mode>[_ws] call. unaligned: the output starts 4 bytes past a 16-B boundary
    with a row stride that is no multiple of 4 (the scalar-store epilogue, vo == 0,
    gemm_f16x3_impl). ws: None (no-workspace entry point) or a byte count relative to
    fgr_gemm_workspace's answer (0 = exactly that, -16 = 16 fewer over the same buffer)."""
    x, w, b, r = _gemm_data(m, n, k)
    a = arena.put(x, ld=k + 4, name='a')
    split = 'fgr_split_weights_h3' if mode == 'f16x3' else 'fgr_split_weights_bf16'
    img = _image(arena, w, split, colmajor)
    bias = arena.put(b, name='bias')
    rr = arena.put(r, ld=n + 8, name='r') if (res or act == ACT_RELU_RES_LEAKY) else None
    ldc = n + 4
    if unaligned:
        ldc = n + 5 if (n + 5) % 4 else n + 6
    c = arena.matrix(m, n, ldc, F32, 'out', name='c', misalign=4 if unaligned else 0)
    args = (_p(a), k + 4, _p(img), _p(c), ldc, _p(bias), _p(rr), n + 8 if rr is not None else 0,
            m, n, k, act)
    if ws is None:
        name = 'fgr_gemm_' + mode
        _ok(getattr(_L(), name)(*args, _st()), name)
    else:
        need = _size('fgr_gemm_workspace', m, n, k, 0 if mode == 'f16x3' else 1)
        assert need > 0, 'shape does not split'
        wsb = arena.bytes(need, name='ws')
        name = 'fgr_gemm_' + mode + '_ws'
        _ok(getattr(_L(), name)(*args, _p(wsb), need + ws, _st()), name)
    return c


RAGGED = [(65, 20, 40), (77, 50, 36), (130, 33, 72)]
EPILOGUES = [(ACT_NONE, True), (ACT_RELU_RES_LEAKY, True)]
TILES = list('befghijklmtuvwxyz') + list('ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789')


@pytest.mark.parametrize('tile', TILES)
def test_gemm_f16x3_tiles_footprint(gpu, tile, monkeypatch):
    """Every f16x3 tile / pipeline variant (FGR_GEMM16_TILE, read per call by h3_tile,
    gemm16.hip) on ragged shapes: (65, 20, 40) two row tiles and a partial column tile,
    (77, 50, 36) K % 8 != 0 -- where every g5 letter runs the k-looped dispatcher's own choice
    (h3_tile_kloop) -- and (130, 33, 72) odd N; bias, residual with ldr = n + 8, plain and
    ReLU-residual-LeakyReLU epilogues; once with 16-B aligned float4 stores and once through
    the scalar-store epilogue."""
    monkeypatch.setenv('FGR_GEMM16_TILE', tile)
    for m, n, k in RAGGED:
        for act, res in EPILOGUES:
            for unaligned in (False, True):
                out = _both(lambda ar: _gemm(ar, m, n, k, act, res, unaligned=unaligned), gpu)
                e = rel_err(out, _gemm_ref(m, n, k, act, res))
                assert e < 2e-6, (tile, m, n, k, act, unaligned, e)


@pytest.mark.parametrize('m,n,k', [(4097, 256, 256), (4097, 512, 256), (4097, 768, 256),
                                   (4097, 1024, 256), (8001, 224, 128), (8001, 640, 256)])
def test_gemm_f16x3_default_dispatch_footprint(gpu, m, n, k, monkeypatch):
    """The default dispatch one ragged row past its thresholds: K = 256 with >= 4096 rows and
    N in {256, 512, 768, 1024} is the weight-split kernel (gemm_ws_supported,
    taken only with FGR_GEMM16_TILE unset, gemm_f16x3_impl; it has the plain / ReLU epilogues
    and the residual add, gemm_ws_f16x3); >= 8000 rows with K <= 128 and N >= 224, or
    N >= 640, is the row-stationary 'z' (h3_tile)."""
    monkeypatch.delenv('FGR_GEMM16_TILE', raising=False)
    for act, res in [(ACT_NONE, True), (ACT_RELU, False)] + ([(ACT_RELU_RES_LEAKY, True)] if m == 8001 else []):
        out = _both(lambda ar: _gemm(ar, m, n, k, act, res), gpu)
        e = rel_err(out, _gemm_ref(m, n, k, act, res))
        assert e < 2e-6, (m, n, k, act, e)


@pytest.mark.parametrize('mode', ['f16x3', 'bf16'])
def test_gemm_splitk_exact_workspace(gpu, mode, monkeypatch):
    """Split-K (2120 x 128 x 1920, splitk_shape via h3_tile_kloop) with exactly
    fgr_gemm_workspace's bytes, 0xFF-prefilled in the poisoned run; and with ws_bytes 16
    smaller, which the header says runs unsplit (gemm_f16x3_impl) -- same contract, so the same
    bound, and the workspace then stays untouched."""
    monkeypatch.delenv('FGR_GEMM16_TILE', raising=False)
    monkeypatch.delenv('FGR_GEMM_BF16_TILE', raising=False)
    m, n, k = 2120, 128, 1920
    bf = mode == 'bf16'
    tol = 1e-5 if bf else 2e-6
    ref = _gemm_ref(m, n, k, ACT_RELU_RES_LEAKY, True, bf16=bf)
    out = _both(lambda ar: _gemm(ar, m, n, k, ACT_RELU_RES_LEAKY, True, mode=mode, ws=0), gpu)
    assert rel_err(out, ref) < tol

    def short(ar):
        c = _gemm(ar, m, n, k, ACT_RELU_RES_LEAKY, True, mode=mode, ws=-16)
        ws = ar.regions[-1].view
        assert ar.regions[-1].name == 'ws'
        torch.cuda.synchronize()
        assert bool((ws == (0xFF if ar.poison else 0)).all()), 'unsplit fallback wrote the workspace'
        return c
    out2 = _both(short, gpu)
    assert rel_err(out2, ref) < tol


@pytest.mark.parametrize('tile', ['', 'z', 'A', 'B', 'I', 'K', 'O', 'D', 'S', 'T', '0', '2', '5'])
def test_gemm_bf16_tiles_footprint(gpu, tile, monkeypatch):
    """fgr_gemm_bf16 over the variants of test_gemm_bf16_rounding_points (FGR_GEMM_BF16_TILE) on
    the ragged shapes of the f16x3 test: vs the bf16-rounded operands in fp64 within 1e-5, vs
    exact fp64 within 1e-2 (that test's bounds)."""
    monkeypatch.setenv('FGR_GEMM_BF16_TILE', tile)
    for m, n, k in RAGGED:
        for act, res in EPILOGUES:
            for unaligned in (False, True):
                out = _both(lambda ar: _gemm(ar, m, n, k, act, res, mode='bf16',
                                             unaligned=unaligned), gpu)
                e = rel_err(out, _gemm_ref(m, n, k, act, res, bf16=True))
                assert e < 1e-5, (tile, m, n, k, act, unaligned, e)
                if act == ACT_NONE:
                    assert rel_err(out, _gemm_ref(m, n, k, act, res)) < 1e-2


@pytest.mark.parametrize('split', ['fgr_split_weights_h3', 'fgr_split_weights_bf16'])
@pytest.mark.parametrize('n,k,colmajor', [(3, 36, False), (17, 8, False), (200, 1000, False),
                                          (33, 1032, False), (33, 1032, True)])
def test_weight_image_exact_bytes(gpu, split, n, k, colmajor, monkeypatch):
    """Weight images in exact-*_bytes scratch views: (3, 36) and (17, 8) partial 16-row panels and
    K-padding, (200, 1000) the largest of the fused split's range (k <= kSplitFusedK = 1024,
    fgr_split_weights_h3), (33, 1032) past it the scale pass + split pass, and with stride_n == 1 the
    column-major scale pass (its k >= 1024 branch). The GEMM
    consuming the image built over 0x00 and over 0xFF bytes must give bit-identical output
    (the arena checks nothing was written past the reported bytes); the image bytes themselves
    are compared too and a difference is reported as don't-care bytes."""
    monkeypatch.delenv('FGR_GEMM16_TILE', raising=False)
    monkeypatch.delenv('FGR_GEMM_BF16_TILE', raising=False)
    mode = 'f16x3' if split.endswith('h3') else 'bf16'
    m = 70
    imgs = []

    def run(ar):
        c = _gemm(ar, m, n, k, ACT_NONE, False, mode=mode, colmajor=colmajor)
        imgs.append([r for r in ar.regions if r.name == 'w_img'][0].view.clone())
        return c
    out = _both(run, gpu)
    e = rel_err(out, _gemm_ref(m, n, k, ACT_NONE, False, bf16=mode == 'bf16'))
    assert e < (2e-6 if mode == 'f16x3' else 1e-5), e
    assert bit_equal(imgs[0], imgs[1]), \
        f'{int((imgs[0] != imgs[1]).sum())} image bytes keep their previous contents'


def test_weight_image_batch_matches_single(gpu):
    """fgr_split_weights_h3_batch over three descriptors into exact-size images: bit-equal to
    fgr_split_weights_h3's, nothing written outside."""
    from fgreg.linear import _DESC
    shapes = [(3, 36), (17, 8), (200, 1000)]

    def run(ar):
        d = np.zeros(len(shapes), dtype=_DESC)
        singles, batch, p0 = [], [], 0
        for i, (n, k) in enumerate(shapes):
            w = _gemm_data(70, n, k)[1]
            singles.append(_image(ar, w))
            wd = ar.put(w, name='w')
            img = ar.bytes(_size('fgr_split_weights_h3_bytes', n, k), name='w_img_b')
            d[i] = (wd.data_ptr(), img.data_ptr(), k, 1, p0, n, k)
            p0 += (n + 15) // 16
            batch.append(img)
        dd = ar.put(torch.frombuffer(bytearray(d.tobytes()), dtype=torch.uint8), name='descs')
        _ok(_L().fgr_split_weights_h3_batch(_p(dd), len(shapes), p0, _st()), 'split_batch')
        torch.cuda.synchronize()
        for s, b in zip(singles, batch):
            assert bit_equal(s, b)
        return torch.cat(batch)
    _both(run, gpu)


# ---------------------------------------------------------------------------------------------
# d. fused feed-forward, correspondence head
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ffn_data(m, f):
    d = 256
    g = torch.Generator().manual_seed(m + f)
    gamma = 1 + 0.2 * torch.randn(d, generator=g)
    beta = 0.2 * torch.randn(d, generator=g)
    w1 = torch.randn(f, d, generator=g) / math.sqrt(d)
    b1 = 0.5 * torch.randn(f, generator=g)
    w2 = torch.randn(d, f, generator=g) / math.sqrt(f)
    b2 = torch.randn(d, generator=g)
    x = 3.0 + 2.0 * torch.randn(m, d, generator=g)
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    a = (xd - mu) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double()
    h = (a @ w1.double().t() + b1.double()).clamp_min(0)
    ref = xd + h @ w2.double().t() + b2.double()
    return x, gamma, beta, w1, b1, w2, b2, ref


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('m,f', [(1, 64), (65, 64), (193, 192)])
def test_ffn_footprint(gpu, m, f, in_place):
    """fgr_ffn_f16x3 (ffn.hip, d = 256) on 1 row, a partial second 64-row block and three blocks
    plus one row with three 64-wide hidden chunks; ldx = ldo = 260, out of place and with
    out == x (x is then an in/out operand whose pad columns must survive)."""
    d, ld = 256, 260
    x, gamma, beta, w1, b1, w2, b2, ref = _ffn_data(m, f)

    def run(ar):
        i1 = _image(ar, w1)
        i2 = _image(ar, w2, 'fgr_split_weights_ffn2')
        bound = ar.put(torch.stack([w1.norm(dim=1).max(), b1.abs().max()]), name='bound')
        ga, be, B1, B2 = (ar.put(t) for t in (gamma, beta, b1, b2))
        if in_place:
            out = xin = ar.matrix(m, d, ld, F32, 'out', name='x_out')
            out.copy_(x)
        else:
            xin = ar.put(x, ld=ld, name='x')
            out = ar.matrix(m, d, ld, F32, 'out', name='out')
        _ok(_L().fgr_ffn_f16x3(_p(xin), ld, _p(ga), _p(be), 1e-5, _p(i1), _p(B1), _p(i2), _p(B2),
                               _p(bound), _p(out), ld, m, d, f, _st()), 'fgr_ffn_f16x3')
        return out
    out = _both(run, gpu)
    e = rel_err(out, ref)
    assert e < 2e-6, e


@pytest.mark.parametrize('m,d', [(97, 64), (333, 128)])
def test_corr_head_footprint(gpu, m, d):
    """fgr_corr_head_f16x3 (two row-stationary launches, gemm16.hip): hidden (m, d) is
    caller scratch of exactly 4 m d bytes, corr (m, 3) and logits (m) contiguous guarded
    outputs, f strided. Bound of test_corr_head_fused_vs_fp64: 1e-5 of each row's
    |.|-weighted magnitude."""
    g = torch.Generator().manual_seed(m + d)
    f = torch.randn(m, d, generator=g) * 0.7
    w0, wc, w2, w4 = (torch.randn(r, d, generator=g) / math.sqrt(d) for r in (d, 1, d, 3))
    b0, bc, b2, b4 = (0.3 * torch.randn(r, generator=g) for r in (d, 1, d, 3))
    w0c = torch.cat([w0, wc, torch.zeros(15, d)])
    b0c = torch.cat([b0, bc, torch.zeros(15)])

    def run(ar):
        i0, i2 = _image(ar, w0c), _image(ar, w2)
        F = ar.put(f, ld=d + 4, name='f')
        hidden = ar.bytes(4 * m * d, name='hidden')
        corr = ar.matrix(m, 3, 3, F32, 'out', name='corr')
        logits = ar.vector(m, F32, 'out', name='logits')
        _ok(_L().fgr_corr_head_f16x3(_p(F), d + 4, m, d, _p(i0), _p(ar.put(b0c)), _p(i2),
                                     _p(ar.put(b2)), _p(ar.put(w4)), _p(ar.put(b4)), _p(hidden),
                                     _p(corr), _p(logits), _st()), 'fgr_corr_head_f16x3')
        return corr, logits
    corr, logits = _both(run, gpu)
    x = f.double()
    h = torch.relu(x @ w0.double().t() + b0.double())
    h2 = torch.relu(h @ w2.double().t() + b2.double())
    c64 = h2 @ w4.double().t() + b4.double()
    l64 = (x @ wc.double().t() + bc.double())[:, 0]
    den_c = (h2.abs() @ w4.double().abs().t()).max(1, keepdim=True).values + 1e-30
    den_l = (x.abs() @ wc.double().abs().t())[:, 0] + 1e-30
    ec = float(((corr.double().cpu() - c64).abs() / den_c).max())
    el = float(((logits.double().cpu() - l64).abs() / den_l).max())
    assert ec < 1e-5 and el < 1e-5, (ec, el)


# ---------------------------------------------------------------------------------------------
# e. attention
# ---------------------------------------------------------------------------------------------
QLENS, KLENS, KV_SEG = [300, 1, 64, 129], [65, 700, 1, 128], [1, 0, 3, 2]


def _attn_ref(q, k, v, qlens, klens, kv_seg, nhead):
    d = q.shape[1]
    dh = d // nhead
    qo, ko = np.cumsum([0] + qlens), np.cumsum([0] + klens)
    out = torch.zeros_like(q)
    for i in range(len(qlens)):
        j = kv_seg[i]
        qs = q[qo[i]:qo[i + 1]].view(-1, nhead, dh).transpose(0, 1) * math.sqrt(1.0 / dh)
        ks = k[ko[j]:ko[j + 1]].view(-1, nhead, dh).transpose(0, 1)
        vs = v[ko[j]:ko[j + 1]].view(-1, nhead, dh).transpose(0, 1)
        out[qo[i]:qo[i + 1]] = (torch.softmax(qs @ ks.transpose(1, 2), -1) @ vs).transpose(0, 1).reshape(-1, d)
    return out


@functools.lru_cache(maxsize=None)
def _attn_data(nhead, d):
    rng = np.random.default_rng(7 + d + nhead)
    q = torch.from_numpy(rng.normal(size=(sum(QLENS), d)))
    k = torch.from_numpy(rng.normal(size=(sum(KLENS), d)))
    v = torch.from_numpy(rng.normal(size=(sum(KLENS), d)))
    return q, k, v, _attn_ref(q, k, v, QLENS, KLENS, KV_SEG, nhead)


def _attn_operands(ar, nhead, d):
    q, k, v, _ = _attn_data(nhead, d)
    ld = d + 4
    Q, K, V = (ar.put(t.float(), ld=ld, name=nm) for t, nm in ((q, 'q'), (k, 'k'), (v, 'v')))
    o = ar.matrix(sum(QLENS), d, ld, F32, 'out', name='o')
    off = lambda lens: torch.tensor(np.cumsum([0] + lens), dtype=I64)
    qo, ko = ar.put(off(QLENS), name='q_off'), ar.put(off(KLENS), name='kv_off')
    seg = ar.put(torch.tensor(KV_SEG, dtype=I32), name='kv_seg')
    return Q, K, V, o, qo, ko, seg, ld


def _attn_split(ar, name, nhead, d, short=0):
    Q, K, V, o, qo, ko, seg, ld = _attn_operands(ar, nhead, d)
    need = _size(name + '_workspace', sum(KLENS), len(KLENS), nhead)
    ws = ar.bytes(need, name='ws')
    rc = getattr(_L(), name)(_p(Q), ld, _p(K), ld, _p(V), ld, _p(o), ld, _p(qo), _p(ko), _p(seg),
                             len(QLENS), len(KLENS), sum(KLENS), max(QLENS), max(KLENS), nhead,
                             d // nhead, math.sqrt(nhead / d), _p(ws), need - short, _st())
    return rc, o, ws


@pytest.mark.parametrize('d', [256, 512])
def test_attention_f16x3_footprint(gpu, d):
    """fgr_attention_f16x3 (attention_f16x3_impl, head dim 32 / 64) on the segment sets of
    test_attention_split_is_fp32_accurate (partial and 1-key tiles, key segments != query
    segments), ld = d + 4, the workspace exactly fgr_attention_f16x3_workspace bytes: 1e-5 vs
    fp64."""
    def run(ar):
        rc, o, _ = _attn_split(ar, 'fgr_attention_f16x3', 8, d)
        _ok(rc, 'fgr_attention_f16x3')
        return o
    out = _both(run, gpu)
    assert rel_err(out.double(), _attn_data(8, d)[3]) < 1e-5


@pytest.mark.parametrize('d', [256, 512])
def test_attention_bf16_footprint(gpu, d):
    """fgr_attention_bf16 (bf16.hip), same cases; test_attention_bf16's bound vs exact fp64
    at O(1) scores: 1e-2."""
    def run(ar):
        rc, o, _ = _attn_split(ar, 'fgr_attention_bf16', 8, d)
        _ok(rc, 'fgr_attention_bf16')
        return o
    out = _both(run, gpu)
    assert rel_err(out.double(), _attn_data(8, d)[3]) < 1e-2


@pytest.mark.parametrize('name', ['fgr_attention_f16x3', 'fgr_attention_bf16'])
def test_attention_refuses_short_workspace(gpu, name):
    """ws_bytes 16 below the kernel's own need (head dim 64, where fgr_*_workspace reports
    exactly that) is refused before the first launch (attention_f16x3_impl, fgr_attention_bf16):
    non-zero status, a message, output and workspace untouched."""
    ar = Arena(gpu, poison=True)
    rc, o, ws = _attn_split(ar, name, 8, 512, short=16)
    torch.cuda.synchronize()
    _refused(rc)
    for r in ar.regions:
        r.full = False
    ar.check()
    assert bool(torch.isnan(o).all()) and bool((ws == 0xFF).all())


@pytest.mark.parametrize('nhead,d', [(2, 16), (1, 256)])
def test_attention_fp32_footprint(gpu, nhead, d):
    """fgr_attention (attention.hip, the any-head-dim fp32 MFMA kernel) at head dim 8 and 256."""
    def run(ar):
        Q, K, V, o, qo, ko, seg, ld = _attn_operands(ar, nhead, d)
        _ok(_L().fgr_attention(_p(Q), ld, _p(K), ld, _p(V), ld, _p(o), ld, _p(qo), _p(ko), _p(seg),
                               len(QLENS), max(QLENS), nhead, d // nhead, math.sqrt(nhead / d),
                               _st()), 'fgr_attention')
        return o
    out = _both(run, gpu)
    assert rel_err(out.double(), _attn_data(nhead, d)[3]) < TOL


# ---------------------------------------------------------------------------------------------
# f. norms and small ops
# ---------------------------------------------------------------------------------------------
def _instnorm_ref(x, lens):
    out = torch.empty_like(x)
    o = 0
    for n in lens:
        s = x[o:o + n]
        out[o:o + n] = (s - s.mean(0)) / torch.sqrt(s.var(0, unbiased=False) + 1e-5)
        o += n
    return out


def _instnorm_call(ar, x, div, res, lens, short=0):
    n, c = x.shape
    need = _size('fgr_instnorm_workspace', max(lens), c, len(lens))
    X, D, R = ar.put(x, name='x'), ar.put(div, name='row_div'), ar.put(res, name='residual')
    off = ar.put(torch.tensor(np.cumsum([0] + lens), dtype=I64), name='seg_off')
    out = ar.matrix(n, c, c, F32, 'out', name='out')
    ws = ar.bytes(need, name='ws') if need else None
    rc = _L().fgr_instnorm(_p(X), n, c, _p(off), len(lens), max(lens), _p(D), 1e-5, ACT_NONE, _p(R),
                           ACT_LEAKY, _p(out), _p(ws), need - short, _st())
    return rc, out, ws, need


@pytest.mark.parametrize('lens,c', [([700, 1, 33, 512], 72), ([1025, 2], 64)])
def test_instnorm_footprint(gpu, lens, c):
    """fgr_instnorm with row_div and residual: [700, 1, 33, 512] x 72 is the one-launch register
    path (segments <= kSegRows = 1024, fgr_instnorm; no workspace), [1025, 2] x 64 one row past
    it the three-launch long-segment path (ls_ok) over exactly
    fgr_instnorm_workspace bytes."""
    rng = np.random.default_rng(5)
    n = sum(lens)
    x = torch.from_numpy(rng.normal(2.0, 3.0, (n, c)).astype(np.float32))
    div = torch.from_numpy(rng.integers(1, 9, n).astype(np.float32))
    res = torch.from_numpy(rng.normal(size=(n, c)).astype(np.float32))
    ref = torch.nn.functional.leaky_relu(
        _instnorm_ref(x.double() / div.double()[:, None], lens) + res.double(), 0.1)

    def run(ar):
        rc, out, ws, need = _instnorm_call(ar, x, div, res, lens)
        assert (need > 0) == (max(lens) > 1024)
        _ok(rc, 'fgr_instnorm')
        return out
    out = _both(run, gpu)
    assert rel_err(out, ref) < TOL


def test_instnorm_refuses_short_workspace(gpu):
    """The long-segment path checks ws_bytes before its first launch (fgr_instnorm)."""
    lens, c = [1025, 2], 64
    n = sum(lens)
    ar = Arena(gpu, poison=True)
    rc, out, ws, need = _instnorm_call(ar, torch.randn(n, c), torch.ones(n), torch.zeros(n, c),
                                       lens, short=16)
    torch.cuda.synchronize()
    _refused(rc)
    for r in ar.regions:
        r.full = False
    ar.check()
    assert bool(torch.isnan(out).all()) and bool((ws == 0xFF).all())


@pytest.mark.parametrize('d', [32, 96, 256])
def test_layernorm_footprint(gpu, d):
    """fgr_layernorm with add and pre_bias (x is a documented in/out: x += pre_bias) at 67 rows:
    d = 32 layernorm_kernel<1>, 96 layernorm_kernel<4>, 256 the vector path
    layernorm_lpr_kernel<32, 2> (fgr_layernorm); 67 rows leave the last 8- / 4-row block
    partial. fgr_layernorm_dual on the same rows."""
    n = 67
    g = torch.Generator().manual_seed(d)
    x = 1 + 2 * torch.randn(n, d, generator=g)
    w, b, pb = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g), torch.randn(d, generator=g)
    w2, b2 = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    a = torch.randn(n, d, generator=g)
    xd = x.double() + pb.double()
    ln = lambda t, ww, bb: torch.nn.functional.layer_norm(t, (d,), ww.double(), bb.double(), 1e-5)

    def run(ar):
        X = ar.matrix(n, d, d, F32, 'out', name='x_inout')
        X.copy_(x)
        out = ar.matrix(n, d, d, F32, 'out', name='out')
        _ok(_L().fgr_layernorm(_p(X), n, d, _p(ar.put(w)), _p(ar.put(b)), 1e-5, _p(ar.put(a, name='add')),
                               _p(ar.put(pb)), _p(out), _st()), 'fgr_layernorm')
        o1 = ar.matrix(n, d, d, F32, 'out', name='dual_out')
        o2 = ar.matrix(n, d, d, F32, 'out', name='dual_out2')
        X2 = ar.put(x, name='x')
        _ok(_L().fgr_layernorm_dual(_p(X2), n, d, _p(ar.put(w)), _p(ar.put(b)), None, _p(o1),
                                    _p(ar.put(w2)), _p(ar.put(b2)), _p(ar.put(a, name='add2')),
                                    _p(o2), 1e-5, _st()), 'fgr_layernorm_dual')
        return X, out, o1, o2
    X, out, o1, o2 = _both(run, gpu)
    assert rel_err(X, xd) < 1e-7
    assert rel_err(out, ln(xd, w, b) + a.double()) < TOL
    assert rel_err(o1, ln(x.double(), w, b)) < TOL
    assert rel_err(o2, ln(x.double(), w2, b2) + a.double()) < TOL


def test_add_footprint(gpu):
    """fgr_add over 1027 floats (one past a float4 multiple and past 1024)."""
    n = 1027
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)

    def run(ar):
        out = ar.vector(n, F32, 'out', name='out')
        _ok(_L().fgr_add(_p(ar.put(a, name='a')), _p(ar.put(b, name='b')), n, _p(out), _st()), 'fgr_add')
        return out
    assert torch.equal(_both(run, gpu).cpu(), a + b)


@pytest.mark.parametrize('d', [32, 256])
def test_sine_pos_embed_footprint(gpu, d):
    """fgr_sine_pos_embed at 67 rows (a partial last row block); d = 32 leaves 2 trailing
    zero-padded columns (d - 3 * npf), 256 leaves 4 (position_embedding.py:29-49)."""
    import model_oracle as mo
    n = 67
    xyz = torch.randn(n, 3, generator=torch.Generator().manual_seed(d))

    def run(ar):
        out = ar.matrix(n, d, d, F32, 'out', name='out')
        _ok(_L().fgr_sine_pos_embed(_p(ar.put(xyz, name='xyz')), n, d, 10000.0, 2 * math.pi, _p(out),
                                    _st()), 'fgr_sine_pos_embed')
        return out
    assert rel_err(_both(run, gpu), mo.sine_pos_embed(xyz, d)) < TOL


@pytest.mark.parametrize('n', [1, 65])
def test_lengths_to_offsets_footprint(gpu, n):
    lens = torch.arange(3, 3 + n, dtype=I64)

    def run(ar):
        out = ar.vector(n + 1, I64, 'out', name='offsets')
        _ok(_L().fgr_lengths_to_offsets(_p(ar.put(lens, name='lengths')), n, _p(out), _st()),
            'fgr_lengths_to_offsets')
        return out
    out = _both(run, gpu)
    assert torch.equal(out.cpu(), torch.cat([torch.zeros(1, dtype=I64), lens.cumsum(0)]))


# ---------------------------------------------------------------------------------------------
# g. KPConv gather, max pool: the shadow row x[ns] / s[ns] is the poisoned tail guard
# ---------------------------------------------------------------------------------------------
def _table(rng, nq, ns, H):
    idx = rng.integers(0, ns, (nq, H))
    idx[rng.uniform(size=(nq, H)) < 0.25] = ns                # shadows
    idx[3] = ns                                               # whole shadow rows
    idx[nq - 1] = ns
    return torch.from_numpy(idx)


@pytest.mark.parametrize('H', [7, 50])
@pytest.mark.parametrize('cin', [1, 16, 32, 64, 128])
def test_kpconv_gather_footprint(gpu, cin, H):
    """fgr_kpconv_gather at 300 queries over 257 supports: cin 1 the stem kernel, 16 / 32 the
    quad-lane kernels, 64 / 128 the wide kernels (fgr_kpconv_gather); H = 7 and 50. A quarter of
    the table is the shadow index ns; the supports and features end exactly at row ns, so s[ns]
    and x[ns] are NaN in the poisoned run: "the shadow row is never read" is the bit-equality.
    fgr_kpconv_gather_workspace reports 0 bytes (kpconv.hip), so no workspace is passed."""
    nq, ns, n_kp, ext = 300, 257, 15, 0.5
    rng = np.random.default_rng(cin + H)
    s = rng.uniform(-1, 1, (ns, 3)).astype(np.float32)
    q = (s[rng.choice(ns, nq, replace=True)] + rng.normal(0, 0.01, (nq, 3))).astype(np.float32)
    idx = _table(rng, nq, ns, H)
    x = torch.from_numpy(rng.normal(size=(ns, cin)).astype(np.float32))
    kp = torch.from_numpy((rng.normal(size=(n_kp, 3)) * 0.3).astype(np.float32))
    s, q = torch.from_numpy(s), torch.from_numpy(q)
    assert _size('fgr_kpconv_gather_workspace', ns, cin) == 0

    def run(ar):
        wf = ar.matrix(nq, n_kp * cin, n_kp * cin, F32, 'out', name='wf')
        nn_ = ar.vector(nq, F32, 'out', name='nnorm')
        _ok(_L().fgr_kpconv_gather(_p(ar.put(q, name='q')), _p(ar.put(s, name='s')), nq, ns,
                                   _p(ar.put(idx, name='idx')), H, _p(ar.put(x, name='x')), cin,
                                   _p(ar.put(kp, name='kp')), n_kp, ext, _p(wf), _p(nn_), None, 0,
                                   _st()), 'fgr_kpconv_gather')
        return wf, nn_
    wf, nn_ = _both(run, gpu)
    sp = torch.cat([s, torch.zeros(1, 3) + 1e6])
    nb = sp[idx] - q.unsqueeze(1)
    d2 = ((nb.unsqueeze(2) - kp) ** 2).sum(3)
    w = torch.clamp(1 - torch.sqrt(d2) / ext, min=0).transpose(1, 2)
    nx = torch.cat([x, torch.zeros(1, cin)])[idx]
    assert rel_err(wf.view(nq, n_kp, cin), torch.matmul(w, nx)) < TOL
    assert torch.equal(nn_.cpu(), torch.clamp((nx.sum(-1) > 0).sum(-1), min=1).float())


@pytest.mark.parametrize('c', [33, 64])
def test_max_pool_footprint(gpu, c):
    """fgr_max_pool: c = 33 the per-element kernel, 64 the wave-per-row kernel (kpconv.hip);
    shadow entries read as 0, never x[ns]."""
    nq, ns, H = 300, 257, 9
    rng = np.random.default_rng(c)
    idx = _table(rng, nq, ns, H)
    x = torch.from_numpy(rng.normal(size=(ns, c)).astype(np.float32))

    def run(ar):
        out = ar.matrix(nq, c, c, F32, 'out', name='out')
        _ok(_L().fgr_max_pool(_p(ar.put(x, name='x')), ns, c, _p(ar.put(idx, name='idx')), nq, H,
                              _p(out), _st()), 'fgr_max_pool')
        return out
    out = _both(run, gpu)
    ref = torch.cat([x, torch.zeros(1, c)])[idx].max(1).values
    assert torch.equal(out.cpu(), ref)


# ---------------------------------------------------------------------------------------------
# c. fused transformer GEMMs
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ln_data(m, n, k):
    g = torch.Generator().manual_seed(m + n + k)
    x = 3.0 + 2.0 * torch.randn(m, k, generator=g)
    x[7] = 0.0                                   # constant rows: var 0
    x[8] = 5.0
    gam, bet = 1 + 0.2 * torch.randn(k, generator=g), 0.2 * torch.randn(k, generator=g)
    gam2, bet2 = 1 + 0.3 * torch.randn(k, generator=g), 0.3 * torch.randn(k, generator=g)
    pos = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / math.sqrt(k)
    b = torch.randn(n, generator=g)
    ln = lambda ga, be: torch.nn.functional.layer_norm(x.double(), (k,), ga.double(), be.double(), 1e-5)
    y = (ln(gam, bet) + pos.double()) @ w.double().t() + b.double()
    return x, gam, bet, gam2, bet2, pos, w, b, y, ln(gam2, bet2)


@pytest.mark.parametrize('m,n,k', [(4097, 768, 256), (8001, 640, 256)])
@pytest.mark.parametrize('side', [False, True])
def test_gemm_ln_footprint(gpu, m, n, k, side, monkeypatch):
    """fgr_gemm_f16x3_ln / _ln_out2 one ragged row past the smallest supported row counts:
    4097 x 768 x 256 the weight-split kernel with the LN prologue (gemm_ws_ln_supported),
    8001 x 640 x 256 the row-stationary one (h3_tile 'z');
    x, add, c and out2 strided by + 4. 1e-5 vs fp64 (test_gemm_ln_vs_fp64), the side output
    1e-6 (test_ln_qkv_images_vs_two_launch_path)."""
    monkeypatch.delenv('FGR_GEMM16_TILE', raising=False)
    assert _L().fgr_gemm_f16x3_ln_supported(m, n, k)
    x, gam, bet, gam2, bet2, pos, w, b, y, ref2 = _ln_data(m, n, k)

    def run(ar):
        img = _image(ar, w)
        X, P = ar.put(x, ld=k + 4, name='x'), ar.put(pos, ld=k + 4, name='add')
        c = ar.matrix(m, n, n + 4, F32, 'out', name='c')
        head = (_p(X), k + 4, _p(ar.put(gam)), _p(ar.put(bet)), 1e-5, _p(P), k + 4, _p(img), _p(c),
                n + 4, _p(ar.put(b)), m, n, k, ACT_NONE)
        if not side:
            _ok(_L().fgr_gemm_f16x3_ln(*head, _st()), 'fgr_gemm_f16x3_ln')
            return c
        out2 = ar.matrix(m, k, k + 4, F32, 'out', name='out2')
        _ok(_L().fgr_gemm_f16x3_ln_out2(*head, _p(ar.put(gam2)), _p(ar.put(bet2)), _p(out2), k + 4,
                                        _st()), 'fgr_gemm_f16x3_ln_out2')
        return c, out2
    out = _both(run, gpu)
    if side:
        assert rel_err(out[1], ref2) < 1e-6
        out = out[0]
    assert rel_err(out, y) < 1e-5


def _attn64(qkv, d, nh, lens, kv):
    dh = d // nh
    offs = np.cumsum([0] + lens)
    outs = []
    for i in range(len(lens)):
        j = kv[i]
        q = qkv[offs[i]:offs[i + 1], :d].reshape(-1, nh, dh).transpose(0, 1) / math.sqrt(dh)
        k = qkv[offs[j]:offs[j + 1], d:2 * d].reshape(-1, nh, dh).transpose(0, 1)
        v = qkv[offs[j]:offs[j + 1], 2 * d:].reshape(-1, nh, dh).transpose(0, 1)
        outs.append((torch.softmax(q @ k.transpose(1, 2), -1) @ v).transpose(0, 1).reshape(-1, d))
    return torch.cat(outs, 0)


def _attend_img(ar, fn, q, ld_q, img, lens, kv, n, d, nh):
    o = ar.matrix(n, d, d + 4, F32, 'out', name='o')
    off = ar.put(torch.tensor(np.cumsum([0] + lens), dtype=I64), name='off')
    seg = ar.put(torch.tensor(kv, dtype=I32), name='kv_seg')
    _ok(getattr(_L(), fn)(_p(q), ld_q, _p(img), n, _p(o), d + 4, _p(off), _p(off), _p(seg),
                          len(lens), max(lens), nh, d // nh, math.sqrt(nh / d), _st()), fn)
    return o


def test_gemm_ln_qkv_footprint(gpu, monkeypatch):
    """fgr_gemm_f16x3_ln_qkv at 4097 rows (d 256, 8 heads of 32: the weight-split kernel's K / V
    image epilogue, gemm_ws_f16x3) into an exact-fgr_kv_image_bytes scratch view, with the
    side output; the images are checked by feeding them to fgr_attention_f16x3_img: its output
    is bit-equal between the clean and the 0xFF-prefilled run and within 1e-5 of fp64. Segments
    start inside 64-row tiles (incl. a 1-row cloud); the last tile holds 1 row."""
    monkeypatch.delenv('FGR_GEMM16_TILE', raising=False)
    m, d, nh = 4097, 256, 8
    lens, kv = [1500, 1, 1100, 1496], [2, 3, 0, 1]
    assert _L().fgr_gemm_f16x3_ln_qkv_supported(m, d, nh)
    x, gam, bet, gam2, bet2, pos, w, b, y, ref2 = _ln_data(m, 3 * d, d)

    def run(ar):
        img = _image(ar, w)
        X, P = ar.put(x, ld=d + 4, name='x'), ar.put(pos, ld=d + 4, name='add')
        q = ar.matrix(m, d, d + 4, F32, 'out', name='q')
        out2 = ar.matrix(m, d, d + 4, F32, 'out', name='out2')
        kvi = ar.bytes(_size('fgr_kv_image_bytes', m, nh, d // nh), name='kv_img')
        _ok(_L().fgr_gemm_f16x3_ln_qkv(_p(X), d + 4, _p(ar.put(gam)), _p(ar.put(bet)), 1e-5, _p(P),
                                       d + 4, _p(img), _p(q), d + 4, _p(ar.put(b)), m, d, nh,
                                       _p(kvi), _p(ar.put(gam2)), _p(ar.put(bet2)), _p(out2), d + 4,
                                       _st()), 'fgr_gemm_f16x3_ln_qkv')
        return _attend_img(ar, 'fgr_attention_f16x3_img', q, d + 4, kvi, lens, kv, m, d, nh), q, out2
    o, q, out2 = _both(run, gpu)
    assert rel_err(q, y[:, :d]) < 1e-5 and rel_err(out2, ref2) < 1e-6
    assert rel_err(o, _attn64(y, d, nh, lens, kv)) < 1e-5


@pytest.mark.parametrize('mode', ['f16x3', 'bf16'])
def test_gemm_qkv_dh64_footprint(gpu, mode, monkeypatch):
    """fgr_gemm_f16x3_qkv / fgr_gemm_bf16_qkv (head dim 64: the staged 64 x 128 g5 epilogue,
    gemm16.hip / bf16.hip) at m = 130, d = 128, 2 heads: three row tiles, the last with
    2 rows, segments [65, 1, 64] crossing tiles; K / V images in exact fgr_kv_image[_bf16]_bytes
    views, consumed by fgr_attention_f16x3_img / _bf16_img. 1e-5 vs fp64 (f16x3,
    test_qkv_images_dh64_vs_two_launch_path), 1e-2 (bf16, test_bf16_qkv_images_vs_two_launch_path)."""
    monkeypatch.delenv('FGR_GEMM16_TILE', raising=False)
    monkeypatch.delenv('FGR_GEMM_BF16_TILE', raising=False)
    m, d, nh = 130, 128, 2
    lens, kv = [65, 1, 64], [2, 0, 1]
    g = torch.Generator().manual_seed(m)
    h = torch.randn(m, d, generator=g) * 1.5
    w = torch.randn(3 * d, d, generator=g) / math.sqrt(d)
    b = torch.randn(3 * d, generator=g)
    f16 = mode == 'f16x3'
    names = (('fgr_split_weights_h3', 'fgr_kv_image_bytes', 'fgr_gemm_f16x3_qkv', 'fgr_attention_f16x3_img')
             if f16 else ('fgr_split_weights_bf16', 'fgr_kv_image_bf16_bytes', 'fgr_gemm_bf16_qkv',
                          'fgr_attention_bf16_img'))
    assert getattr(_L(), names[2] + '_supported')(m, d, nh)

    def run(ar):
        img = _image(ar, w, names[0])
        H = ar.put(h, ld=d + 4, name='a')
        q = ar.matrix(m, d, d + 4, F32, 'out', name='q')
        kvi = ar.bytes(_size(names[1], m, nh, d // nh), name='kv_img')
        _ok(getattr(_L(), names[2])(_p(H), d + 4, _p(img), _p(q), d + 4, _p(ar.put(b)), m, d, nh,
                                    _p(kvi), _st()), names[2])
        o = _attend_img(ar, names[3], q, d + 4, kvi, lens, kv, m, d, nh)
        # the unfused in_proj of the same operands: the fp32 q | k | v the images stand for
        full = ar.matrix(m, 3 * d, 3 * d + 4, F32, 'out', name='qkv')
        gemm = 'fgr_gemm_f16x3' if f16 else 'fgr_gemm_bf16'
        _ok(getattr(_L(), gemm)(_p(H), d + 4, _p(img), _p(full), 3 * d + 4, _p(ar.put(b)), None, 0,
                                m, 3 * d, d, ACT_NONE, _st()), gemm)
        return o, q, full
    o, q, full = _both(run, gpu)
    if f16:
        qkv = h.double() @ w.double().t() + b.double()
        assert rel_err(q, qkv[:, :d]) < 1e-5
        assert rel_err(o, _attn64(qkv, d, nh, lens, kv)) < 1e-5
    else:
        # as test_bf16_qkv_images_vs_two_launch_path: the fp64 attention of the bf16 in_proj's own
        # fp32 output (the exact chain would add the GEMM's bf16 error, amplified by the softmax);
        # q against the bf16-rounded operands in fp64 (test_gemm_bf16_rounding_points)
        qr = h.bfloat16().double() @ w.bfloat16().double().t() + b.double()
        assert rel_err(q, qr[:, :d]) < 1e-5
        assert rel_err(o, _attn64(full.double().cpu(), d, nh, lens, kv)) < 1e-2


# ---------------------------------------------------------------------------------------------
# h. Res2Net chains
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 65, 150])
@pytest.mark.parametrize('kind,w', [('h3', 28), ('h3', 56), ('h3', 112), ('h3', 224), ('x6', 112),
                                    ('x6', 224)])
def test_res2net_chain_footprint(gpu, kind, w, n):
    """fgr_res2net_chain_h3 (16-column tile counts 2 / 4 / 7 / 14, res2net.hip; width 28 pads
    its last tile) and fgr_res2net_chain6 (112, 224; 16-row blocks below 32 rows at 224,
    FGR_R2N_ROWS) at 1 row, 65 (a 1-row last block) and 150 rows; scale 8, cin 32, the
    fragment images and scales in exact-size views, ld_cat = scale w + cin + 4: nothing past
    column scale w + cin of cat is written. TOL vs fp64 (test_res2net_block_vs_oracle)."""
    from fgreg import ops
    assert ops.res2net_chain_supported(w, h3=kind == 'h3')
    scale, cin = 8, 32
    g = torch.Generator().manual_seed(w + n)
    W = torch.randn(scale - 1, w, w, generator=g) / math.sqrt(w)
    bias = 0.2 * torch.randn(scale - 1, w, generator=g)
    h = torch.randn(n, scale * w, generator=g)
    x = torch.randn(n, cin, generator=g)
    sp, parts = torch.zeros(n, w, dtype=torch.float64), []
    for i in range(scale - 1):
        sp = torch.relu((sp + h[:, i * w:(i + 1) * w].double()) @ W[i].double().t() + bias[i].double())
        parts.append(sp)
    ref = torch.cat(parts + [h[:, (scale - 1) * w:].double(), x.double()], 1)
    if kind == 'h3':
        frag, wsc = ops.res2net_fragments_h3(W.to(gpu))
    else:
        frag, wsc = ops.res2net_fragments3(W.to(gpu)), None
    frag = frag.contiguous().view(-1).view(torch.uint8).cpu()
    width = scale * w + cin
    ld = width + 4

    def run(ar):
        F = ar.put(frag, name='w_img')
        cat = ar.matrix(n, width, ld, F32, 'out', name='cat')
        H, X, Bi = ar.put(h, name='h'), ar.put(x, name='x'), ar.put(bias.reshape(-1), name='bias')
        if kind == 'h3':
            S = ar.put(wsc.cpu().reshape(-1), name='w_scale')
            _ok(_L().fgr_res2net_chain_h3(_p(H), n, w, scale, _p(F), _p(S), _p(Bi), _p(X), cin,
                                          _p(cat), ld, _st()), 'fgr_res2net_chain_h3')
        else:
            _ok(_L().fgr_res2net_chain6(_p(H), n, w, scale, _p(F), _p(Bi), _p(X), cin, _p(cat), ld,
                                        _st()), 'fgr_res2net_chain6')
        return cat
    assert rel_err(_both(run, gpu), ref) < TOL


# ---------------------------------------------------------------------------------------------
# i. geometry
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clouds():
    rng = np.random.default_rng(0)
    P = np.concatenate([rng.uniform(-1, 1, (n, 3)).astype(np.float32) for n in (300, 1, 65)])
    return P, [300, 1, 65]


def _cloud_ops(ar):
    P, lens = _clouds()
    pts = ar.put(torch.from_numpy(P), name='points')
    off = ar.put(torch.tensor(np.cumsum([0] + lens), dtype=I64), name='off')
    return P, lens, pts, off


def test_grid_subsample_footprint(gpu):
    """fgr_grid_subsample_count / _fill over three clouds of 300, 1 and 65 points in exactly
    fgr_grid_subsample_workspace bytes (0xFF-prefilled in the poisoned run: the histogram must
    be cleared by the count call itself); counts, points and keys equal the oracle's."""
    import geom as og
    P, lens = _clouds()
    dl = 0.2
    o_pts, o_lens, o_keys = og.grid_subsample(P, lens, dl, return_keys=True)

    def run(ar):
        _, _, pts, off = _cloud_ops(ar)
        n, nc = len(P), len(lens)
        need = _size('fgr_grid_subsample_workspace', n, nc, 0)
        ws = ar.bytes(need, name='ws')
        counts = ar.vector(nc + 1, I64, 'out', name='counts')
        _ok(_L().fgr_grid_subsample_count(_p(pts), _p(off), nc, n, dl, 0, _p(ws), need, _p(counts),
                                          _st()), 'fgr_grid_subsample_count')
        host = counts.cpu().tolist()
        assert host[:nc] == [int(v) for v in o_lens] and host[nc] == len(o_pts)
        out = ar.matrix(host[nc], 3, 3, F32, 'out', name='out_points')
        keys = ar.vector(host[nc], I64, 'out', name='out_keys')
        _ok(_L().fgr_grid_subsample_fill(n, nc, 0, host[nc], _p(ws), need, _p(pts), _p(out),
                                         _p(keys), _st()), 'fgr_grid_subsample_fill')
        return out, keys, counts
    out, keys, _ = _both(run, gpu)
    assert np.array_equal(out.cpu().numpy(), o_pts) and np.array_equal(keys.cpu().numpy(), o_keys)


@pytest.mark.parametrize('mode', [0, 1])
def test_radius_search_footprint(gpu, mode):
    """fgr_radius_search, fgr_radius_count, fgr_radius_grid_build and fgr_radius_search_grid
    (tables and counts) over the same three clouds, width 24, radius 0.3: out (nq, width) int64
    with guards, the grid an exact fgr_radius_grid_workspace view; every table equals the
    oracle's (geom.radius_search / radius_counts). The points end at the tail guard, so a read
    of row ns sees the origin in the clean run and NaN in the poisoned one."""
    import geom as og
    P, lens = _clouds()
    r, K = 0.3, 24
    want = og.radius_search(P, lens, P, lens, r, K, mode)
    oc, omx = og.radius_counts(P, lens, P, lens, r)
    K = want.shape[1]                     # DIST: min(max count, limit), as fgreg.ops sizes it
    assert 0 < K <= 24

    def run(ar):
        _, _, pts, off = _cloud_ops(ar)
        n, nc = len(P), len(lens)
        out = ar.matrix(n, K, K, I64, 'out', name='out')
        _ok(_L().fgr_radius_search(_p(pts), _p(off), _p(pts), _p(off), nc, n, n, max(lens), r, mode,
                                   K, _p(out), _st()), 'fgr_radius_search')
        cnt, mx = ar.vector(n, I32, 'out', name='counts'), ar.vector(1, I32, 'out', name='max')
        _ok(_L().fgr_radius_count(_p(pts), _p(off), _p(pts), _p(off), nc, n, max(lens), r, _p(cnt),
                                  _p(mx), _st()), 'fgr_radius_count')
        need = _size('fgr_radius_grid_workspace', n, nc)
        grid = ar.bytes(need, name='grid')
        _ok(_L().fgr_radius_grid_build(_p(pts), _p(off), nc, n, r, _p(grid), need, _st()),
            'fgr_radius_grid_build')
        gout = ar.matrix(n, K, K, I64, 'out', name='grid_out')
        _ok(_L().fgr_radius_search_grid(_p(pts), _p(off), nc, n, max(lens), _p(pts), _p(off), n,
                                        _p(grid), need, r, mode, K, _p(gout), None, None, _st()),
            'fgr_radius_search_grid')
        gcnt, gmx = ar.vector(n, I32, 'out', name='grid_counts'), ar.vector(1, I32, 'out', name='grid_max')
        _ok(_L().fgr_radius_search_grid(_p(pts), _p(off), nc, n, max(lens), _p(pts), _p(off), n,
                                        _p(grid), need, r, 0, 0, None, _p(gcnt), _p(gmx), _st()),
            'fgr_radius_search_grid (counts)')
        return out, cnt, mx, gout, gcnt, gmx
    out, cnt, mx, gout, gcnt, gmx = _both(run, gpu)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(gout.cpu().numpy(), want)
    for c, m_ in ((cnt, mx), (gcnt, gmx)):
        assert np.array_equal(c.cpu().numpy().astype(np.int64), oc) and int(m_) == omx


@pytest.mark.parametrize('which', ['count', 'fill', 'build', 'search'])
def test_geometry_refuses_short_workspace(gpu, which):
    """ws_bytes / grid_bytes 16 below the reported size is refused before the first launch
    (fgr_grid_subsample_count / _fill, fgr_radius_grid_build, fgr_radius_search_grid):
    non-zero status, a message, outputs and workspace untouched."""
    P, lens = _clouds()
    n, nc = len(P), len(lens)
    ar = Arena(gpu, poison=True)
    _, _, pts, off = _cloud_ops(ar)
    if which in ('count', 'fill'):
        need = _size('fgr_grid_subsample_workspace', n, nc, 0)
        ws = ar.bytes(need, name='ws')
        counts = ar.vector(nc + 1, I64, 'out', name='counts')
        out = ar.matrix(n, 3, 3, F32, 'out', name='out_points')
        if which == 'count':
            rc = _L().fgr_grid_subsample_count(_p(pts), _p(off), nc, n, 0.2, 0, _p(ws), need - 16,
                                               _p(counts), _st())
        else:
            rc = _L().fgr_grid_subsample_fill(n, nc, 0, n, _p(ws), need - 16, _p(pts), _p(out), None,
                                              _st())
    else:
        need = _size('fgr_radius_grid_workspace', n, nc)
        ws = ar.bytes(need, name='grid')
        out = ar.matrix(n, 24, 24, I64, 'out', name='out')
        if which == 'build':
            rc = _L().fgr_radius_grid_build(_p(pts), _p(off), nc, n, 0.3, _p(ws), need - 16, _st())
        else:
            rc = _L().fgr_radius_search_grid(_p(pts), _p(off), nc, n, max(lens), _p(pts), _p(off), n,
                                             _p(ws), need - 16, 0.3, 0, 24, _p(out), None, None, _st())
    torch.cuda.synchronize()
    _refused(rc)
    for reg in ar.regions:
        reg.full = False
    ar.check()
    assert bool((ws == 0xFF).all())
    assert all(bool((reg.view.view(I32) == 0x7FC5A5A5).all()) for reg in ar.regions if reg.role == 'out')


# ---------------------------------------------------------------------------------------------
# Guarded-workspace replay: everything the Python wrappers launch, over exact-size scratch
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def guarded_scratch(gpu, monkeypatch):
    """-> a context manager that swaps every scratch provider of the package (fgreg.ops.scratch:
    the per-call buffers and the weight images; fgreg.ops._workspace and PrivateWorkspace.get:
    the grow-only >= 1 MiB buffers) for one that returns a fresh exact-size arena view,
    0xFF-prefilled, and checks all guards when the block ends. Yields the list of requested
    sizes."""
    import contextlib
    from fgreg import ops

    @contextlib.contextmanager
    def guard():
        arena, sizes = Arena(gpu, poison=True), []

        def provide(device, nbytes):
            assert torch.device(device) == arena.device
            sizes.append(int(nbytes))
            return arena.bytes(max(int(nbytes), 1), name=f'scratch #{len(sizes)} ({int(nbytes)} B)')
        with monkeypatch.context() as mp:
            mp.setattr(ops, 'scratch', provide)
            mp.setattr(ops, '_workspace', provide)
            mp.setattr(ops.PrivateWorkspace, 'get', lambda self, device, nbytes: provide(device, nbytes))
            yield sizes
            torch.cuda.synchronize()
        arena.check()
        assert sizes, 'the block requested no scratch: nothing was exercised'
    return guard


def _same(a, b, what=''):
    """Bit-equality of two nested results (dicts / lists / tensors / arrays / floats)."""
    if isinstance(a, dict):
        assert list(a) == list(b), what
        for k in a:
            _same(a[k], b[k], f'{what}.{k}')
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f'{what}[{i}]')
    elif torch.is_tensor(a):
        assert bit_equal(a.detach(), b.detach()), what
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what
    else:
        assert a == b or (a != a and b != b), what


def _eval_forward_and_tail(gpu, circle):
    """The eager inference forward on forward_modelnet_small (a fresh model per call: its first
    forward is eager and builds every weight image) and the test-step tail on its outputs."""
    import fgreg
    from conftest import forward_fixture, loss_fixture
    from fgreg import loss as fl
    import types
    cfg, sd, src, tgt, meta, _ = forward_fixture('forward_modelnet_small')
    _, _, batch, _, _, _, W, W_un = loss_fixture(gpu)
    model = fgreg.RegTR(cfg)
    model.load_state_dict(sd, strict=False)
    model = model.to(gpu).eval()
    model.preprocessor = fgreg.FixedMetaPreprocessor(batch['kpconv_meta'])
    out = model({'src_xyz': batch['src_xyz'], 'tgt_xyz': batch['tgt_xyz']})
    batch['kpconv_meta'] = {k: list(v) for k, v in batch['kpconv_meta'].items()}
    loss_cfg = type(cfg)(cfg)
    if circle:
        loss_cfg['feature_loss_type'] = 'circle'
    crit = types.SimpleNamespace(cfg=loss_cfg, feature_criterion=types.SimpleNamespace(W=W),
                                 feature_criterion_un=types.SimpleNamespace(W=W_un))
    losses = fl.compute_loss(crit, out, batch)
    metrics = fl.compute_metrics(out, batch)
    torch.cuda.synchronize()
    return dict(out), dict(losses), dict(metrics)


@pytest.mark.parametrize('feature_loss', ['infonce', 'circle'])
def test_replay_forward_and_test_step_tail(gpu, guarded_scratch, feature_loss):
    """Eager forward + compute_loss (InfoNCE / CircleLoss) + compute_metrics over guarded
    exact-size 0xFF scratch: outputs, losses and metrics bit-identical to the unguarded run."""
    plain = _eval_forward_and_tail(gpu, feature_loss == 'circle')
    with guarded_scratch():
        guarded = _eval_forward_and_tail(gpu, feature_loss == 'circle')
    _same(plain, guarded, feature_loss)


def test_replay_modelnet_metrics(gpu, guarded_scratch):
    """benchmark_modelnet.compute_metrics (fgr_modelnet_metrics) on the reference fixture."""
    from conftest import golden
    from fgreg import benchmark_modelnet as bm
    g = golden('modelnet_metrics')

    def run():
        T = lambda k: torch.from_numpy(g[k]).to(gpu)
        data = {'points_src': T('points_src'), 'points_ref': T('points_ref'),
                'points_raw': T('points_raw'), 'transform_gt': T('transform_gt')}
        return dict(bm.compute_metrics(data, T('pred_transforms')))
    plain = run()
    with guarded_scratch():
        guarded = run()
    _same(plain, guarded, 'metrics')


def test_replay_training_step(gpu, guarded_scratch):
    """One training step on test_gpu_train.py's small fixture (forward in train(), loss,
    backward through every fgr_*_bwd*, fgr_gemm_f16x3_wgrad, fgr_segnorm_*, fgr_colsum,
    fgr_nbr_inverse and fgr_kpconv_scatter launch): losses and every gradient bit-identical
    to the unguarded step."""
    from conftest import train_fixture
    from test_gpu_train import _gpu_train_step
    cfg, sd, src, tgt, meta, batch, W, W_un, _ = train_fixture()

    def run():
        losses, grads, _ = _gpu_train_step(cfg, sd, src, tgt, meta, batch, W, W_un, gpu)
        torch.cuda.synchronize()
        return {k: v.detach() for k, v in losses.items()}, grads
    plain = run()
    with guarded_scratch() as sizes:
        guarded = run()
    assert len(sizes) > 100          # the backward's per-call workspaces went through the arena
    _same(plain, guarded, 'train')


def test_replay_decoder_topk(gpu, guarded_scratch):
    """The CorrespondenceDecoder with num_neighbors > 0 (fgr_corr_attention + fgr_corr_topk_mask)
    on two cases of the reference's own fixture that do not raise (equal-length clouds k = 4, a
    padded batch k = 2; packing as test_gpu_topk_matches_reference): NaN rows and values
    bit-identical over guarded scratch."""
    from conftest import golden
    from fgreg.regtr import CorrespondenceDecoder
    from fgreg.transformer import PositionEmbeddingCoordsSine, Segments
    from test_decoder_topk import FIX, _case
    d = golden(FIX)
    for case in ('eq_k4', 'pad_k2'):
        B, sd, sx, tx, sf, tf, k, raised = _case(d, case)
        assert not raised
        L, D = sf.shape[0], sf.shape[-1]
        lens = [len(x) for x in sx] + [len(x) for x in tx]
        phantoms = [sf.shape[1] - n for n in lens[:B]] + [tf.shape[1] - n for n in lens[B:]]
        feats = torch.cat([sf[:, :len(sx[b]), b] for b in range(B)]
                          + [tf[:, :len(tx[b]), b] for b in range(B)]
                          + [sf[:, len(sx[b]):, b] for b in range(B)]
                          + [tf[:, len(tx[b]):, b] for b in range(B)], 1).contiguous().to(gpu)
        xyz = torch.cat(sx + tx, 0).contiguous().to(gpu)

        def run():
            pe = PositionEmbeddingCoordsSine(3, D)
            dec = CorrespondenceDecoder(D, True, pe, num_neighbors=k)
            dec.load_state_dict(sd)
            dec = dec.to(gpu).eval()
            seg = Segments(lens, gpu, n_layers=L, phantoms=phantoms)
            with torch.no_grad():
                out = dec.forward_packed(feats, xyz, pe(xyz), seg)
            torch.cuda.synchronize()
            return out
        plain = run()
        with guarded_scratch():
            guarded = run()
        assert bool(torch.isnan(plain[0]).any()) and not bool(torch.isnan(plain[0]).all())
        _same(plain, guarded, case)


def test_replay_forward_own_preprocessor(gpu, guarded_scratch):
    """A whole eager forward with the model's own preprocessor (grid subsampling and radius
    search scratch, fgreg.ops.scratch) and the top-k decoder, on the padded decoder fixture; an
    IndexError (raised where the reference raises, test_decoder_topk) must be raised in both."""
    import fgreg
    from conftest import forward_fixture
    cfg, sd, src, tgt, _, _ = forward_fixture('forward_modelnet_decoder')

    def run(k):
        model = fgreg.RegTR(cfg)
        model.load_state_dict(sd, strict=False)
        model.correspondence_decoder.num_neighbors = k
        model = model.to(gpu).eval()
        batch = {'src_xyz': [torch.from_numpy(c).to(gpu) for c in src],
                 'tgt_xyz': [torch.from_numpy(c).to(gpu) for c in tgt]}
        try:
            out = dict(model(batch))
        except IndexError:
            return 'IndexError'
        torch.cuda.synchronize()
        return out, batch['kpconv_meta']['neighbors']
    for k in (0, 3):
        plain = run(k)
        with guarded_scratch():
            guarded = run(k)
        _same(plain, guarded, f'forward k={k}')
