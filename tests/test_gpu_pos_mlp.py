"""The learned positional embedding's MLP in one launch (fgr_pos_mlp_f16x3, ops.pos_mlp;
position_embedding.py:52-71): 3 -> 32 -> 64 -> 128 -> 256 -> d_model with ReLU between the
layers, the hidden activations kept on chip.

Checked against a float64 restatement (the criterion of test_gpu_ffn.py: fp32-level error and no
worse than a few times torch's own fp32 chain), against the reference's own outputs
(pos_embed_learned.npz), against the five-launch path it replaces, for row independence (bit
for bit), for its memory footprint (tests/_arena.py) and for the C ABI's refusals. The kernel
reads the plain fgr_split_weights_h3 images (layout pinned by test_gpu_footprint.py), so there
is no new image format to pin here.
"""
import ast
import functools
import math

import numpy as np
import pytest
import torch

from _arena import assert_both_equal, bit_equal, run_both
from conftest import golden, rel_err

pytestmark = pytest.mark.gpu
WIDTHS = (3, 32, 64, 128, 256)


def _weights(d, seed, case='plain'):
    """[(W_l, b_l)] l = 0..4 at PyTorch's default Linear scale."""
    g = torch.Generator().manual_seed(seed)
    dims = WIDTHS + (d,)
    ws = []
    for l in range(5):
        k, n = dims[l], dims[l + 1]
        w = (2 * torch.rand(n, k, generator=g) - 1) / math.sqrt(k)
        b = 0.1 * torch.randn(n, generator=g)
        ws.append([w, b])
    if case == 'big_row':
        ws[2][0][3] *= 1e4              # one hidden unit of a middle layer 1e4 x the rest
    if case == 'neg_bias':
        # every hidden bias negative: the ReLUs cut 50-95 % of the units (more with depth), and
        # at the all-zero point every hidden layer is cut entirely, so its output is b4. (A
        # uniform shift of -0.5 instead zeroes the last hidden layer of EVERY row at these
        # weight scales, which tests nothing.)
        for l in range(4):
            ws[l][1] = -ws[l][1].abs()
            assert bool((ws[l][1] < 0).all())
    return [(w, b) for w, b in ws]


def _points(n, seed):
    """Coordinates at ModelNet scale (|x| <= 1), at 3DMatch scale (a few metres, off-centre)
    and an all-zero point."""
    g = torch.Generator().manual_seed(seed)
    x = 2 * torch.rand(n, 3, generator=g) - 1
    far = 3 * torch.rand(n, 3, generator=g) - 1.5 + torch.tensor([2.5, -1.0, 1.2])
    if n == 1:
        return far if seed % 2 else x
    x[n // 2:] = far[n // 2:]
    if n > 8:
        x[7] = 0.0
    return x


def _ref64(x, ws):
    h = x.double()
    for l, (w, b) in enumerate(ws):
        h = h @ w.double().t() + b.double()
        if l < 4:
            h = h.clamp_min(0)
    return h


def _run(gpu, x, ws, out=None):
    from fgreg import linear as fl
    from fgreg import ops
    W = [(w.to(gpu), b.to(gpu)) for w, b in ws]
    imgs = [fl.weight_image(w, mode='f16x3', cache=False) for w, _ in W[1:]]
    return ops.pos_mlp(x, W[0][0], W[0][1], imgs, [b for _, b in W[1:]], out=out)


@pytest.mark.parametrize('d', [256, 512])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 717, 9544])
@pytest.mark.parametrize('case', ['plain', 'big_row', 'neg_bias'])
def test_pos_mlp_vs_fp64(gpu, n, d, case):
    from fgreg import ops
    assert ops.pos_mlp_supported(n, d)
    ws = _weights(d, n + d, case)
    x = _points(n, n + d // 256)
    ref = _ref64(x, ws)
    X = x.to(gpu)
    out = _run(gpu, X, ws)
    h32 = X                              # torch fp32 (the comparison baseline only)
    for l, (w, b) in enumerate(ws):
        h32 = torch.addmm(b.to(gpu), h32, w.to(gpu).t())
        if l < 4:
            h32 = h32.clamp_min(0)
    e32, e = rel_err(h32, ref), rel_err(out, ref)
    print(f'n {n} d {d} {case}: e {e:.3g} e32 {e32:.3g}')
    assert e < 1e-5 and e < 4 * e32 + 1e-6, (e, e32)
    if case == 'neg_bias' and n > 8:
        # the all-zero point: every hidden layer is cut entirely, the output is b4 itself
        assert bool((ref[7] == ws[4][1].double()).all())
        assert bit_equal(out[7].cpu(), ws[4][1])
        assert bool((out.cpu() != ws[4][1]).any(1).sum() > n // 4)     # not a degenerate case


@functools.lru_cache(maxsize=None)
def _reference_fixture():
    return golden('pos_embed_learned')


@pytest.mark.parametrize('d', [256, 512])
@pytest.mark.parametrize('scale', ['modelnet', '3dmatch'])
def test_pos_mlp_vs_reference(gpu, d, scale):
    """The reference's PositionEmbeddingLearned on its own outputs (weights rebuilt from
    (key, shape, seed): golden/named_weights.py)."""
    from named_weights import named_value
    from fgreg.transformer import PositionEmbeddingLearned
    f = _reference_fixture()
    raw = f[f'sd_keys.{d}'].item()
    keys = ast.literal_eval(raw.decode() if isinstance(raw, bytes) else str(raw))
    m = PositionEmbeddingLearned(3, d)
    assert [(k, list(v.shape)) for k, v in m.state_dict().items()] == [(k, list(s)) for k, s in keys]
    m.load_state_dict({k: torch.from_numpy(named_value(k, s, int(f['sd_seed']), 0.0)) for k, s in keys})
    m = m.to(gpu).eval()
    with torch.no_grad():
        out = m(torch.from_numpy(f[f'in.{scale}']).to(gpu))
    e = rel_err(out, f[f'out.{scale}.{d}'])
    print(f'd {d} {scale}: {e:.3g}')
    assert e < 1e-5, e


@pytest.mark.parametrize('n,d', [(9544, 256), (717, 512), (65, 256)])
def test_pos_mlp_equals_five_launch_path(gpu, n, d):
    """ops.pos_mlp against five linear() launches (ReLU on the first four): the same f16x3
    products with the hidden activations in HBM and the GEMM's own row scales."""
    from fgreg import linear as fl
    from fgreg import ops
    ws = _weights(d, 5)
    X = _points(n, 5).to(gpu)
    out = _run(gpu, X, ws)
    h = X
    for l, (w, b) in enumerate(ws):
        h = fl.linear(h, w.to(gpu), b.to(gpu), act=ops.ACT_RELU if l < 4 else ops.ACT_NONE,
                      cache=False)
    e = rel_err(out, h)
    print(f'n {n} d {d}: {e:.3g}')
    assert e < 4e-6, e


@pytest.mark.parametrize('d', [256, 512])
def test_pos_mlp_row_independence(gpu, d):
    """A row's bits depend on that row's coordinates alone: every row of an n = 65 call equals
    the same point embedded alone (n = 1), and a call repeats itself bit for bit."""
    n = 65
    ws = _weights(d, 11)
    X = _points(n, 11).to(gpu)
    out = _run(gpu, X, ws)
    again = _run(gpu, X, ws)
    assert bit_equal(out, again)
    for r in range(n):
        one = _run(gpu, X[r:r + 1].clone(), ws)
        assert bit_equal(one[0], out[r]), r
    # and of the row tiling: the same points as the tail of a longer call (other block sizes)
    big = torch.cat([_points(9000, 12).to(gpu), X])
    assert bit_equal(_run(gpu, big, ws)[9000:], out)


@pytest.mark.parametrize('n,d', [(1, 256), (65, 256), (65, 512), (4200, 256)])
def test_pos_mlp_footprint(gpu, n, d):
    """fgr_pos_mlp_f16x3 through ctypes on a guarded arena: strided output (ldo = d + 4) with
    sentinel pads and guards, images of exactly the reported bytes prefilled 0x00 / 0xFF,
    poisoned input guards; clean and poisoned outputs bit-identical. n = 4200: the 32-row tiling
    with a partial last block (64-row blocks: test_pos_mlp_vs_fp64 at n = 9544 and the tail of
    test_pos_mlp_row_independence)."""
    from fgreg import _lib
    L = _lib.load()
    ws = _weights(d, n + d)
    x = _points(n, 3)
    ref = _ref64(x, ws)
    st = torch.cuda.current_stream().cuda_stream

    def image(ar, w):
        nb = _lib._sz(0)
        _lib.check(L.fgr_split_weights_h3_bytes(w.shape[0], w.shape[1], nb), 'bytes')
        img = ar.bytes(nb.value, name='w_img')
        wd = ar.put(w, name='w')
        _lib.check(L.fgr_split_weights_h3(wd.data_ptr(), w.shape[0], w.shape[1], w.shape[1], 1,
                                          img.data_ptr(), st), 'fgr_split_weights_h3')
        return img

    def run(ar):
        xin = ar.put(x, name='xyz')
        w0, b0 = ar.put(ws[0][0], name='w0'), ar.put(ws[0][1], name='b0')
        imgs = [image(ar, w) for w, _ in ws[1:]]
        bs = [ar.put(b, name='bias') for _, b in ws[1:]]
        out = ar.matrix(n, d, d + 4, torch.float32, 'out', name='out')
        _lib.check(L.fgr_pos_mlp_f16x3(
            xin.data_ptr(), n, w0.data_ptr(), b0.data_ptr(), imgs[0].data_ptr(), bs[0].data_ptr(),
            imgs[1].data_ptr(), bs[1].data_ptr(), imgs[2].data_ptr(), bs[2].data_ptr(),
            imgs[3].data_ptr(), bs[3].data_ptr(), d, out.data_ptr(), d + 4, st), 'fgr_pos_mlp_f16x3')
        return out
    clean, poisoned = run_both(run, gpu)
    assert_both_equal(clean, poisoned)
    e = rel_err(clean, ref)
    assert e < 1e-5, e


def test_pos_mlp_refusals(gpu):
    import fgreg
    from fgreg import _lib
    L = _lib.load()
    assert L.fgr_pos_mlp_f16x3_supported(1, 256) and L.fgr_pos_mlp_f16x3_supported(1 << 33, 512)
    assert not L.fgr_pos_mlp_f16x3_supported(100, 128)
    assert not L.fgr_pos_mlp_f16x3_supported(100, 384)
    assert not L.fgr_pos_mlp_f16x3_supported(0, 256)
    ws = _weights(256, 1)
    x = _points(10, 1).to(gpu)
    W = [(w.to(gpu), b.to(gpu)) for w, b in ws]
    from fgreg import linear as fl
    im = [fl.weight_image(w, mode='f16x3', cache=False).img for w, _ in W[1:]]
    out = torch.full((10, 256), 7.0, device=gpu)
    p = lambda t: t.data_ptr()        # noqa: E731
    args = [p(x), 10, p(W[0][0]), p(W[0][1]), p(im[0]), p(W[1][1]), p(im[1]), p(W[2][1]), p(im[2]),
            p(W[3][1]), p(im[3]), p(W[4][1]), 256, p(out), 256, None]

    def refused(a):
        rc = L.fgr_pos_mlp_f16x3(*a)
        assert rc != 0 and len(L.fgr_last_error()) > 0
        with pytest.raises(fgreg.FgrError):
            _lib.check(rc, 'fgr_pos_mlp_f16x3')
    for width in (128, 384, 1024):                       # unsupported d_model
        a = list(args)
        a[12] = width
        a[14] = width
        refused(a)
    for i in (0, 2, 3, 4, 5, 10, 11, 13):                # null pointers
        a = list(args)
        a[i] = None
        refused(a)
    a = list(args)
    a[14] = 255                                          # ldo < d_model
    refused(a)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                      # a refused call writes nothing
    # n = 0 touches nothing (as fgr_sine_pos_embed)
    a = list(args)
    a[0], a[1], a[13] = None, 0, None
    assert L.fgr_pos_mlp_f16x3(*a) == 0
