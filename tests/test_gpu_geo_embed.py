"""The geometric structure embedding's two kernels (fgr_geo_embed_indices, fgr_geo_embed_f16x3;
ops.geo_embed_indices, ops.geo_embed) and the module built on them (fgreg.transformer.
GeometricStructureEmbedding; position_embedding.py:129-196).

Checked against the host restatement tests/_geo_ref.py: the neighbour choice bit for bit on a
lattice (where every squared distance is exact in fp32, so the tie rule is what is tested), the
distances and angles against fp64, the fused embedding against fp64 by the criterion of
test_gpu_pos_mlp.py (fp32-level error, and no worse than a few times what torch's own fp32
gives), against the composed path it replaces, for point and cloud independence (bit for bit),
against the reference class's own outputs (pos_embed_geo.npz), for its memory footprint
(tests/_arena.py) and for the C ABI's refusals.
"""
import ast
import functools
import math

import numpy as np
import pytest
import torch

import _geo_ref as gr
from _arena import assert_both_equal, bit_equal, run_both
from conftest import golden, rel_err

pytestmark = pytest.mark.gpu
D = 256
SIGMA_D, SIGMA_A = 0.2, 15
PACK = [4, 65, 17, 130]


def _shapes(k):
    """Single clouds of k + 1, k + 2, 63, 64, 65 points and one packed call. The pack is
    [4, 65, 17, 130]; at k = 4 its first cloud has 5 points, because a cloud needs more than k
    points (the definition: n <= k raises)."""
    return [[k + 1], [k + 2], [63], [64], [65], [max(PACK[0], k + 1)] + PACK[1:]]


SHAPES = [(k, i) for k in (1, 3, 4) for i in range(6)]


def _lattice(lengths, seed):
    """Clouds of distinct points on a 0.25-spaced lattice of 6^3 cells, every cloud drawn from
    the same box: clouds overlap in space (points of different clouds coincide), so a neighbour
    taken across a cloud boundary changes the answer; within a cloud ties are everywhere."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        cells = rng.choice(6 ** 3, size=n, replace=False)
        out.append(np.stack([cells // 36, cells // 6 % 6, cells % 6], 1) * 0.25)
    return np.concatenate(out).astype(np.float32)


def _random(lengths, scale, seed):
    rng = np.random.default_rng(seed)
    n = sum(lengths)
    if scale == 'modelnet':
        return rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    return (rng.uniform(-1.5, 1.5, (n, 3)) + np.array([2.5, -1.0, 1.2])).astype(np.float32)


def _indices(gpu, x, lengths, k):
    from fgreg import ops
    X = torch.from_numpy(x).to(gpu)
    return ops.geo_embed_indices(X, ops.offsets(lengths, gpu), k, SIGMA_D, SIGMA_A)


@pytest.mark.parametrize('k,shape', SHAPES)
def test_indices_lattice_bit_exact(gpu, k, shape):
    """nn equals "the k nearest by index-excluded squared distance, ties to the lower index"
    bit for bit; every d^2 here is a multiple of 1/16 below 2^24 / 16, exact in fp32."""
    lengths = _shapes(k)[shape]
    x = _lattice(lengths, 10 * k + shape)
    nn, d, a = _indices(gpu, x, lengths, k)
    want = gr.knn(x, lengths, k, dtype=np.float32)
    assert nn.dtype == torch.int32 and tuple(nn.shape) == (len(x), k)
    assert np.array_equal(nn.cpu().numpy().astype(np.int64), want)
    if len(lengths) > 1:
        # not a vacuous pack: ignoring the cloud boundaries gives other neighbours
        assert not np.array_equal(gr.knn(x, [len(x)], k, dtype=np.float32), want)
    d64, a64 = gr.indices(x, want, SIGMA_D, SIGMA_A)
    assert float((d.cpu().double() - d64).abs().max()) <= 1e-6 * float(d64.max())
    assert float((a.cpu().double() - a64).abs().max()) <= 1e-5
    assert bool((a.cpu()[:, torch.arange(k), torch.arange(k)] == 0).all())      # r == j: angle 0


@pytest.mark.parametrize('k', [1, 3, 4])
@pytest.mark.parametrize('scale,seed', [('modelnet', 1), ('3dmatch', 2)])
def test_indices_vs_fp64(gpu, k, scale, seed):
    """d and a against fp64 on random clouds. Points whose k-th and (k+1)-th fp64 neighbours lie
    within relative 1e-4 in d^2 are left out (fp32 may rank them either way); at most 1 % may be.
    Seeds 1 / 2: fp64 alone leaves out at most 1 of the 1 065 points at any k (checked on the CPU).

    Bounds. d: differences, three products, two sums, sqrt and a division are each within half
    an ulp, about 4 * 2^-24 relative in all: 1e-6 relative. a: the cross and dot products carry
    about ten roundings of 2^-24 relative to |v_r| |v_j|, i.e. at most ~1e-6 rad in the angle
    (near-parallel vectors included, where |cross| is small but so is its absolute error), plus
    atan2f's own ulps of at most pi; times 180 / (15 pi) = 3.8: 1e-5 absolute."""
    lengths = [100, 257, 65, 643]
    x = _random(lengths, scale, seed)
    margin = gr.knn_margin(x, lengths, k)
    keep = margin > 1e-4
    print(f'{scale} k {k}: left out {int((~keep).sum())} of {len(x)}')
    assert (~keep).mean() <= 0.01
    nn, d, a = _indices(gpu, x, lengths, k)
    nn = nn.cpu().numpy().astype(np.int64)
    want = gr.knn(x, lengths, k)
    assert np.array_equal(np.sort(nn[keep], 1), np.sort(want[keep], 1))
    off = np.concatenate([[0], np.cumsum(lengths)])
    cloud = np.searchsorted(off, np.arange(len(x)), side='right') - 1
    assert bool(((nn >= off[cloud][:, None]) & (nn < off[cloud + 1][:, None])).all())
    assert bool((nn != np.arange(len(x))[:, None]).all())
    d64, a64 = gr.indices(x, nn, SIGMA_D, SIGMA_A)                # of the kernel's own choice
    ed = float(((d.cpu().double() - d64).abs() / d64)[keep].max())
    ea = float((a.cpu().double() - a64).abs()[keep].max())
    print(f'  d rel {ed:.3g}  a abs {ea:.3g}')
    assert ed <= 1e-6 and ea <= 1e-5, (ed, ea)


def _weights(seed, case='plain'):
    """(Wd, bd, Wa, ba) at PyTorch's default Linear scale; neg_bias: both biases negative."""
    g = torch.Generator().manual_seed(seed)
    ws = []
    for _ in range(2):
        w = (2 * torch.rand(D, D, generator=g) - 1) / math.sqrt(D)
        b = 0.1 * torch.randn(D, generator=g)
        ws += [w, -b.abs() if case == 'neg_bias' else b]
    return ws


def _fused(gpu, d, a, ws, reduction, out=None):
    from fgreg import linear as fl
    from fgreg import ops
    Wd, bd, Wa, ba = (t.to(gpu) for t in ws)
    return ops.geo_embed(d, a, gr.div_term(D, torch.float32).to(gpu),
                         fl.weight_image(Wd, mode='f16x3', cache=False), bd,
                         fl.weight_image(Wa, mode='f16x3', cache=False), ba,
                         ops.GEO_MEAN if reduction == 'mean' else ops.GEO_MAX, out=out)


@pytest.mark.parametrize('case', ['plain', 'neg_bias'])
@pytest.mark.parametrize('reduction', ['max', 'mean'])
@pytest.mark.parametrize('k,shape', SHAPES)
def test_fused_vs_fp64(gpu, k, shape, reduction, case):
    """Against the fp64 restatement of the definition given the kernel's own nn; e32 is torch's
    fp32 evaluation of the same k (1 + k) rows per point. Lattice clouds: the arguments reach
    7.7."""
    from fgreg import ops
    lengths = _shapes(k)[shape]
    x = _lattice(lengths, 10 * k + shape)
    assert ops.geo_embed_supported(len(x), D, k)
    nn, d, a = _indices(gpu, x, lengths, k)
    ws = _weights(100 * k + shape, case)
    out = _fused(gpu, d, a, ws, reduction)
    nn = nn.cpu().numpy()
    w = gr.div_term(D)
    ref = gr.forward(x, lengths, k, SIGMA_D, SIGMA_A, w, *ws, reduction, nn=nn)
    f32 = gr.forward(x, lengths, k, SIGMA_D, SIGMA_A, w, *ws, reduction, nn=nn, dtype=torch.float32)
    e32, e = rel_err(f32, ref), rel_err(out, ref)
    print(f'k {k} {lengths} {reduction} {case}: e {e:.3g} e32 {e32:.3g}')
    assert e < 1e-5 and e < 4 * e32 + 1e-6, (e, e32)


def _module(gpu, reduction, k=3, seed=7):
    from fgreg.transformer import GeometricStructureEmbedding
    torch.manual_seed(seed)
    return GeometricStructureEmbedding(D, angle_k=k, reduction_a=reduction).to(gpu).eval()


def _embed(m, gpu, x, lengths, composed=False):
    from fgreg import ops
    X = torch.from_numpy(x).to(gpu)
    off = ops.offsets(lengths, gpu)
    with torch.no_grad():
        return (m.forward_composed if composed else m)(X, off, lengths)


@pytest.mark.parametrize('reduction', ['max', 'mean'])
@pytest.mark.parametrize('lengths', [PACK, [717, 700]])
def test_fused_equals_composed_path(gpu, lengths, reduction):
    """The two-launch path against the composed one (indices kernel, torch sin / cos, two
    linear() launches, torch reductions): the same f16x3 products, with the embedding rows in HBM
    and the GEMM's own row scales; test_pos_mlp_equals_five_launch_path's tolerance."""
    m = _module(gpu, reduction)
    x = _lattice(lengths, 3) if lengths == PACK else _random(lengths, 'modelnet', 3)
    e = rel_err(_embed(m, gpu, x, lengths), _embed(m, gpu, x, lengths, composed=True))
    print(f'{lengths} {reduction}: {e:.3g}')
    assert e < 4e-6, e


@pytest.mark.parametrize('reduction', ['max', 'mean'])
def test_cloud_independence_and_repeat(gpu, reduction):
    """Embedding the pack equals embedding each cloud alone, bit for bit (other block
    boundaries, other neighbours in the call), and a call repeats itself bit for bit."""
    m = _module(gpu, reduction)
    x = _lattice(PACK, 5)
    out = _embed(m, gpu, x, PACK)
    assert bit_equal(out, _embed(m, gpu, x, PACK))
    o = 0
    for n in PACK:
        assert bit_equal(_embed(m, gpu, x[o:o + n], [n]), out[o:o + n]), n
        o += n


@functools.lru_cache(maxsize=None)
def _reference_fixture():
    return golden('pos_embed_geo')


@pytest.mark.parametrize('reduction', ['max', 'mean'])
@pytest.mark.parametrize('scale', ['modelnet', '3dmatch'])
def test_vs_reference_class(gpu, scale, reduction):
    """The reference's GeometricStructureEmbedding on its own outputs (weights rebuilt from (key,
    shape, seed)). Bound 1e-5 + 2 e_ref, e_ref the reference's own error against fp64 stored by
    the generator (its fp32 x^2 - 2 x.y + y^2 distances): e_ref 1.0e-6 / 1.1e-6 (modelnet max /
    mean), 3.1e-6 / 3.4e-6 (3dmatch). Measured on the MI355X, e against the reference's outputs:
    1.08e-6 / 1.18e-6 (modelnet max / mean), 3.14e-6 / 3.34e-6 (3dmatch) -- the reference's own
    distance error, to the digit; against fp64 the kernel is at 2e-7 .. 4e-7 (test_fused_vs_fp64).
    Also in DESIGN.md "Geometric structure embedding"."""
    from named_weights import named_value
    from fgreg.transformer import GeometricStructureEmbedding
    f = _reference_fixture()
    raw = f['sd_keys'].item()
    keys = ast.literal_eval(raw.decode() if isinstance(raw, bytes) else str(raw))
    k = int(f['angle_k'])
    m = GeometricStructureEmbedding(D, angle_k=k, reduction_a=reduction)
    assert [(n, list(v.shape)) for n, v in m.state_dict().items()] == [(n, list(s)) for n, s in keys]
    sd = {n: torch.from_numpy(named_value(n, s, int(f['sd_seed']), 0.0)) for n, s in keys}
    sd['embedding.div_term'] = torch.from_numpy(f['div_term'])
    # constants from torch.exp on the host: the last bit differs between CPUs' vector libraries
    assert torch.allclose(m.embedding.div_term, sd['embedding.div_term'], rtol=1e-6, atol=0)
    m.load_state_dict(sd)
    m = m.to(gpu).eval()
    x = f[f'in.{scale}']
    out = _embed(m, gpu, x, [len(x)])
    e, e_ref = rel_err(out, f[f'out.{scale}.{reduction}']), float(f[f'e_ref.{scale}.{reduction}'])
    print(f'{scale} {reduction}: e {e:.3g} e_ref {e_ref:.3g}')
    assert e < 1e-5 + 2 * e_ref, (e, e_ref)


def test_errors(gpu):
    import fgreg
    from fgreg import ops
    from fgreg.transformer import GeometricStructureEmbedding
    with pytest.raises(ValueError, match='Unsupported reduction mode'):
        GeometricStructureEmbedding(D, reduction_a='sum')
    m = _module(gpu, 'max')
    x = torch.from_numpy(_lattice([3, 65], 1)).to(gpu)
    for fn in (m, m.forward_composed, m.train_forward):
        with pytest.raises(ValueError, match='3 points'):          # n <= k, from the host lengths
            fn(x, ops.offsets([3, 65], gpu), [3, 65])
    with pytest.raises(fgreg.FgrError):
        ops.geo_embed_indices(x, ops.offsets([3, 65], gpu), 5, SIGMA_D, SIGMA_A)


@pytest.mark.parametrize('k,lengths', [(3, [4]), (3, PACK), (4, [5, 65]), (1, [2, 63])])
def test_footprint(gpu, k, lengths):
    """Both entry points through ctypes on a guarded arena: exact outputs (strided out, ldo =
    D + 4) with sentinel pads and guards, images of exactly the reported bytes, poisoned input
    guards; clean and poisoned outputs bit-identical."""
    from fgreg import _lib
    L = _lib.load()
    x = torch.from_numpy(_lattice(lengths, 2))
    n = x.shape[0]
    ws = _weights(3)
    off = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64)
    st = torch.cuda.current_stream().cuda_stream

    def image(ar, w):
        nb = _lib._sz(0)
        _lib.check(L.fgr_split_weights_h3_bytes(D, D, nb), 'bytes')
        img = ar.bytes(nb.value, name='w_img')
        wd = ar.put(w, name='w')
        _lib.check(L.fgr_split_weights_h3(wd.data_ptr(), D, D, D, 1, img.data_ptr(), st), 'split')
        return img

    def run(ar):
        xin, offs = ar.put(x, name='xyz'), ar.put(off, name='cloud_off')
        nn = ar.matrix(n, k, k, torch.int32, 'out', name='nn')
        d = ar.matrix(n, k, k, torch.float32, 'out', name='d')
        a = ar.matrix(n, k * k, k * k, torch.float32, 'out', name='a')
        _lib.check(L.fgr_geo_embed_indices(xin.data_ptr(), n, offs.data_ptr(), len(lengths), k,
                                           SIGMA_D, 180.0 / (SIGMA_A * math.pi), nn.data_ptr(),
                                           d.data_ptr(), a.data_ptr(), st), 'fgr_geo_embed_indices')
        imgs = [image(ar, ws[0]), image(ar, ws[2])]
        bs = [ar.put(ws[1], name='bd'), ar.put(ws[3], name='ba')]
        w = ar.put(gr.div_term(D, torch.float32), name='div_term')
        out = ar.matrix(n, D, D + 4, torch.float32, 'out', name='out')
        _lib.check(L.fgr_geo_embed_f16x3(d.data_ptr(), a.data_ptr(), n, k, w.data_ptr(),
                                         imgs[0].data_ptr(), bs[0].data_ptr(), imgs[1].data_ptr(),
                                         bs[1].data_ptr(), D, 0, out.data_ptr(), D + 4, st),
                   'fgr_geo_embed_f16x3')
        return nn, d, a, out
    clean, poisoned = run_both(run, gpu)
    assert_both_equal(clean, poisoned)
    nn = clean[0].cpu().numpy()
    assert np.array_equal(nn.astype(np.int64), gr.knn(x.numpy(), lengths, k, dtype=np.float32))
    ref = gr.forward(x.numpy(), lengths, k, SIGMA_D, SIGMA_A, gr.div_term(D), *ws, 'max', nn=nn)
    assert rel_err(clean[3], ref) < 1e-5


def test_refusals(gpu):
    import fgreg
    from fgreg import _lib
    from fgreg import linear as fl
    L = _lib.load()
    assert L.fgr_geo_embed_f16x3_supported(1, 256, 1) and L.fgr_geo_embed_f16x3_supported(9544, 256, 4)
    for bad in ((100, 128, 3), (100, 512, 3), (100, 256, 0), (100, 256, 5), (0, 256, 3)):
        assert not L.fgr_geo_embed_f16x3_supported(*bad)
    lengths = [10]
    x = _lattice(lengths, 1)
    nn, d, a = _indices(gpu, x, lengths, 3)
    Wd, bd, Wa, ba = (t.to(gpu) for t in _weights(1))
    im = [fl.weight_image(w, mode='f16x3', cache=False).img for w in (Wd, Wa)]
    w = gr.div_term(D, torch.float32).to(gpu)
    out = torch.full((10, D), 7.0, device=gpu)
    p = lambda t: t.data_ptr()        # noqa: E731
    args = [p(d), p(a), 10, 3, p(w), p(im[0]), p(bd), p(im[1]), p(ba), D, 0, p(out), D, None]

    def refused(fn, a_):
        rc = fn(*a_)
        assert rc != 0 and len(L.fgr_last_error()) > 0
        with pytest.raises(fgreg.FgrError):
            _lib.check(rc, 'geo_embed')
    for i, v in ((9, 128), (9, 512), (3, 0), (3, 5), (10, 2), (12, 255), (12, 258)):
        a_ = list(args)
        a_[i] = v
        refused(L.fgr_geo_embed_f16x3, a_)
    for i in (0, 1, 4, 5, 6, 7, 8, 11):                  # null pointers
        a_ = list(args)
        a_[i] = None
        refused(L.fgr_geo_embed_f16x3, a_)
    X = torch.from_numpy(x).to(gpu)
    from fgreg import ops
    off = ops.offsets(lengths, gpu)
    nn2 = torch.full((10, 3), 7, dtype=torch.int32, device=gpu)
    iargs = [p(X), 10, p(off), 1, 3, SIGMA_D, 1.0, p(nn2), p(d), p(a), None]
    for i, v in ((4, 0), (4, 5), (5, 0.0), (5, -1.0), (3, 0), (0, None), (2, None), (7, None),
                 (8, None), (9, None)):
        a_ = list(iargs)
        a_[i] = v
        refused(L.fgr_geo_embed_indices, a_)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((nn2 == 7).all())      # a refused call writes nothing
    # n = 0 touches nothing
    a_ = list(args)
    a_[0], a_[1], a_[2], a_[11] = None, None, 0, None
    assert L.fgr_geo_embed_f16x3(*a_) == 0
    a_ = list(iargs)
    a_[0], a_[1], a_[7], a_[8], a_[9] = None, 0, None, None, None
    assert L.fgr_geo_embed_indices(*a_) == 0
