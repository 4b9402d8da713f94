"""Grid subsampling of large-extent clouds: the radix-sorted sparse path
(fgr_grid_subsample_sparse_*, fgreg.ops.grid_subsample(..., sparse=)) against oracle/geom.py.

Every comparison is np.array_equal / bit equality on points, lengths and keys: the sparse path
restates the dense path's and the oracle's arithmetic, so there is no tolerance anywhere.
"""
import functools

import numpy as np
import pytest
import torch

import geom as og
import model_oracle as mo
from _arena import Arena, assert_both_equal, bit_equal, run_both
from conftest import forward_fixture, golden
from fgreg.ops import GRID_SPARSE_TILE as T
from test_gpu_footprint import guarded_scratch  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
F32, I64 = torch.float32, torch.int64


def _run(gpu, P, lens, dl, **kw):
    """ops.grid_subsample(return_keys=True) -> (points, lengths, keys) as numpy / list."""
    import fgreg.ops as ops
    lens = [int(v) for v in lens]
    pts = torch.from_numpy(np.ascontiguousarray(P, np.float32)).to(gpu)
    off = ops.offsets(lens, gpu)
    sub, sl, keys = ops.grid_subsample(pts, off, lens, dl, return_keys=True, **kw)
    return sub.cpu().numpy(), sl, keys.cpu().numpy()


def _assert_oracle(got, P, lens, dl):
    o_pts, o_lens, o_keys = og.grid_subsample(P, lens, dl, return_keys=True)
    sub, sl, keys = got
    assert sl == [int(v) for v in o_lens]
    assert np.array_equal(keys, o_keys)
    assert np.array_equal(sub, o_pts)


# ---------------------------------------------------------------------------------------------
# 1. two points
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sparse', ['auto', True])
def test_two_points_past_the_dense_limit(gpu, sparse):
    """(0,0,0) and (1000,1000,1000) at dl = 1: a 1001^3 key space (> 2^28) holding two voxels.
    The default sparse=False still raises (the regression guard)."""
    import fgreg
    import fgreg.ops as ops
    P = np.array([[0, 0, 0], [1000, 1000, 1000]], np.float32)
    sub, sl, keys = _run(gpu, P, [2], 1.0, sparse=sparse)
    assert sl == [2]
    assert keys.tolist() == [0, 1003003000]
    assert np.array_equal(sub, P)
    _assert_oracle((sub, sl, keys), P, [2], 1.0)
    pts = torch.from_numpy(P).to(gpu)
    with pytest.raises(fgreg.FgrError, match='dense histogram limit'):
        ops.grid_subsample(pts, ops.offsets([2], gpu), [2], 1.0)


# ---------------------------------------------------------------------------------------------
# 2. tile borders and wide keys
# ---------------------------------------------------------------------------------------------
def _wide_cloud(n):
    """n points at dl = 1 with integer coordinates in [0, 2^20) x [0, 2^20) x [0, 4) plus a
    per-point fractional offset in [0.1, 0.9) (fp32 keeps at least 1/8 at 2^20: the offset
    never leaves the voxel): 42-bit keys. The two extreme corners come first, about a sixth of
    the rest share a voxel with another point, and the rows are shuffled."""
    rng = np.random.default_rng(1000 + n)
    cells = np.zeros((n, 3), np.int64)
    n_dup = (n - 2) // 6 if n > 2 else 0
    n_rand = n - n_dup
    cells[:n_rand, 0] = rng.integers(0, 1 << 20, n_rand)
    cells[:n_rand, 1] = rng.integers(0, 1 << 20, n_rand)
    cells[:n_rand, 2] = rng.integers(0, 4, n_rand)
    cells[0] = (0, 0, 0)
    if n > 1:
        cells[1] = ((1 << 20) - 1, (1 << 20) - 1, 3)
    if n_dup:
        cells[n_rand:] = cells[rng.integers(0, n_rand, n_dup)]
    P = (cells + rng.uniform(0.1, 0.9, (n, 3))).astype(np.float32)
    assert (np.floor(P).astype(np.int64) == cells).all()
    return P[rng.permutation(n)]


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_tile_borders_and_wide_keys(gpu, n):
    """Point counts around the wave (64) and the sort block (T = GRID_SPARSE_TILE) sizes, one
    and several blocks; from n = 2 on the key space is 2^42 cells, so six 8-bit passes run."""
    P = _wide_cloud(n)
    got = _run(gpu, P, [n], 1.0, sparse=True)
    _assert_oracle(got, P, [n], 1.0)
    if n >= 2:
        assert got[2].max() == (1 << 42) - 1 and got[2].min() == 0
        assert len(got[0]) < n or n < 8                  # duplicates merged
        auto = _run(gpu, P, [n], 1.0, sparse='auto')
        for a, b in zip(got, auto):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------
# 3. a heavy voxel across blocks
# ---------------------------------------------------------------------------------------------
def test_heavy_voxel_across_blocks(gpu):
    """600 distinct points of one voxel scattered among 900 others (1501 points: two sort
    blocks), plus one far point that pushes the key space past 2^28. The barycentre is the
    oracle's index-order sum bit for bit, and a second run gives the same bits."""
    rng = np.random.default_rng(7)
    dl = 0.1
    heavy = (np.array([0.5, 0.7, 0.3]) + rng.uniform(0.005, 0.095, (600, 3))).astype(np.float32)
    assert len(np.unique(heavy, axis=0)) == 600
    others = rng.uniform(0.0, 3.0, (900, 3)).astype(np.float32)
    P = np.concatenate([heavy, others])[rng.permutation(1500)]
    P = np.concatenate([P, np.array([[100.0, 100.0, 100.0]], np.float32)])
    a = _run(gpu, P, [len(P)], dl, sparse='auto')
    b = _run(gpu, P, [len(P)], dl, sparse='auto')
    _assert_oracle(a, P, [len(P)], dl)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    o_pts, _, _ = og.grid_subsample(P, [len(P)], dl, return_keys=True)
    inside = np.all(np.floor(o_pts / np.float32(dl)) == np.array([5, 7, 3]), axis=1)
    assert inside.sum() == 1                             # the heavy voxel is there, once


# ---------------------------------------------------------------------------------------------
# 4. several clouds
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lidar_clouds():
    from fgreg.synthetic import lidar_like_pair
    src, tgt, _ = lidar_like_pair(0)
    return src, tgt


def test_several_clouds_with_empty_and_single(gpu):
    """Lengths [6000, 0, 1, 6000] at dl = 0.05: the lidar pair with an empty and a one-point
    cloud between its halves; with keys, and with the device layout."""
    import fgreg.ops as ops
    src, tgt = _lidar_clouds()
    one = np.array([[3.0, -2.0, 1.0]], np.float32)
    P, lens = np.concatenate([src, one, tgt]), [6000, 0, 1, 6000]
    got = _run(gpu, P, lens, 0.05, sparse='auto')
    _assert_oracle(got, P, lens, 0.05)
    assert got[1][1] == 0 and got[1][2] == 1
    pts, off = torch.from_numpy(P).to(gpu), ops.offsets(lens, gpu)
    sub, sl, len_dev, off_dev = ops.grid_subsample(pts, off, lens, 0.05, device_layout=True,
                                                   sparse='auto')
    assert np.array_equal(sub.cpu().numpy(), got[0]) and sl == got[1]
    assert len_dev.dtype == I64 and len_dev.tolist() == sl
    assert off_dev.tolist() == np.cumsum([0] + sl).tolist()


# ---------------------------------------------------------------------------------------------
# 5. dense and sparse agree where both apply
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['modelnet', 'indoor', 'edge', 'coincident'])
def test_dense_and_sparse_agree(gpu, case):
    if case == 'coincident':
        rng = np.random.default_rng(5)
        P = rng.uniform(-1, 1, (1000, 3)).astype(np.float32)
        P[rng.permutation(1000)[:600]] = np.array([0.3, -0.2, 0.1], np.float32)
        lens, dl = [400, 600], 0.05
    else:
        g = golden(f'geom_{case}')
        P, lens, dl = g['points'], [int(v) for v in g['lengths']], float(g['dl'])
    dense = _run(gpu, P, lens, dl, sparse=False)
    sparse = _run(gpu, P, lens, dl, sparse=True)
    auto = _run(gpu, P, lens, dl, sparse='auto')
    for d, s, a in zip(dense, sparse, auto):
        assert np.array_equal(d, s) and np.array_equal(d, a)
    _assert_oracle(sparse, P, lens, dl)


# ---------------------------------------------------------------------------------------------
# 6. limits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sparse', ['auto', True])
def test_axis_limit_is_reported(gpu, sparse):
    """More than 2^20 voxels along one axis: an FgrError, never a truncated key."""
    import fgreg
    P = np.array([[0, 0, 0], [2e6, 0, 0]], np.float32)
    with pytest.raises(fgreg.FgrError, match='key space'):
        _run(gpu, P, [2], 1.0, sparse=sparse)


# ---------------------------------------------------------------------------------------------
# 7. footprint
# ---------------------------------------------------------------------------------------------
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


def _ws_size(n, nc):
    from fgreg import _lib
    nb = _lib._sz(0)
    _ok(_L().fgr_grid_subsample_sparse_workspace(n, nc, nb), 'fgr_grid_subsample_sparse_workspace')
    return nb.value


FP_DL = 0.2


@functools.lru_cache(maxsize=None)
def _fp_clouds():
    rng = np.random.default_rng(0)
    lens = [300, 1, 65]
    P = np.concatenate([rng.uniform(-1, 1, (n, 3)).astype(np.float32) for n in lens])
    P[17] = np.float32(1000 * FP_DL)                      # a 1000^3-voxel first cloud
    return P, lens


def _fp_ops(ar):
    P, lens = _fp_clouds()
    pts = ar.put(torch.from_numpy(P), name='points')
    off = ar.put(torch.tensor(np.cumsum([0] + lens), dtype=I64), name='off')
    return P, lens, pts, off


@pytest.mark.parametrize('key_bits', [0, 31])
def test_sparse_footprint(gpu, key_bits):
    """fgr_grid_subsample_sparse_count / _fill over clouds of 300, 1 and 65 points (one point
    at (1000, 1000, 1000) dl) in exactly fgr_grid_subsample_sparse_workspace bytes: the clean
    and the 0xFF-prefilled runs are bit-equal and equal the oracle, all guards intact. With all
    eight passes launched (key_bits 0) and with the four a 31-bit hint allows."""
    P, lens = _fp_clouds()
    o_pts, o_lens, o_keys = og.grid_subsample(P, lens, FP_DL, return_keys=True)
    assert int(o_keys.max()) >= 1 << 28

    def run(ar):
        _, _, pts, off = _fp_ops(ar)
        n, nc = len(P), len(lens)
        need = _ws_size(n, nc)
        ws = ar.bytes(need, name='ws')
        counts = ar.vector(nc + 1, I64, 'out', name='counts')
        _ok(_L().fgr_grid_subsample_sparse_count(_p(pts), _p(off), nc, n, FP_DL, key_bits, _p(ws),
                                                 need, _p(counts), _st()),
            'fgr_grid_subsample_sparse_count')
        host = counts.cpu().tolist()
        assert host[:nc] == [int(v) for v in o_lens] and host[nc] == len(o_pts)
        out = ar.matrix(host[nc], 3, 3, F32, 'out', name='out_points')
        keys = ar.vector(host[nc], I64, 'out', name='out_keys')
        _ok(_L().fgr_grid_subsample_sparse_fill(n, nc, host[nc], _p(ws), need, _p(pts), _p(out),
                                                _p(keys), _st()), 'fgr_grid_subsample_sparse_fill')
        return out, keys, counts
    clean, poisoned = run_both(run, gpu)
    assert_both_equal(clean, poisoned)
    out, keys, _ = clean
    assert np.array_equal(out.cpu().numpy(), o_pts) and np.array_equal(keys.cpu().numpy(), o_keys)


def test_sparse_key_bits_hint_too_small_is_reported(gpu):
    """A key_bits hint below what the key space needs (30 bits here) is reported as -3 with
    zero counts, not sorted on too few digits."""
    P, lens = _fp_clouds()
    ar = Arena(gpu, poison=True)
    _, _, pts, off = _fp_ops(ar)
    n, nc = len(P), len(lens)
    need = _ws_size(n, nc)
    ws = ar.bytes(need, name='ws')
    counts = ar.vector(nc + 1, I64, 'out', name='counts')
    _ok(_L().fgr_grid_subsample_sparse_count(_p(pts), _p(off), nc, n, FP_DL, 16, _p(ws), need,
                                             _p(counts), _st()), 'fgr_grid_subsample_sparse_count')
    assert counts.cpu().tolist() == [0, 0, 0, -3]
    ar.check()


@pytest.mark.parametrize('which', ['count', 'fill'])
def test_sparse_refuses_short_workspace(gpu, which):
    """ws_bytes 16 below the reported size is refused before the first launch: non-zero
    status, a message, outputs and workspace untouched."""
    P, lens = _fp_clouds()
    n, nc = len(P), len(lens)
    ar = Arena(gpu, poison=True)
    _, _, pts, off = _fp_ops(ar)
    need = _ws_size(n, nc)
    ws = ar.bytes(need, name='ws')
    counts = ar.vector(nc + 1, I64, 'out', name='counts')
    out = ar.matrix(n, 3, 3, F32, 'out', name='out_points')
    if which == 'count':
        rc = _L().fgr_grid_subsample_sparse_count(_p(pts), _p(off), nc, n, FP_DL, 0, _p(ws),
                                                  need - 16, _p(counts), _st())
    else:
        rc = _L().fgr_grid_subsample_sparse_fill(n, nc, n, _p(ws), need - 16, _p(pts), _p(out),
                                                 None, _st())
    torch.cuda.synchronize()
    assert rc != 0 and b'workspace' in _L().fgr_last_error()
    for reg in ar.regions:
        reg.full = False
    ar.check()
    assert bool((ws == 0xFF).all())
    assert all(bool((reg.view.view(torch.int32) == 0x7FC5A5A5).all())
               for reg in ar.regions if reg.role == 'out')


def test_sparse_workspace_ignores_the_extent():
    """The workspace is a function of (n_points, n_clouds) alone and grows linearly."""
    a, b = _ws_size(12000, 2), _ws_size(24000, 2)
    assert 0 < a < 12000 * 64 and b < 2 * a + 4096


# ---------------------------------------------------------------------------------------------
# 8. / 9. the pyramid and the forward on a lidar-like pair
# ---------------------------------------------------------------------------------------------
MODES = {'ball_query': og.INDEX, 'nanoflann': og.DIST}


@functools.lru_cache(maxsize=None)
def _oracle_meta(mode):
    cfg = forward_fixture('forward_3dmatch_small')[0]
    src, tgt = _lidar_clouds()
    return mo.preprocess(cfg, [src, tgt], mode=MODES[mode])


@pytest.mark.parametrize('mode', ['ball_query', 'nanoflann'])
def test_pyramid_on_lidar_like_pair(gpu, mode, monkeypatch):
    """PreprocessorHIP on lidar_like_pair(0) with the 3DMatch fixture's cfg (first pooling voxel
    0.05 m: past the dense limit, tests/test_sparse_grid_inputs.py): every level's points, stack
    lengths, neighbours, pools and upsamples equal the oracle's, and the first level did go
    through the sparse path."""
    import fgreg
    from fgreg import ops
    cfg = forward_fixture('forward_3dmatch_small')[0]
    src, tgt = _lidar_clouds()
    want = _oracle_meta(mode)
    pre = fgreg.PreprocessorHIP(cfg, neighbor_mode=mode)
    sparse_calls, inner = [], ops._grid_subsample_sparse
    monkeypatch.setattr(ops, '_grid_subsample_sparse',
                        lambda pts, *a: (sparse_calls.append(int(pts.shape[0])), inner(pts, *a))[1])
    meta = pre([torch.from_numpy(src).to(gpu), torch.from_numpy(tgt).to(gpu)])
    assert sparse_calls and sparse_calls[0] == 12000
    assert len(want['points']) == 4
    for key in ('points', 'stack_lengths', 'neighbors', 'pools', 'upsamples'):
        assert len(meta[key]) == len(want[key])
        for lvl, (a, b) in enumerate(zip(meta[key], want[key])):
            assert np.array_equal(a.cpu().numpy(), b.numpy()), (key, lvl)


def _bits_equal(a, b, what=''):
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _bits_equal(x, y, f'{what}[{i}]')
    else:
        assert bit_equal(a.detach(), b.detach()), what


OUT_KEYS = ('pose', 'src_feat', 'tgt_feat', 'src_kp', 'tgt_kp', 'src_kp_warped', 'tgt_kp_warped',
            'src_overlap', 'tgt_overlap')


def test_forward_on_lidar_like_pair(gpu, guarded_scratch):
    """RegTR with the 3DMatch fixture's weights on the lidar-like pair, with its own
    preprocessor: bit-equal to the same model on the oracle's meta (FixedMetaPreprocessor), to a
    run over guarded exact-size scratch, and to fgreg.pipeline(model, [batch, batch])."""
    import fgreg
    cfg, sd, *_ = forward_fixture('forward_3dmatch_small')
    src, tgt = _lidar_clouds()

    def model_():
        m = fgreg.RegTR(cfg)
        m.load_state_dict(sd, strict=False)
        return m.to(gpu).eval()

    def batch_():
        return {'src_xyz': [torch.from_numpy(src).to(gpu)], 'tgt_xyz': [torch.from_numpy(tgt).to(gpu)]}

    def outs(o):
        return [o[k] if torch.is_tensor(o[k]) else list(o[k]) for k in OUT_KEYS]

    with torch.no_grad():
        model = model_()
        batch = batch_()
        own = outs(model(batch))
        levels = batch['kpconv_meta']['stack_lengths']
        assert len(levels) == 4 and int(levels[1].sum()) < 12000      # the pyramid was built
        fixed = model_()
        fixed.preprocessor = fgreg.FixedMetaPreprocessor(
            {k: [t.to(gpu) for t in v] for k, v in _oracle_meta('ball_query').items()})
        _bits_equal(own, outs(fixed(batch_())), 'oracle meta')
        with guarded_scratch():
            guarded = outs(model_()(batch_()))
            torch.cuda.synchronize()
        _bits_equal(own, guarded, 'guarded scratch')
        piped = list(fgreg.pipeline(model, [batch_(), batch_()]))
        torch.cuda.synchronize()
        assert len(piped) == 2
        for i, o in enumerate(piped):
            _bits_equal(own, outs(o), f'pipeline[{i}]')
