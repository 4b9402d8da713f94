"""The loss, pose and metric kernels (csrc/loss.hip, csrc/pose.hip, csrc/metrics.hip) row by row
against fp64 (tests/_tail_ref.py, pinned on the CPU by tests/test_tail_ref.py), called through
the C ABI with every operand carved out of a guarded arena (tests/_arena.py): each case runs on
a clean and on a poisoned arena with bit-identical results, strided operands (ld = cols + 4)
keep their sentinel / poisoned pad columns, workspaces are exactly the bytes the library asks
for. Shapes are the smallest at which the kernels can still go wrong: lane 63 / 64 / 65, rows
that are no multiple of a block's four waves, empty segments, 1023 / 1024 / 1025 elements of the
single-block reductions, 255 / 256 / 257 points of a 256-thread block, the 2048-point LDS stage.

Discrete contracts (row masks, the positive's column, zero patterns of dlogits, NaN patterns,
R = I for a pair without a weight over the threshold) are compared exactly. Values are compared
at BOUNDS below: worst error of each family measured on the MI355X against the fp64 reference
(the kernels are deterministic: the factor <= 4 only absorbs a compiler reordering one fma),
never looser than the bound the project already used for the family.

Errors are |got - ref| / max(1, |ref|) per element unless said otherwise.

  family (entry points)                          measured   asserted   bound before
  infonce_row     fgr_infonce_rows row_loss      1.28e-07   5.0e-07    1e-5
  infonce_scalar  fgr_infonce_reduce             9.66e-08   3.0e-07    1e-5
  infonce_dlogits fgr_infonce_rows_bwd           1.15e-07   4.5e-07    (GRAD_TOL, whole model)
  pair_cdist      fgr_pair_cdist                 3.68e-07   1.4e-06    1e-5 (through the loss)
  circle          fgr_circle_loss                1.62e-08   6.0e-08    1e-5
  bce             fgr_bce_logits_mean            1.09e-07   4.0e-07    1e-5
  transform       fgr_transform_points           1.19e-07   4.7e-07    1e-5 (through the loss)
  corr            fgr_corr_loss                  2.87e-08   1.1e-07    1e-5
  overlap_pool    fgr_overlap_pool               1.84e-07   7.0e-07    1e-6 rel + 1e-7
  se3_cos         fgr_se3_compare, cos(angle)    2.50e-07   9.5e-07    2e-6
  se3_deg         ... angle, 1 <= theta <= 179   5.20e-05   2.0e-04    1e-3 degrees
  se3_trans       ... translation error          9.99e-08   3.9e-07    1e-5
  pose            fgr_procrustes, fgr_pair_pose  2.98e-08   1.1e-07    1e-4
  ortho           collinear: R^T R - I, det - 1  3.00e-08   1.15e-07   1e-6 (the issue's)
  metrics_*       fgr_modelnet_metrics, relative to the array's largest value:
    r_mse 1.37e-15 -> 5.4e-15, r_mae 1.14e-15 -> 4.5e-15 (fp64 on both sides), t_mse 1.14e-07
    -> 4.5e-07, t_mae 8.85e-08 -> 3.5e-07, err_t 7.28e-08 -> 2.9e-07, chamfer_dist 2.66e-07 ->
    1.0e-06; err_r_deg 1.71e-05 -> 6.5e-05 degrees absolute on the pairs with pred != gt (for
    pred == gt the kernel returns, as the reference does, acos of a float32 trace: up to 0.03
    degrees, inside check_modelnet_metrics' floor). All also pass check_modelnet_metrics(1e-4).
The collinear case's weighted residual is 1 + 1.3e-7 times the fp64 optimum (bound 1 + 1e-6).

Shown on scratch builds (not committed) to fail when the kernel is broken:
  the nearest-positive tie-break comparing oj > bj -- forward: row_loss of the tied rows
  (errors 0.2 .. 4.0), backward: the positive's column / the zero pattern, both in
  test_infonce_rows_reduce_bwd[lattice-*, pm80, no-kept-row];
  fgr_infonce_rows_bwd not zeroing columns >= p1 -- every test_infonce_rows_reduce_bwd case
  (dlogits elements never written);
  block_sum adding nw - 1 waves -- test_bce_logits_mean[1024 / 1025 / 3000],
  test_corr_loss[False], test_infonce_reduce_sizes, test_circle_loss[long].
"""
import functools
import math

import numpy as np
import pytest
import torch

import _tail_ref as tr
import metrics_oracle as mt
from _arena import assert_both_equal, run_both
from test_oracle import check_modelnet_metrics

pytestmark = pytest.mark.gpu
F32, F64, I64 = torch.float32, torch.float64, torch.int64

# family -> asserted bound on |got - ref| / max(1, |ref|) unless said otherwise
BOUNDS = {
    'infonce_row': 5e-7, 'infonce_scalar': 3e-7, 'infonce_dlogits': 4.5e-7,
    'pair_cdist': 1.4e-6, 'circle': 6e-8, 'bce': 4e-7, 'transform': 4.7e-7, 'corr': 1.1e-7,
    'overlap_pool': 7e-7,
    'se3_cos': 9.5e-7,          # absolute, on the cosine
    'se3_deg': 2e-4,          # absolute, degrees, 1 <= theta <= 179
    'se3_trans': 3.9e-7,
    'pose': 1.1e-7,           # |dR|, |dt| / max(1, max|t|)
    'ortho': 1.15e-7,         # R^T R = I, det R = 1 (collinear clouds)
    # ModelNet metrics, relative to the array's largest value (check_modelnet_metrics' form)
    'metrics_r_mse': 5.4e-15, 'metrics_r_mae': 4.5e-15, 'metrics_t_mse': 4.5e-7,
    'metrics_t_mae': 3.5e-7, 'metrics_err_t': 2.9e-7, 'metrics_chamfer_dist': 1e-6,
    'metrics_err_r_deg': 6.5e-5,    # absolute, degrees, the pairs with pred != gt
}


def _check(family, err, what=''):
    """Prints the figure (the measurement), then asserts it."""
    err = float(err)
    print(f'MEASURE {family} {err:.3e} bound {BOUNDS[family]:.1e} {what}')
    assert err <= BOUNDS[family], (family, what, err, BOUNDS[family])


def _relmax(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def _L():
    from fgreg import _lib
    return _lib.load()


def _ok(rc, name):
    from fgreg import _lib
    _lib.check(rc, name)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr()


def _size(fn, *args):
    from fgreg import _lib
    nb = _lib._sz(0)
    _ok(getattr(_L(), fn)(*args, nb), fn)
    return nb.value


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _both(fn, gpu):
    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    one = torch.is_tensor(clean)
    out = tuple(t.cpu().numpy() for t in ((clean,) if one else clean))
    return out[0] if one else out


def _same_nan(got, ref):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)


# ---------------------------------------------------------------------------------------------
# InfoNCE: fgr_infonce_rows, fgr_infonce_reduce, fgr_infonce_rows_bwd
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _infonce_ref(name):
    x = tr.infonce_inputs(name)
    args = (x['logits'], x['axyz'], x['pxyz'], x['a_off'], x['p_off'])
    pos, mask, rl, s = tr.infonce_rows(*args)
    dl = tr.infonce_dlogits(*args, g=tr.INFONCE_G)
    return x, pos, mask, rl, s, dl, tr.infonce_row_weight(mask, x['a_off'])


@pytest.mark.parametrize('name', list(tr.INFONCE_CASES))
def test_infonce_rows_reduce_bwd(gpu, name):
    x, pos, mask, rl_ref, s_ref, dl_ref, w = _infonce_ref(name)
    n_a, n_cols, n_pairs = len(pos), x['n_cols'], len(x['a_off']) - 1
    ld = n_cols + 4
    L = _L()

    def fn(ar):
        lg = ar.put(_t(x['logits']), ld=ld, name='logits')
        ax, px = ar.put(_t(x['axyz']), name='axyz'), ar.put(_t(x['pxyz']), name='pxyz')
        ao, po = ar.put(_t(x['a_off']), name='a_off'), ar.put(_t(x['p_off']), name='p_off')
        rl, rm = ar.vector(n_a, F32, 'out', 'row_loss'), ar.vector(n_a, F32, 'out', 'row_mask')
        _ok(L.fgr_infonce_rows(_p(lg), ld, _p(ax), _p(px), _p(ao), _p(po), n_pairs, n_a, tr.R_P,
                               tr.R_N, _p(rl), _p(rm), _st()), 'fgr_infonce_rows')
        out = ar.vector(1, F32, 'out', 'loss')
        _ok(L.fgr_infonce_reduce(_p(rl), _p(rm), _p(ao), n_pairs, _p(out), _st()),
            'fgr_infonce_reduce')
        wt, g = ar.put(_t(w), name='row_weight'), ar.put(torch.tensor([tr.INFONCE_G]), name='g')
        dl = ar.matrix(n_a, n_cols, ld, F32, 'out', 'dlogits')
        _ok(L.fgr_infonce_rows_bwd(_p(lg), ld, _p(ax), _p(px), _p(ao), _p(po), n_pairs, n_a, n_cols,
                                   tr.R_N, _p(wt), _p(g), _p(dl), ld, _st()), 'fgr_infonce_rows_bwd')
        return rl, rm, out, dl

    rl, rm, out, dl = _both(fn, gpu)
    assert np.array_equal(rm, mask.astype(np.float32)), (rm, mask)
    _same_nan(rl, rl_ref)
    fin = ~np.isnan(rl_ref)
    _check('infonce_row', _relmax(rl[fin], rl_ref[fin]), name)
    _same_nan(out, np.array([s_ref]))
    if not math.isnan(s_ref):
        _check('infonce_scalar', _relmax(out, [s_ref]), name)
    # dlogits: exact zeros outside the row's pair block (padding included), on ignored columns
    # and on every column of an unkept row; the rest element-wise against autograd
    zero = np.ones((n_a, n_cols), bool)
    for b in range(n_pairs):
        a0, a1, p0, p1 = (int(v) for v in (*x['a_off'][b:b + 2], *x['p_off'][b:b + 2]))
        if a1 > a0 and p1 > p0:
            ign = tr.point_dist(x['axyz'][a0:a1], x['pxyz'][p0:p1]) < tr.R_N
            ign[np.arange(a1 - a0), pos[a0:a1] - p0] = False
            zero[a0:a1, p0:p1] = ign | ~mask[a0:a1, None]
    assert (dl_ref[zero] == 0).all()
    assert (dl[zero] == 0).all(), np.argwhere(zero & (dl != 0))[:5]
    assert np.isfinite(dl).all()
    _check('infonce_dlogits', _relmax(dl, dl_ref), name)
    # the positive's column: the one negative entry of a kept row (softmax - 1 < 0), unless the
    # positive's softmax rounds to 1 (reference gradient above -1e-6 of the row's weight)
    for i in np.flatnonzero(mask):
        neg = set(np.flatnonzero(dl[i] < 0).tolist())
        assert neg <= {int(pos[i])}, (i, neg, pos[i])
        if dl_ref[i, pos[i]] < -1e-6 * tr.INFONCE_G * w[i]:
            assert neg == {int(pos[i])}, (i, neg, pos[i])
    if name == 'only-positive':
        assert mask.any() and np.abs(rl).max() <= 1e-6 and (dl == 0).all()


@pytest.mark.parametrize('a_lens', [[1023, 1], [1024, 0, 1025], [7, 2000, 3]], ids=str)
def test_infonce_reduce_sizes(gpu, a_lens):
    """fgr_infonce_reduce alone on given rows, around and past the 1024 threads of its block;
    unkept rows hold NaN (as the rows of an empty positive cloud do) and must not count."""
    rng = np.random.default_rng(sum(a_lens))
    a_off = tr.offsets(a_lens)
    n = int(a_off[-1])
    mask = rng.random(n) < 0.8
    mask[a_off[:-1][np.asarray(a_lens) > 0]] = True     # a kept row in every non-empty pair
    mask[a_off[1:][np.asarray(a_lens) > 0] - 1] = True  # and its last row (the last wave's)
    loss = rng.uniform(0.0, 9.0, n).astype(np.float32)
    loss[~mask] = np.nan
    terms = [loss[a_off[b]:a_off[b + 1]][mask[a_off[b]:a_off[b + 1]]].astype(np.float64).sum() /
             max(int(mask[a_off[b]:a_off[b + 1]].sum()), 1) if a_lens[b] else np.nan
             for b in range(len(a_lens))]
    ref = float(np.mean(terms))

    def fn(ar):
        rl, rm = ar.put(_t(loss), name='row_loss'), ar.put(_t(mask.astype(np.float32)), name='row_mask')
        ao = ar.put(_t(a_off), name='a_off')
        out = ar.vector(1, F32, 'out', 'loss')
        _ok(_L().fgr_infonce_reduce(_p(rl), _p(rm), _p(ao), len(a_lens), _p(out), _st()),
            'fgr_infonce_reduce')
        return out

    out = _both(fn, gpu)
    _same_nan(out, np.array([ref]))
    assert math.isnan(ref) == (0 in a_lens)
    if not math.isnan(ref):
        _check('infonce_scalar', _relmax(out, [ref]), f'reduce {a_lens}')


# ---------------------------------------------------------------------------------------------
# Circle: fgr_pair_cdist, fgr_circle_loss
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', tr.CDIST_DIMS)
def test_pair_cdist(gpu, d):
    x = tr.cdist_inputs(d)
    n_pairs, fd_elems = len(x['a_lens']), int(x['fd_off'][-1])
    ref = np.concatenate([f.ravel() for f in tr.pair_cdist(x['af'], x['pf'], x['a_off'], x['p_off'])])

    def fn(ar):
        af, pf = ar.put(_t(x['af']), name='af'), ar.put(_t(x['pf']), name='pf')
        ao, po, fo = (ar.put(_t(x[k]), name=k) for k in ('a_off', 'p_off', 'fd_off'))
        fd = ar.vector(fd_elems, F32, 'out', 'fd')
        _ok(_L().fgr_pair_cdist(_p(af), _p(pf), d, _p(ao), _p(po), _p(fo), n_pairs,
                                max(x['a_lens']), max(x['p_lens']), _p(fd), _st()), 'fgr_pair_cdist')
        return fd

    fd = _both(fn, gpu)
    _check('pair_cdist', _relmax(fd, ref), f'd={d}')
    i_eq = int(x['fd_off'][1]) + 0 * 17 + 3            # anchor row 0 == positive row 3 of pair 1
    assert abs(ref[i_eq] - 1e-6) < 1e-18 and abs(fd[i_eq] - 1e-6) <= 1e-11, fd[i_eq]


@pytest.mark.parametrize('name', list(tr.CIRCLE_CASES))
def test_circle_loss(gpu, name):
    x = tr.circle_inputs(name)
    _, ref = tr.circle_lines(x['af'], x['pf'], x['axyz'], x['pxyz'], x['a_off'], x['p_off'])
    n_pairs, fd_elems = len(x['a_lens']), int(x['fd_off'][-1])
    n_a, n_p = sum(x['a_lens']), sum(x['p_lens'])
    need = _size('fgr_circle_loss_workspace', fd_elems, n_a, n_p)
    assert need == 4 * (fd_elems + 2 * (n_a + n_p))

    def fn(ar):
        af, pf = ar.put(_t(x['af']), name='af'), ar.put(_t(x['pf']), name='pf')
        ax, px = ar.put(_t(x['axyz']), name='axyz'), ar.put(_t(x['pxyz']), name='pxyz')
        ao, po, fo = (ar.put(_t(x[k]), name=k) for k in ('a_off', 'p_off', 'fd_off'))
        ws = ar.bytes(need, name='ws')
        out = ar.vector(1, F32, 'out', 'loss')
        _ok(_L().fgr_circle_loss(_p(af), _p(pf), x['d'], _p(ax), _p(px), _p(ao), _p(po), _p(fo),
                                 n_pairs, n_a, n_p, max(x['a_lens']), max(x['p_lens']), fd_elems,
                                 tr.R_P, tr.R_N, _p(ws), need, _p(out), _st()), 'fgr_circle_loss')
        return out

    out = _both(fn, gpu)
    assert math.isnan(ref) != x['finite']
    _same_nan(out, np.array([ref]))
    if x['finite']:
        _check('circle', _relmax(out, [ref]), name)


# ---------------------------------------------------------------------------------------------
# Small reductions and maps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 3])
@pytest.mark.parametrize('n', [1, 63, 1024, 1025, 3000])
def test_bce_logits_mean(gpu, n, stride):
    rng = np.random.default_rng(n + stride)
    xs = (rng.normal(size=n) * 4).astype(np.float32)
    special = np.array([-90, 90, 20, -20, 0], np.float32)
    xs[:min(n, 5)] = special[:min(n, 5)]
    ys = rng.random(n).astype(np.float32)
    ref = tr.bce_mean(xs, ys)

    def fn(ar):
        xd = ar.put(_t(xs.reshape(n, 1)), ld=stride, name='x')
        yd = ar.put(_t(ys), name='y')
        out = ar.vector(1, F32, 'out', 'loss')
        _ok(_L().fgr_bce_logits_mean(_p(xd), stride, _p(yd), n, _p(out), _st()),
            'fgr_bce_logits_mean')
        return out

    _check('bce', _relmax(_both(fn, gpu), [ref]), f'n={n} stride={stride}')


@pytest.mark.parametrize('inverse', [0, 1])
def test_transform_points(gpu, inverse):
    lens = [5, 0, 300, 1]
    rng = np.random.default_rng(11 + inverse)
    seg_off = tr.offsets(lens)
    n = int(seg_off[-1])
    xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    pose = np.stack([tr.random_pose(rng) for _ in lens]).astype(np.float32)
    ref = tr.transform_points(xyz, seg_off, pose, bool(inverse))

    def fn(ar):
        xd, so = ar.put(_t(xyz), name='xyz'), ar.put(_t(seg_off), name='seg_off')
        pd = ar.put(_t(pose.reshape(len(lens), 12)), name='pose')
        out = ar.matrix(n, 3, 3, F32, 'out', 'out')
        _ok(_L().fgr_transform_points(_p(xd), n, _p(so), len(lens), _p(pd), inverse, _p(out),
                                      _st()), 'fgr_transform_points')
        return out

    _check('transform', _relmax(_both(fn, gpu), ref), f'inverse={inverse}')


@pytest.mark.parametrize('tgt_zero', [False, True])
def test_corr_loss(gpu, tgt_zero):
    lens = [3, 0, 1100, 2]                              # src_0, src_1 | tgt_0, tgt_1
    rng = np.random.default_rng(21)
    seg_off = tr.offsets(lens)
    n = int(seg_off[-1])
    xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    pose = np.stack([tr.random_pose(rng) for _ in range(2)]).astype(np.float32)
    want = tr.transform_points(xyz, seg_off, np.concatenate([pose, tr.pose_inverse(pose)]))
    corr = (want + rng.normal(size=(n, 3)) * 0.05).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    if tgt_zero:
        w[3:] = 0
    ref = tr.corr_loss(xyz, corr, w, seg_off, 2, pose)
    if tgt_zero:                                        # the 1e-6 clamp: 0 for that direction
        assert ref == tr.corr_loss(xyz[:3], corr[:3], w[:3], np.array([0, 3, 3, 3, 3]), 2, pose)

    def fn(ar):
        xd, cd, wd = ar.put(_t(xyz), name='xyz'), ar.put(_t(corr), name='corr'), ar.put(_t(w), name='w')
        so, pd = ar.put(_t(seg_off), name='seg_off'), ar.put(_t(pose.reshape(2, 12)), name='pose')
        out = ar.vector(1, F32, 'out', 'loss')
        _ok(_L().fgr_corr_loss(_p(xd), _p(cd), _p(wd), _p(so), 2, _p(pd), _p(out), _st()),
            'fgr_corr_loss')
        return out

    out = _both(fn, gpu)
    assert np.isfinite(out).all()
    _check('corr', _relmax(out, [ref]), f'tgt_zero={tgt_zero}')


@pytest.mark.parametrize('width', [1, 40])
@pytest.mark.parametrize('nq', [1, 257])
def test_overlap_pool(gpu, nq, width):
    n_prev = 50
    rng = np.random.default_rng(nq + width)
    prev = rng.uniform(-0.2, 1.2, n_prev).astype(np.float32)         # the clamp has work to do
    idx = rng.integers(-n_prev, n_prev + 1, (nq, width)).astype(np.int64)   # n_prev: the shadow
    idx[0, 0] = -3
    if nq > 1:
        idx[1, 0], idx[2, 0], idx[3, 0] = n_prev - 1, -n_prev, 0
        idx[100] = n_prev                                            # no valid entry: NaN
        idx[nq - 1, :] = -1
    ref = tr.overlap_pool(prev, idx)
    assert (nq == 1) or (math.isnan(ref[100]) and np.isnan(ref).sum() < nq // 4)
    assert (idx < 0).any() and (nq == 1 or (idx == n_prev).any())

    def fn(ar):
        pv, ix = ar.put(_t(prev), name='prev'), ar.put(_t(idx), name='idx')
        out = ar.vector(nq, F32, 'out', 'out')
        _ok(_L().fgr_overlap_pool(_p(pv), n_prev, _p(ix), nq, width, _p(out), _st()),
            'fgr_overlap_pool')
        return out

    out = _both(fn, gpu)
    _same_nan(out, ref)
    fin = ~np.isnan(ref)
    _check('overlap_pool', _relmax(out[fin], ref[fin]), f'nq={nq} width={width}')
    np.testing.assert_allclose(out[fin], ref[fin], rtol=1e-6, atol=1e-7)    # test_gpu_loss's form


def test_se3_compare(gpu):
    L_, B = 6, 13                                       # 78 units: more than one 64-thread block
    rng = np.random.default_rng(31)
    gt = np.stack([tr.random_pose(rng) for _ in range(B)]).astype(np.float32)
    angles = [0.0, math.degrees(1e-3), 90.0, 179.9]
    pred = np.empty((L_, B, 3, 4), np.float32)
    for l in range(L_):
        for b in range(B):
            u = l * B + b
            deg = angles[u] if u < len(angles) else rng.uniform(5.0, 175.0)
            R = tr.rotation(rng.normal(size=3), deg) @ gt[b, :, :3].astype(np.float64)
            t = gt[b, :, 3] + rng.normal(size=3) * (0.0 if u == 0 else 0.1)
            pred[l, b] = np.concatenate([R, t[:, None]], 1)
    pred[3, 7] = gt[7]                                  # bit-equal to gt
    c_ref, deg_ref, t_ref = tr.se3_compare(pred, gt)

    def fn(ar):
        pd, gd = ar.put(_t(pred.reshape(L_ * B, 12)), name='pred'), ar.put(_t(gt.reshape(B, 12)), name='gt')
        rot, trn = ar.matrix(L_, B, B, F32, 'out', 'rot'), ar.matrix(L_, B, B, F32, 'out', 'trans')
        _ok(_L().fgr_se3_compare(_p(pd), _p(gd), L_, B, _p(rot), _p(trn), _st()), 'fgr_se3_compare')
        return rot, trn

    rot, trn = _both(fn, gpu)
    assert np.isfinite(rot).all() and (rot >= 0).all() and (rot <= 180).all()
    _check('se3_cos', np.abs(np.cos(np.radians(rot.astype(np.float64))) - c_ref).max())
    mid = (deg_ref >= 1.0) & (deg_ref <= 179.0)
    assert mid.sum() >= L_ * B - 6
    _check('se3_deg', np.abs(rot - deg_ref)[mid].max())
    _check('se3_trans', _relmax(trn, t_ref))
    assert rot[3, 7] < 0.1 and trn[3, 7] < 1e-6         # float32 rounding of R R^T only


# ---------------------------------------------------------------------------------------------
# Pose: fgr_procrustes, fgr_pair_pose
# ---------------------------------------------------------------------------------------------
def _pose_err(got, ref):
    """conftest's 1e-4 as test_gpu_kernels.test_procrustes_vs_reference applies it: the rotation
    absolute, the translation relative to max(1, max|t|)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return max(float(np.abs(got[..., :3] - ref[..., :3]).max()),
               float(np.abs(got[..., 3] - ref[..., 3]).max()) / max(1.0, float(np.abs(ref[..., 3]).max())))


def _procrustes(gpu, a, b, w, thr):
    nb, n = w.shape

    def fn(ar):
        ad, bd = ar.put(_t(a.reshape(nb * n, 3)), name='a'), ar.put(_t(b.reshape(nb * n, 3)), name='b')
        wd = ar.put(_t(w.reshape(-1)), name='w')
        out = ar.matrix(nb, 12, 12, F32, 'out', 'pose')
        _ok(_L().fgr_procrustes(_p(ad), _p(bd), _p(wd), nb, n, thr, _p(out), _st()), 'fgr_procrustes')
        return out

    return _both(fn, gpu).reshape(nb, 3, 4)


def _rigid_problem(rng, nb, n, noise=0.01):
    a = rng.uniform(-1, 1, (nb, n, 3))
    T = np.stack([tr.random_pose(rng) for _ in range(nb)])
    b = a @ np.swapaxes(T[:, :, :3], 1, 2) + T[:, None, :, 3] + rng.normal(size=a.shape) * noise
    return a.astype(np.float32), b.astype(np.float32)


@pytest.mark.parametrize('thr', [0.85, -1.0])
@pytest.mark.parametrize('n', [3, 4, 255, 256, 257, 1000])
def test_procrustes(gpu, n, thr):
    rng = np.random.default_rng(n)
    a, b = _rigid_problem(rng, 3, n)
    w = tr.weights_away_from(rng, 3 * n).reshape(3, n)
    w[:, :3] = rng.uniform(0.9, 1.0, (3, 3)).astype(np.float32)     # three points always count
    assert (np.abs(w.astype(np.float64) - 0.85) >= 1e-3).all()
    got = _procrustes(gpu, a, b, w, thr)
    ref = np.stack([tr.kabsch(a[i], b[i], w[i], thr) for i in range(3)])
    _check('pose', _pose_err(got, ref), f'procrustes n={n} thr={thr}')


def test_pair_pose(gpu):
    n_pairs, n_layers, thr = 3, 2, 0.85
    lens = [200, 1, 40, 60, 300, 0]                     # src_0..2 | tgt_0..2
    seg_off = tr.offsets(lens)
    n_tot = int(seg_off[-1])
    rng = np.random.default_rng(41)
    xyz = rng.uniform(-1, 1, (n_tot, 3)).astype(np.float32)
    pose = np.stack([tr.random_pose(rng) for _ in range(n_pairs)])
    want = tr.transform_points(xyz, seg_off, np.concatenate([pose, tr.pose_inverse(pose)]))
    corr = (want[None] + rng.normal(size=(n_layers, n_tot, 3)) * 0.02).astype(np.float32)
    logits = tr.logits_away_from(rng, n_layers * n_tot, thr).reshape(n_layers, n_tot)
    dead = slice(int(seg_off[2]), int(seg_off[3]))      # layer 1, pair 2 (tgt empty): every
    logits[1, dead] = -2.0                              # weight under the threshold
    logits[0, dead][:4] = 4.0
    logits[:, int(seg_off[1])] = 4.0                    # the one-point src cloud counts
    ref = tr.pair_pose(xyz, corr, logits, seg_off, n_pairs, thr)

    def fn(ar):
        xd = ar.put(_t(xyz), name='xyz')
        cd = ar.put(_t(corr.reshape(n_layers * n_tot, 3)), name='corr')
        ld = ar.put(_t(logits.reshape(-1)), name='logits')
        so = ar.put(_t(seg_off), name='seg_off')
        out = ar.matrix(n_layers * n_pairs, 12, 12, F32, 'out', 'pose')
        _ok(_L().fgr_pair_pose(_p(xd), _p(cd), _p(ld), n_tot, _p(so), n_pairs, n_layers, thr,
                               _p(out), _st()), 'fgr_pair_pose')
        return out

    got = _both(fn, gpu).reshape(n_layers, n_pairs, 3, 4)
    for l in range(n_layers):
        for p in range(n_pairs):
            _check('pose', _pose_err(got[l, p], ref[l, p]), f'pair_pose layer {l} pair {p}')
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    assert np.array_equal(ref[1, 2], eye) and np.array_equal(got[1, 2], eye.astype(np.float32))
    assert not np.array_equal(got[0, 2], eye.astype(np.float32))


def _weights(rng, n):
    return rng.uniform(0.1, 1.0, (1, n)).astype(np.float32)


def test_procrustes_coplanar(gpu):
    """Rank-2 covariance (the source points in one plane): R is still unique."""
    rng = np.random.default_rng(51)
    for tilt in (False, True):
        a = rng.uniform(-1, 1, (1, 60, 3))
        a[..., 2] = 0.0
        if tilt:
            a = a @ tr.rotation([1, 2, 3], 33.0).T + 0.3
        a = a.astype(np.float32)
        T = tr.random_pose(rng)
        b = (a.astype(np.float64) @ T[:, :3].T + T[:, 3] + rng.normal(size=a.shape) * 0.01).astype(np.float32)
        w = _weights(rng, 60)
        got = _procrustes(gpu, a, b, w, -1.0)
        _check('pose', _pose_err(got[0], tr.kabsch(a[0], b[0], w[0], -1.0)), f'coplanar tilt={tilt}')


def test_procrustes_mirrored(gpu):
    """A mirrored cloud: det(V U^T) < 0, the reflection branch."""
    rng = np.random.default_rng(52)
    a = (rng.uniform(-1, 1, (1, 80, 3)) * (1.0, 0.7, 0.4)).astype(np.float32)
    T = tr.random_pose(rng)
    b = (a.astype(np.float64) * (1, 1, -1)) @ T[:, :3].T + T[:, 3] + rng.normal(size=a.shape) * 0.01
    b = b.astype(np.float32)
    w = _weights(rng, 80)
    H = (a[0] - a[0].mean(0)).astype(np.float64).T @ (b[0] - b[0].mean(0)).astype(np.float64)
    assert np.linalg.det(H) < 0
    got = _procrustes(gpu, a, b, w, -1.0)
    _check('pose', _pose_err(got[0], tr.kabsch(a[0], b[0], w[0], -1.0)), 'mirrored')


@pytest.mark.parametrize('exact', [True, False])
def test_procrustes_collinear(gpu, exact):
    """Rank-1 covariance (the source points on one line): R is not unique, so the properties of
    a solution are asserted -- a proper rotation whose weighted residual is the optimum's.
    exact: a line along (1, 2, 2) / 8 whose float32 coordinates are exactly collinear."""
    rng = np.random.default_rng(53)
    k = rng.integers(-16, 17, 40).astype(np.float64)
    direction = np.array([1.0, 2.0, 2.0]) / 8 if exact else np.array([0.3, -0.5, 0.81])
    a = (k[:, None] * direction + (0.0 if exact else 0.21)).astype(np.float32)[None]
    T = tr.random_pose(rng)
    b = (a.astype(np.float64) @ T[:, :3].T + T[:, 3] + rng.normal(size=a.shape) * 0.01).astype(np.float32)
    w = _weights(rng, 40)
    got = _procrustes(gpu, a, b, w, -1.0)[0].astype(np.float64)
    R = got[:, :3]
    _check('ortho', max(np.abs(R.T @ R - np.eye(3)).max(), abs(np.linalg.det(R) - 1.0)),
           f'collinear exact={exact}')
    opt = tr.weighted_residual(tr.kabsch(a[0], b[0], w[0], -1.0), a[0], b[0], w[0])
    res = tr.weighted_residual(got, a[0], b[0], w[0])
    print(f'MEASURE residual got {res:.9e} optimum {opt:.9e}')
    assert res <= opt * (1 + 1e-6) + 1e-10, (res, opt)


# ---------------------------------------------------------------------------------------------
# ModelNet metrics: fgr_modelnet_metrics
# ---------------------------------------------------------------------------------------------
METRIC_KEYS = ('r_mse', 'r_mae', 't_mse', 't_mae', 'err_r_deg', 'err_t', 'chamfer_dist')


@pytest.mark.parametrize('n_raw', [1, 2047, 2048, 2049])
@pytest.mark.parametrize('n_pts', [1, 255, 256, 257])
def test_modelnet_metrics(gpu, n_pts, n_raw):
    from scipy.spatial.transform import Rotation
    B = 3
    rng = np.random.default_rng(1000 * n_pts + n_raw)

    def euler_pose():                                   # |beta| <= 80 degrees: no gimbal lock
        e = rng.uniform((-180, -80, -180), (180, 80, 180))
        return np.concatenate([Rotation.from_euler('xyz', e, degrees=True).as_matrix(),
                               rng.uniform(-1, 1, (3, 1))], 1)

    gt = np.stack([euler_pose() for _ in range(B)]).astype(np.float32)
    pred = np.stack([euler_pose() for _ in range(B)]).astype(np.float32)
    pred[1] = gt[1]
    raw = rng.uniform(-1, 1, (B, n_raw, 3)).astype(np.float32)
    src = rng.uniform(-1, 1, (B, n_pts, 3)).astype(np.float32)
    ref = rng.uniform(-1, 1, (B, n_pts, 3)).astype(np.float32)
    need = _size('fgr_modelnet_metrics_workspace', B, n_pts)
    assert need == B * 2 * n_pts * 4

    def fn(ar):
        pd, gd = ar.put(_t(pred.reshape(B, 12)), name='pred'), ar.put(_t(gt.reshape(B, 12)), name='gt')
        sd, rd = ar.put(_t(src.reshape(-1, 3)), name='src'), ar.put(_t(ref.reshape(-1, 3)), name='ref')
        wd = ar.put(_t(raw.reshape(-1, 3)), name='raw')
        ws = ar.bytes(need, name='ws')
        out = ar.matrix(B, 7, 7, F64, 'out', 'metrics')
        _ok(_L().fgr_modelnet_metrics(_p(pd), _p(gd), _p(sd), _p(rd), _p(wd), B, n_pts, n_raw,
                                      _p(ws), need, _p(out), _st()), 'fgr_modelnet_metrics')
        return out

    out = _both(fn, gpu)
    got = {k: out[:, i] for i, k in enumerate(METRIC_KEYS)}
    want = mt.compute_metrics(src, ref, raw, gt, pred)
    check_modelnet_metrics(got, want, rel=1e-4)
    for k in METRIC_KEYS:
        if k == 'err_r_deg':        # pred == gt: acos of the float32 trace, the reference's own
            _check('metrics_err_r_deg', np.abs(got[k] - want[k])[[0, 2]].max())    # floor
        else:
            _check('metrics_' + k, np.abs(got[k] - want[k]).max() / max(np.abs(want[k]).max(), 1e-30))
