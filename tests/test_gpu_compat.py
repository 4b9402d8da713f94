"""The spatial-compatibility kernels (csrc/compat.hip: fgr_compat_pose) against the numpy
restatement tests/_compat_ref.py (pinned on the CPU by tests/test_compat_ref.py), through the C
ABI with every operand carved out of a guarded arena (tests/_arena.py) -- each call runs on a
clean and on a poisoned arena with bit-identical results and the workspace is exactly
fgr_compat_workspace bytes -- and through fgreg.compat.

Discrete results are compared exactly: n_eligible, row_score and seed_row against the
restatement (integers of the same correctly rounded fp32 comparisons), which seeds are valid,
every seed_count recomputed in numpy from the device's own seed_pose, best_seed as the first
maximum of the device's counts, and -- on inputs whose every scored pose keeps all rows at least
1e-3 r2 away from the radius, asserted first -- n_updates, n_inliers and the mask of the refit
loop restarted in numpy from the device's winning seed. Values are compared at BOUNDS: the worst
error measured on the MI355X against the fp64 restatement, times <= 4, never looser than the
family ceiling 1e-4 of test_gpu_tail_kernels.py. The pose error is test_gpu_icp.py's: |dR|
absolute and |dt| / max(1, max|t|).

  family                                            measured   asserted   ceiling
  pose   seed solves over <= k members (the worst:
         a planted 600-row input), refits, the
         whole call                                 1.78e-15   7.1e-15    1e-4
  rmse   fp64 sqrt(sum d2 / n) stored as fp32       4.16e-10   1.6e-09    1e-4

Both are the fp32 rounding of an fp64 result: the device sums the members' moments in another
order than numpy's centred product and runs a Jacobi SVD where numpy calls LAPACK, and the two
fp64 results round to the same fp32 pose: of the 51 comparisons measured, every seed solve and
every final pose is bit-equal to the restatement's but one element near zero of the
duplicate-rows input (1.78e-15). The rmse values are near 0.01, where half an ulp is 4.7e-10.

The pose bound therefore amounts to bit-equality of fp32 poses (one ulp of a rotation element is
6e-8). That is expected to hold, not luck: both sides compute the same rotation in fp64 to about
1e-15 and round it once to fp32, so they differ only where the fp64 value lies within 1e-15
(relative) of a midpoint between two fp32 numbers, one element in 10^8; the rule above sets the
bound, and a LAPACK that computed the 3 x 3 SVD to less than fp64 accuracy would break it while
the kernel is right.
"""
import functools

import numpy as np
import pytest
import torch

import _compat_ref as cr
import _ransac_ref as rr
from _arena import SENTINEL, Arena, assert_both_equal, bit_equal, run_both
from test_compat_ref import (D2_MARGIN, PROTO_DIST, PROTO_K, PROTO_SEEDS, SHAPE_DIST, SHAPE_K,
                             SHAPE_M, SHAPE_SEEDS, bad_arguments, proto_problem, shape_problem)
from test_gpu_icp import _pose_err, _relmax

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32

BOUNDS = {'pose': 7.1e-15, 'rmse': 1.6e-9}


def _check(family, err, what=''):
    """Prints the figure (the measurement), then asserts it."""
    err = float(err)
    print(f'MEASURE {family} {err:.3e} bound {BOUNDS[family]:.1e} {what}')
    assert err <= BOUNDS[family], (family, what, err, BOUNDS[family])


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


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _need(n_tot, B, max_len, n_seeds):
    from fgreg import _lib
    nb = _lib._sz(0)
    _ok(_L().fgr_compat_workspace(n_tot, B, max_len, n_seeds, nb), 'fgr_compat_workspace')
    return nb.value


KEYS = ('pose', 'n_inliers', 'rmse', 'n_eligible', 'best_seed', 'n_updates', 'mask', 'row_score',
        'seed_row', 'seed_pose', 'seed_count')


def _call(gpu, As, Bs, Ws, cdist, r, n_seeds, k, n_refits=4, w_min=0.0, max_len=None):
    """fgr_compat_pose with every output, on a clean and a poisoned arena -> dict of numpy
    arrays: pose (B, 3, 4), n_inliers, rmse, n_eligible, best_seed, n_updates, mask (n_tot,)
    uint8, row_score (n_tot,), seed_row (B, n_seeds), seed_pose (B, n_seeds, 3, 4), seed_count
    (B, n_seeds)."""
    lens = [len(x) for x in As]
    B, n_tot = len(As), sum(lens)
    max_len = max(lens) if max_len is None else max_len
    a = np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in As])
    b = np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in Bs])
    w = None if Ws is None else np.concatenate([np.asarray(x, np.float32) for x in Ws])
    off = rr.offsets(lens)
    need = _need(n_tot, B, max_len, n_seeds)

    def fn(ar):
        da = ar.put(_t(a), name='a') if n_tot else None
        db = ar.put(_t(b), name='b') if n_tot else None
        dw = ar.put(_t(w), name='w') if (w is not None and n_tot) else None
        do = ar.put(_t(off), name='off')
        ws = ar.bytes(need, name='ws')
        pose = ar.matrix(B, 12, 12, F32, 'out', 'pose')
        ni, ne, bs, nu = (ar.vector(B, I32, 'out', name) for name in
                          ('n_inliers', 'n_eligible', 'best_seed', 'n_updates'))
        rmse = ar.vector(B, F32, 'out', 'rmse')
        # uint8, so not an 'out' region (those are checked in 32-bit words): an exact n_tot-byte
        # view between sentinel guards, prefilled 0x00 / 0xFF; it must hold 0 / 1 afterwards
        mask = ar.bytes(max(n_tot, 1), name='mask')
        score = ar.vector(max(n_tot, 1), I32, 'out', 'row_score', full=n_tot > 0)
        srow = ar.matrix(B, n_seeds, n_seeds, I32, 'out', 'seed_row')
        sp = ar.matrix(B * n_seeds, 12, 12, F32, 'out', 'seed_pose')
        sc = ar.matrix(B, n_seeds, n_seeds, I32, 'out', 'seed_count')
        _ok(_L().fgr_compat_pose(_p(da), _p(db), _p(dw), n_tot, _p(do), B, max_len, w_min, cdist, r,
                                 n_seeds, k, n_refits, _p(ws), need, _p(pose), _p(ni), _p(rmse),
                                 _p(ne), _p(bs), _p(nu), _p(mask) if n_tot else None,
                                 _p(score) if n_tot else None, _p(srow), _p(sp), _p(sc), _st()),
            'fgr_compat_pose')
        return pose, ni, rmse, ne, bs, nu, mask[:n_tot], score[:n_tot], srow, sp, sc

    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    out = dict(zip(KEYS, (t.cpu().numpy() for t in clean)))
    out['pose'] = out['pose'].reshape(B, 3, 4)
    out['seed_pose'] = out['seed_pose'].reshape(B, n_seeds, 3, 4)
    assert set(np.unique(out['mask']).tolist()) <= {0, 1}      # every byte written, also the poisoned
    out['off'] = off
    return out


def _assert_pair(out, p, a, b, w, cdist, r, n_seeds, k, n_refits=4, w_min=0.0, what=''):
    """Pair p of a call against the restatement -> the restatement's dict."""
    a, b = np.asarray(a, np.float32).reshape(-1, 3), np.asarray(b, np.float32).reshape(-1, 3)
    lo, hi = out['off'][p], out['off'][p + 1]
    ref = cr.compat(a, b, w, cdist, r, n_seeds, k, 0, w_min)
    el = rr.eligible(w, w_min, len(a))
    ae, be = a[el], b[el]
    assert out['n_eligible'][p] == ref['n_eligible'] == len(ae), what
    assert np.array_equal(out['row_score'][lo:hi], ref['row_score']), \
        (what, np.flatnonzero(out['row_score'][lo:hi] != ref['row_score'])[:5])
    assert np.array_equal(out['seed_row'][p], ref['seed_row']), (what, out['seed_row'][p], ref['seed_row'])
    sp, sc = out['seed_pose'][p], out['seed_count'][p]
    ok = np.array([mem is not None for mem in ref['members']])
    assert np.array_equal(sc >= 0, ok), (what, sc, ok)
    assert (sc[~ok] == -1).all() and np.array_equal(sp[~ok], np.tile(rr.EYE, (int((~ok).sum()), 1, 1)))
    worst = 0.0
    for q in np.flatnonzero(ok):
        assert sc[q] == rr.count(sp[q], ae, be, r), (what, q)
        R = sp[q][:, :3].astype(np.float64)
        assert np.isfinite(sp[q]).all() and abs(np.linalg.det(R) - 1) < 1e-5
        mem = ref['members'][q]
        ma, mb = ae[mem].astype(np.float64), be[mem].astype(np.float64)
        sv = np.linalg.svd((ma - ma.mean(0)).T @ (mb - mb.mean(0)), compute_uv=False)
        if sv[1] > 1e-6 * sv[0]:          # a rank <= 1 covariance has many optimal rotations
            worst = max(worst, _pose_err(sp[q], ref['seed_pose'][q]))
    if ok.any():
        _check('pose', worst, f'{what} seed solves')
    best = int(out['best_seed'][p])
    assert best == rr.select(sc), (what, best, rr.select(sc))
    mask = out['mask'][lo:hi].astype(bool)
    if best < 0:
        assert np.array_equal(out['pose'][p], rr.EYE) and out['n_inliers'][p] == 0
        assert out['rmse'][p] == 0 and out['n_updates'][p] == 0 and not mask.any()
        return ref
    fit = rr.refit(ae, be, sp[best], int(sc[best]), r, n_refits)
    assert min(fit['gaps']) >= D2_MARGIN, (what, fit['gaps'])      # the precondition, not a skip
    want = np.zeros(len(a), bool)
    want[np.flatnonzero(el)[fit['inl']]] = True
    assert out['n_updates'][p] == fit['n_updates'], (what, out['n_updates'][p], fit['n_updates'])
    assert out['n_inliers'][p] == fit['n_inliers'], (what, out['n_inliers'][p], fit['n_inliers'])
    assert np.array_equal(mask, want), (what, np.flatnonzero(mask != want)[:5])
    _check('pose', _pose_err(out['pose'][p], fit['pose']), f'{what} final pose')
    _check('rmse', _relmax(out['rmse'][p:p + 1], [fit['rmse']]), f'{what} rmse')
    assert out['n_inliers'][p] == mask.sum() and not mask[~el].any()
    return ref


# ---------------------------------------------------------------------------------------------
# shapes: word tails, several tiles in both directions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', SHAPE_M)
def test_shapes(gpu, m):
    a, b = shape_problem(m)
    out = _call(gpu, [a], [b], None, SHAPE_DIST, SHAPE_DIST, SHAPE_SEEDS, SHAPE_K)
    ref = _assert_pair(out, 0, a, b, None, SHAPE_DIST, SHAPE_DIST, SHAPE_SEEDS, SHAPE_K, what=f'm {m}')
    if m >= 63:
        assert out['best_seed'][0] >= 0 and out['n_inliers'][0] > 0.3 * m
        assert len(set(ref['row_score'].tolist())) > 10
    if m < SHAPE_SEEDS:                                         # n_seeds > m: unused positions
        assert (out['seed_row'][0][m:] == -1).all() and (out['seed_count'][0][m:] == -1).all()


def _mixed():
    lens = (300, 0, 65, 17)
    As, Bs = [], []
    for n, m in enumerate(lens):
        a, b, _, _ = cr.planted_unit(70 + n, m, 0.5, 0.005, SHAPE_DIST) if m else \
            (np.zeros((0, 3), np.float32),) * 2 + (None, None)
        As.append(a)
        Bs.append(b)
    rng = np.random.default_rng(71)
    Ws = [rng.uniform(0.3, 1.0, m).astype(np.float32) for m in lens]
    Ws[0][rng.permutation(300)[:60]] = np.float32(0.25)       # exactly w_min: not eligible
    Ws[0][5] = np.nan
    Ws[2][64] = np.float32(0.1)
    return As, Bs, Ws


def test_mixed_batch_with_weights(gpu):
    As, Bs, Ws = _mixed()
    out = _call(gpu, As, Bs, Ws, SHAPE_DIST, SHAPE_DIST, 24, SHAPE_K, w_min=0.25)
    assert out['n_eligible'].tolist() == [int(rr.eligible(w, 0.25, len(w)).sum()) for w in Ws]
    assert out['n_eligible'][0] < 245 and out['n_eligible'].tolist()[1:] == [0, 64, 17]
    for p in range(4):
        _assert_pair(out, p, As[p], Bs[p], Ws[p], SHAPE_DIST, SHAPE_DIST, 24, SHAPE_K, w_min=0.25,
                     what=f'mixed pair {p}')
    assert out['best_seed'][1] == -1 and out['best_seed'][0] >= 0 and out['best_seed'][2] >= 0
    assert (out['row_score'][:300][~rr.eligible(Ws[0], 0.25, 300)] == -1).all()
    # the same rows without weights, and max_len above the true maximum: the same results
    plain = _call(gpu, As, Bs, None, SHAPE_DIST, SHAPE_DIST, 24, SHAPE_K)
    roomy = _call(gpu, As, Bs, None, SHAPE_DIST, SHAPE_DIST, 24, SHAPE_K, max_len=1000)
    assert plain['n_eligible'].tolist() == [300, 0, 65, 17]
    for p in range(4):
        _assert_pair(plain, p, As[p], Bs[p], None, SHAPE_DIST, SHAPE_DIST, 24, SHAPE_K, what=f'mixed, w NULL, pair {p}')
    for key in KEYS:
        assert bit_equal(_t(plain[key]), _t(roomy[key])), key


def test_max_len_below_a_pairs_rows(gpu):
    """max_len bounds the eligible rows of a pair. A pair above it gets no seed (best_seed -1,
    identity, row_score -1) and nothing outside the workspace sized for max_len is touched (the
    arena's guards); the other pairs are unaffected. A pair whose ROWS exceed max_len but whose
    eligible rows do not is served as usual."""
    As, Bs, Ws = _mixed()
    plain = _call(gpu, As, Bs, None, SHAPE_DIST, SHAPE_DIST, 24, SHAPE_K)
    tight = _call(gpu, As, Bs, None, SHAPE_DIST, SHAPE_DIST, 24, SHAPE_K, max_len=100)
    assert tight['n_eligible'].tolist() == [300, 0, 65, 17]
    assert tight['best_seed'][0] == -1 and np.array_equal(tight['pose'][0], rr.EYE)
    assert tight['n_inliers'][0] == 0 and tight['rmse'][0] == 0 and tight['n_updates'][0] == 0
    assert (tight['row_score'][:300] == -1).all() and not tight['mask'][:300].any()
    assert (tight['seed_row'][0] == -1).all() and (tight['seed_count'][0] == -1).all()
    assert np.array_equal(tight['seed_pose'][0], np.tile(rr.EYE, (24, 1, 1)))
    for key in ('pose', 'n_inliers', 'rmse', 'best_seed', 'n_updates', 'seed_row', 'seed_pose', 'seed_count'):
        assert bit_equal(_t(tight[key][1:]), _t(plain[key][1:])), key
    for key in ('mask', 'row_score'):
        assert bit_equal(_t(tight[key][300:]), _t(plain[key][300:])), key
    # 300 rows, fewer than 245 of them eligible: max_len 245 serves the pair
    full = _call(gpu, As, Bs, Ws, SHAPE_DIST, SHAPE_DIST, 24, SHAPE_K, w_min=0.25)
    fits = _call(gpu, As, Bs, Ws, SHAPE_DIST, SHAPE_DIST, 24, SHAPE_K, w_min=0.25, max_len=245)
    assert full['best_seed'][0] >= 0 and full['n_eligible'][0] <= 245
    for key in KEYS:
        assert bit_equal(_t(full[key]), _t(fits[key])), key


def test_k_larger_than_any_neighbourhood(gpu):
    a, b = shape_problem(65)
    out = _call(gpu, [a], [b], None, SHAPE_DIST, SHAPE_DIST, 65, 256)
    ref = _assert_pair(out, 0, a, b, None, SHAPE_DIST, SHAPE_DIST, 65, 256, what='k 256')
    sizes = [len(mem) for mem in ref['members'] if mem is not None]
    assert sizes and max(sizes) < 65 and len(set(sizes)) > 1       # whole neighbourhoods


def test_no_compatible_rows(gpu):
    a = np.random.default_rng(8).uniform(0, 1, (100, 3)).astype(np.float32)
    b = 3 * a
    b[:2] = a[:2]                                                  # one compatible partner: 2 members
    out = _call(gpu, [a], [b], None, 1e-4, 0.05, 16, 8)
    _assert_pair(out, 0, a, b, None, 1e-4, 0.05, 16, 8, what='no compatible rows')
    assert out['best_seed'][0] == -1 and (out['seed_count'][0] == -1).all()
    assert (out['row_score'] == 0).all() and out['seed_row'][0].tolist() == list(range(16))


def test_duplicate_rows_tie_everywhere(gpu):
    base = np.random.default_rng(3).uniform(0, 1, (5, 3)).astype(np.float32)
    a = np.tile(base, (14, 1))                                     # 70 rows: two words
    b = a + np.float32(0.25)
    out = _call(gpu, [a], [b], None, 0.01, 0.01, 9, 4, n_refits=0)
    _assert_pair(out, 0, a, b, None, 0.01, 0.01, 9, 4, n_refits=0, what='duplicates')
    assert len(set(out['row_score'].tolist())) == 1 and out['row_score'][0] == 69 * 68
    assert out['seed_row'][0].tolist() == list(range(9)) and out['best_seed'][0] == 0
    assert (out['seed_count'][0] == 70).all() and out['n_inliers'][0] == 70


@pytest.mark.parametrize('pct,n', [(3, 0), (3, 1), (5, 0), (5, 1)])
def test_planted_inputs(gpu, pct, n):
    a, b, truth, planted = proto_problem(pct, n)
    out = _call(gpu, [a], [b], None, PROTO_DIST, PROTO_DIST, PROTO_SEEDS, PROTO_K)
    _assert_pair(out, 0, a, b, None, PROTO_DIST, PROTO_DIST, PROTO_SEEDS, PROTO_K, what=f'planted {pct} % {n}')
    mask = out['mask'].astype(bool)
    rot, tr = cr.pose_errors(out['pose'][0], truth)
    print(f'planted {pct} % input {n}: best {out["best_seed"][0]} n_updates {out["n_updates"][0]} '
          f'n_inliers {out["n_inliers"][0]} rot {rot:.3f} deg trans {tr:.4f}')
    assert mask[planted].all() and rot < 1.0 and tr < 0.02


# ---------------------------------------------------------------------------------------------
# refusals, determinism
# ---------------------------------------------------------------------------------------------
def test_refused_arguments_write_nothing(gpu):
    """Every refused argument with live device operands: FGR_E_ARG, every output still the
    sentinel, the workspace untouched."""
    a, b = shape_problem(63)
    As, Bs = [a[:40], a[40:]], [b[:40], b[40:]]
    n_tot = 63
    need = _need(n_tot, 2, 60, 16)
    ar = Arena(gpu)
    da, db = ar.put(_t(np.concatenate(As)), name='a'), ar.put(_t(np.concatenate(Bs)), name='b')
    do = ar.put(_t(rr.offsets([40, 23])), name='off')
    ws = ar.bytes(need, name='ws')
    outs = [ar.matrix(2, 12, 12, F32, 'out', 'pose', full=False)] + \
           [ar.vector(2, I32, 'out', f'o{i}', full=False) for i in range(5)]
    extra = [ar.vector(n_tot, I32, 'out', 'row_score', full=False),
             ar.matrix(2, 16, 16, I32, 'out', 'seed_row', full=False),
             ar.matrix(32, 12, 12, F32, 'out', 'seed_pose', full=False),
             ar.matrix(2, 16, 16, I32, 'out', 'seed_count', full=False)]
    good, cases = bad_arguments(need, 0)
    good.update(a=_p(da), b=_p(db), off=_p(do), ws=_p(ws), n_tot=n_tot, pose=_p(outs[0]),
                n_inliers=_p(outs[1]), inlier_rmse=_p(outs[2]), n_eligible=_p(outs[3]),
                best_seed=_p(outs[4]), n_updates=_p(outs[5]), row_score=_p(extra[0]),
                seed_row=_p(extra[1]), seed_pose=_p(extra[2]), seed_count=_p(extra[3]),
                stream=_st())
    for case in cases:
        if 'ws' in case and case['ws'] is not None:
            case = {'ws': _p(ws) + 8}                              # misaligned
        rc = _L().fgr_compat_pose(*{**good, **case}.values())
        assert rc == -1 and b'fgr_compat_pose' in _L().fgr_last_error(), (case, rc)
    rc = _L().fgr_compat_pose(*{**good, 'ws_bytes': need - 16}.values())
    assert rc == -1 and b'fgr_compat_pose: workspace' in _L().fgr_last_error()
    torch.cuda.synchronize()
    ar.check()
    for o in outs + extra:
        assert bool((o.contiguous().view(torch.int32) == SENTINEL).all())
    assert not bool(ws.any())


def test_two_calls_give_the_same_bits(gpu):
    As, Bs, Ws = _mixed()
    one = _call(gpu, As, Bs, Ws, SHAPE_DIST, SHAPE_DIST, 24, SHAPE_K, w_min=0.25)
    two = _call(gpu, As, Bs, Ws, SHAPE_DIST, SHAPE_DIST, 24, SHAPE_K, w_min=0.25)
    for key in KEYS:
        assert bit_equal(_t(one[key]), _t(two[key])), key


# ---------------------------------------------------------------------------------------------
# fgreg.robust, fgreg.match
# ---------------------------------------------------------------------------------------------
def _dev(xs, gpu):
    return [_t(x).to(gpu) for x in xs]


def test_python_api_matches_the_abi(gpu):
    import fgreg
    As, Bs, Ws = _mixed()
    out = fgreg.compat(_dev(As, gpu), _dev(Bs, gpu), _dev(Ws, gpu), compat_dist=SHAPE_DIST,
                       inlier_dist=SHAPE_DIST, n_seeds=24, k=SHAPE_K, w_min=0.25, mask=True,
                       seeds=True, scores=True)
    ref = _call(gpu, As, Bs, Ws, SHAPE_DIST, SHAPE_DIST, 24, SHAPE_K, w_min=0.25)
    assert set(out) == {'pose', 'n_inliers', 'n_eligible', 'inlier_rmse', 'best_seed', 'n_updates',
                        'mask', 'seed_row', 'seed_pose', 'seed_count', 'row_score'}
    for key, rk in (('pose', 'pose'), ('n_inliers', 'n_inliers'), ('n_eligible', 'n_eligible'),
                    ('inlier_rmse', 'rmse'), ('best_seed', 'best_seed'), ('n_updates', 'n_updates'),
                    ('seed_row', 'seed_row'), ('seed_pose', 'seed_pose'), ('seed_count', 'seed_count')):
        assert bit_equal(out[key].cpu(), _t(ref[rk])), key
    assert [len(x) for x in out['mask']] == [300, 0, 65, 17] and out['mask'][0].dtype == torch.bool
    assert np.array_equal(torch.cat(out['mask']).cpu().numpy(), ref['mask'].astype(bool))
    assert [len(x) for x in out['row_score']] == [300, 0, 65, 17]
    assert np.array_equal(torch.cat(out['row_score']).cpu().numpy(), ref['row_score'])
    plain = fgreg.compat(_dev(As, gpu)[0], _dev(Bs, gpu)[0], compat_dist=SHAPE_DIST, inlier_dist=SHAPE_DIST)
    assert set(plain) == {'pose', 'n_inliers', 'n_eligible', 'inlier_rmse', 'best_seed', 'n_updates'}
    assert tuple(plain['pose'].shape) == (1, 3, 4) and int(plain['n_eligible'][0]) == 300
    with pytest.raises(fgreg.FgrError):
        fgreg.compat([_t(x) for x in As], [_t(x) for x in Bs], compat_dist=0.1, inlier_dist=0.1)
    with pytest.raises(fgreg.FgrError):
        fgreg.compat(_dev(As, gpu), _dev(Bs, gpu), compat_dist=-1.0, inlier_dist=0.1)
    with pytest.raises(fgreg.FgrError):
        fgreg.compat(_dev(As, gpu), _dev(Bs, gpu), compat_dist=0.1, inlier_dist=0.1, k=2)


def test_graph_capture(gpu):
    """fgreg.compat in one torch.cuda.graph on one stream, replayed with refreshed inputs: the
    eager call's bits."""
    import fgreg
    probs = [proto_problem(5, n)[:2] for n in (0, 1)]
    sa, sb = torch.empty(600, 3, device=gpu), torch.empty(600, 3, device=gpu)
    sw = torch.ones(600, device=gpu)
    call = lambda: fgreg.compat(sa, sb, sw, compat_dist=PROTO_DIST, inlier_dist=PROTO_DIST,
                                n_seeds=PROTO_SEEDS, k=PROTO_K, w_min=0.5, mask=True, seeds=True,
                                scores=True)
    flat = lambda o: [o[key] for key in ('pose', 'n_inliers', 'n_eligible', 'inlier_rmse',
                                         'best_seed', 'n_updates', 'seed_row', 'seed_pose',
                                         'seed_count')] + list(o['mask']) + list(o['row_score'])
    eager = []
    for a, b in probs:
        sa.copy_(_t(a))
        sb.copy_(_t(b))
        eager.append([t.clone() for t in flat(call())])
    torch.cuda.synchronize()
    assert not bit_equal(eager[0][0], eager[1][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = flat(call())
    for which in (1, 0):
        sa.copy_(_t(probs[which][0]))
        sb.copy_(_t(probs[which][1]))
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(eager[which], cap):
            assert bit_equal(x, y)


@functools.lru_cache(maxsize=None)
def _forward(gpu):
    from test_gpu_match import _forward as forward
    return forward(gpu)


def test_compat_outputs_assembles_the_pose_stage_rows(gpu):
    import fgreg
    _, out = _forward(gpu)
    got = fgreg.compat_outputs(out, 0.1, 0.2, n_seeds=16, mask=True, seeds=True)
    a, b, w = fgreg.robust.correspondences(out)
    hand = fgreg.compat(a, b, w, compat_dist=0.1, inlier_dist=0.2, n_seeds=16, mask=True, seeds=True)
    assert set(got) == set(hand)
    for key in hand:
        xs, ys = (got[key], hand[key]) if isinstance(hand[key], list) else ([got[key]], [hand[key]])
        assert all(bit_equal(x, y) for x, y in zip(xs, ys)), key
    assert tuple(got['pose'].shape) == (len(a), 3, 4) and tuple(got['seed_row'].shape) == (len(a), 16)
    other = fgreg.compat_outputs(out, 0.1, 0.2, layer=0, n_seeds=16)
    assert not bit_equal(other['pose'], got['pose'])


def test_register_features_estimators(gpu):
    """estimator='compat' is fgreg.compat on match_outputs' rows; estimator='ransac' is the call
    without the keyword, bit for bit; anything else is refused."""
    import fgreg
    model, out = _forward(gpu)
    reg = fgreg.register_features(out, 0.1, model=model, estimator='compat', compat_dist=0.05,
                                  n_seeds=32, k=8, n_hyp=7, seed=99, mask=True)
    m = fgreg.match_outputs(out, model=model)
    hand = fgreg.compat(m['a'], m['b'], m['w'], compat_dist=0.05, inlier_dist=0.1, n_seeds=32, k=8,
                        mask=True)
    assert set(reg) == set(hand) | {'matches'} and 'best_seed' in reg and 'best_hyp' not in reg
    for key in hand:
        xs, ys = (reg[key], hand[key]) if isinstance(hand[key], list) else ([reg[key]], [hand[key]])
        assert all(bit_equal(x, y) for x, y in zip(xs, ys)), key
    assert np.array_equal(reg['n_eligible'].cpu().numpy(), m['n_matches'].cpu().numpy())
    # compat_dist defaults to inlier_dist
    dflt = fgreg.register_features(out, 0.1, model=model, estimator='compat')
    hand = fgreg.compat(m['a'], m['b'], m['w'], compat_dist=0.1, inlier_dist=0.1)
    for key in hand:
        assert bit_equal(dflt[key], hand[key]), key
    named = fgreg.register_features(out, 0.1, model=model, n_hyp=256, seed=3, estimator='ransac')
    plain = fgreg.register_features(out, 0.1, model=model, n_hyp=256, seed=3)
    assert set(named) == set(plain) and 'best_hyp' in named
    for key in plain:
        if key != 'matches':
            assert bit_equal(named[key], plain[key]), key
    with pytest.raises(fgreg.FgrError):
        fgreg.register_features(out, 0.1, model=model, estimator='teaser')
