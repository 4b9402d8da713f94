"""The RANSAC kernels (csrc/ransac.hip: fgr_ransac_pose) against the numpy restatement
tests/_ransac_ref.py (pinned on the CPU by tests/test_ransac_ref.py), through the C ABI with
every operand carved out of a guarded arena (tests/_arena.py) -- each call runs on a clean and on
a poisoned arena with bit-identical results and the workspace is exactly fgr_ransac_workspace
bytes -- and through fgreg.robust.

Discrete results are compared exactly: where the ranks repeat, every hypothesis's count (the
same fp32 operations in the same order on both sides, from the device's own pose), the
selection, n_eligible, and -- on inputs whose every scored pose keeps all rows at least
1e-3 r2 away from the radius, asserted first -- n_updates, n_inliers and the mask of the refit
loop restarted in numpy from the device's winning hypothesis. Values are compared at BOUNDS:
the worst error measured on the MI355X against the fp64 restatement, times <= 4, never looser
than the family ceiling 1e-4 of test_gpu_tail_kernels.py. The pose error is test_gpu_icp.py's:
|dR| absolute and |dt| / max(1, max|t|).

  family                                            measured   asserted   ceiling
  pose   3-point solves (the worst: m 529, n_hyp
         1000), refits, the whole call              5.78e-08   2.3e-07    1e-4
  rmse   fp64 sqrt(sum d2 / n) stored as fp32       6.95e-10   2.7e-09    1e-4

Both are the fp32 rounding of an fp64 result (the rmse values are near 0.03, where half an ulp
is 9e-10). Every final pose measured -- the six loop seeds, the mixed batch, the mirrored pair
-- is bit-equal to the restatement's; against fgr_procrustes on the fixture's rows as well.
"""
import functools

import numpy as np
import pytest
import torch

import _ransac_ref as rr
from _arena import assert_both_equal, bit_equal, run_both
from test_gpu_icp import _pose_err, _relmax
from test_ransac_ref import LOOP_HYP, LOOP_R, LOOP_REFITS, LOOP_SEEDS, loop_problem

pytestmark = pytest.mark.gpu
F32, I32, I64 = torch.float32, torch.int32, torch.int64
TILE = 256                                  # kRsTile of csrc/ransac.hip

BOUNDS = {'pose': 2.3e-7, 'rmse': 2.7e-9}


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


def _need(n_tot, B, n_hyp):
    from fgreg import _lib
    nb = _lib._sz(0)
    _ok(_L().fgr_ransac_workspace(n_tot, B, n_hyp, nb), 'fgr_ransac_workspace')
    return nb.value


KEYS = ('pose', 'n_inliers', 'rmse', 'n_eligible', 'best_hyp', 'n_updates', 'mask', 'hyp_pose',
        'hyp_count')


def _call(gpu, As, Bs, Ws, r, n_hyp, seed=0, n_refits=4, w_min=0.0):
    """fgr_ransac_pose with every output, on a clean and a poisoned arena -> dict of numpy
    arrays: pose (B, 3, 4), n_inliers, rmse, n_eligible, best_hyp, n_updates, mask (n_tot,)
    uint8, hyp_pose (B, n_hyp, 3, 4), hyp_count (B, n_hyp)."""
    lens = [len(x) for x in As]
    B, n_tot = len(As), sum(lens)
    a = np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in As])
    b = np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in Bs])
    w = None if Ws is None else np.concatenate([np.asarray(x, np.float32) for x in Ws])
    off = rr.offsets(lens)
    need = _need(n_tot, B, n_hyp)

    def fn(ar):
        da = ar.put(_t(a), name='a') if n_tot else None
        db = ar.put(_t(b), name='b') if n_tot else None
        dw = ar.put(_t(w), name='w') if (w is not None and n_tot) else None
        do = ar.put(_t(off), name='off')
        ws = ar.bytes(need, name='ws')
        pose = ar.matrix(B, 12, 12, F32, 'out', 'pose')
        ni, ne, bh, nu = (ar.vector(B, I32, 'out', k) for k in
                          ('n_inliers', 'n_eligible', 'best_hyp', 'n_updates'))
        rmse = ar.vector(B, F32, 'out', 'rmse')
        # uint8, so not an 'out' region (those are checked in 32-bit words): an exact n_tot-byte
        # view between sentinel guards, prefilled 0x00 / 0xFF; it must hold 0 / 1 afterwards
        mask = ar.bytes(max(n_tot, 1), name='mask')
        hp = ar.matrix(B * n_hyp, 12, 12, F32, 'out', 'hyp_pose')
        hc = ar.matrix(B, n_hyp, n_hyp, I32, 'out', 'hyp_count')
        _ok(_L().fgr_ransac_pose(_p(da), _p(db), _p(dw), n_tot, _p(do), B, w_min, r, n_hyp, seed,
                                 n_refits, _p(ws), need, _p(pose), _p(ni), _p(rmse), _p(ne),
                                 _p(bh), _p(nu), _p(mask) if n_tot else None, _p(hp), _p(hc),
                                 _st()), 'fgr_ransac_pose')
        return pose, ni, rmse, ne, bh, nu, mask[:n_tot], hp, hc

    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    out = dict(zip(KEYS, (t.cpu().numpy() for t in clean)))
    out['pose'] = out['pose'].reshape(B, 3, 4)
    out['hyp_pose'] = out['hyp_pose'].reshape(B, n_hyp, 3, 4)
    assert set(np.unique(out['mask']).tolist()) <= {0, 1}      # every byte written, also the poisoned
    out['off'] = off
    return out


def _eligible_rows(a, b, w, w_min):
    el = rr.eligible(w, w_min, len(a))
    return np.asarray(a, np.float32)[el], np.asarray(b, np.float32)[el], el


def _assert_hypotheses(out, p, a, b, w, r, n_hyp, seed, w_min=0.0, what=''):
    """Pair p of a call: validity where the restated ranks repeat, every valid pose against the
    fp64 Kabsch of the restated sample, every count exactly from the device's own pose, and the
    first-maximum selection of the device's own counts."""
    ae, be, el = _eligible_rows(a, b, w, w_min)
    m = len(ae)
    assert out['n_eligible'][p] == m
    rk = rr.ranks(seed, p, n_hyp, m) if m else np.zeros((n_hyp, 3), np.int64)
    ok = rr.valid_ranks(rk, m) & (m >= 3)
    hp, hc = out['hyp_pose'][p], out['hyp_count'][p]
    assert np.array_equal(hc == -1, ~ok), (what, np.flatnonzero((hc == -1) != ~ok)[:5])
    assert np.array_equal(hp[~ok], np.tile(rr.EYE, (int((~ok).sum()), 1, 1)))
    if ok.any():
        want = rr.sample_poses(ae, be, rk, ok)[ok]
        # a sample whose covariance has rank <= 1 (collinear or repeated points) has many optimal
        # rotations (include/fgreg.h): only a proper rotation can be asked of it
        sa, sb = ae[rk[ok]].astype(np.float64), be[rk[ok]].astype(np.float64)
        sv = np.linalg.svd(np.swapaxes(sa - sa.mean(1, keepdims=True), 1, 2) @ (sb - sb.mean(1, keepdims=True)),
                           compute_uv=False)
        unique = sv[:, 1] > 1e-6 * sv[:, 0]
        if unique.any():
            _check('pose', max(_pose_err(g, t) for g, t in zip(hp[ok][unique], want[unique])),
                   f'{what} 3-point solves')
        R = hp[ok][:, :, :3].astype(np.float64)
        assert np.isfinite(hp[ok]).all() and np.abs(np.linalg.det(R) - 1).max() < 1e-5
        assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() < 1e-5
    for h in np.flatnonzero(ok):
        assert hc[h] == rr.count(hp[h], ae, be, r), (what, h)
    assert out['best_hyp'][p] == rr.select(hc), (what, out['best_hyp'][p], rr.select(hc))
    return ae, be, el, ok, (unique if ok.any() else np.zeros(0, bool))


def _assert_final(out, p, a, b, w, r, n_refits, w_min=0.0, what='', exact=True):
    """Pair p's outputs against the restatement's refit loop started from the device's winner.
    exact: the gap precondition holds (asserted), so the discrete results must be equal."""
    best = int(out['best_hyp'][p])
    lo, hi = out['off'][p], out['off'][p + 1]
    mask = out['mask'][lo:hi].astype(bool)
    start = (best, out['hyp_pose'][p, best], int(out['hyp_count'][p, best])) if best >= 0 else (-1, rr.EYE, 0)
    ref = rr.ransac(a, b, w, r, out['hyp_count'].shape[1], n_refits=n_refits, w_min=w_min, pair=p,
                    start=start)
    if best < 0:
        assert np.array_equal(out['pose'][p], rr.EYE) and out['n_inliers'][p] == 0
        assert out['rmse'][p] == 0 and out['n_updates'][p] == 0 and not mask.any()
        return ref
    if exact:
        assert min(ref['gaps']) >= 1e-3, (what, ref['gaps'])       # the precondition, not a skip
        assert out['n_updates'][p] == ref['n_updates'], (what, out['n_updates'][p], ref['n_updates'])
        assert out['n_inliers'][p] == ref['n_inliers'], (what, out['n_inliers'][p], ref['n_inliers'])
        assert np.array_equal(mask, ref['mask']), (what, np.flatnonzero(mask != ref['mask'])[:5])
        _check('pose', _pose_err(out['pose'][p], ref['pose']), f'{what} final pose')
        _check('rmse', _relmax(out['rmse'][p:p + 1], [ref['rmse']]), f'{what} rmse')
    assert out['n_inliers'][p] == mask.sum() and not mask[~rr.eligible(w, w_min, len(a))].any()
    return ref


# ---------------------------------------------------------------------------------------------
# 1-3: hypotheses, counts, selection
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shape_problem(m):
    r = 0.1
    a, b, _, _ = rr.planted_problem(100 + m, m, 0.5, 0.5 * r, r)
    return a, b, r


@pytest.mark.parametrize('m', [3, 4, TILE - 1, TILE, TILE + 1, 2 * TILE + 17])
def test_hypotheses_counts_and_selection(gpu, m):
    a, b, r = _shape_problem(m)
    for n_hyp in (1, 64, 255, 256, 257, 1000):
        out = _call(gpu, [a], [b], None, r, n_hyp, seed=m + n_hyp)
        _, _, _, ok, unique = _assert_hypotheses(out, 0, a, b, None, r, n_hyp, m + n_hyp,
                                                 what=f'm {m} n_hyp {n_hyp}')
        assert unique.all()
        if n_hyp >= 255:
            assert ok.any() and (m > 4 or (~ok).any())
        if m >= TILE - 1 and n_hyp == 1000:
            hc = out['hyp_count'][0]
            assert hc.max() > 0.3 * m and (hc[ok] < 10).any()      # good and bad hypotheses


def test_selection_tie_goes_to_the_lowest_hypothesis(gpu):
    """Duplicated correspondences and a radius that takes every row: every valid hypothesis
    counts m, so the winner is the first valid one (which is not hypothesis 0 here)."""
    rng = np.random.default_rng(3)
    base = rng.uniform(-1, 1, (5, 3))
    a = np.tile(base, (4, 1)).astype(np.float32)
    b = (a.astype(np.float64) @ rr.rotation([1, 1, 0], 15.0).T + 0.1).astype(np.float32)
    m, n_hyp = len(a), 600
    seed = next(s for s in range(100) if not rr.valid_ranks(rr.ranks(s, 0, n_hyp, m), m)[0])
    out = _call(gpu, [a], [b], None, 10.0, n_hyp, seed=seed, n_refits=0)
    _, _, _, ok, unique = _assert_hypotheses(out, 0, a, b, None, 10.0, n_hyp, seed, what='tie')
    assert unique.any() and not unique.all()              # samples of repeated points among them
    first = int(np.flatnonzero(ok)[0])
    assert first > 0 and (out['hyp_count'][0][ok] == m).all() and out['best_hyp'][0] == first
    # a tie across blocks: the first valid hypothesis of the second block loses to the first's
    assert ok[256:].any() and out['n_inliers'][0] == m


# ---------------------------------------------------------------------------------------------
# 4: the refit loop
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', LOOP_SEEDS)
def test_refit_loop(gpu, seed):
    a, b, planted = loop_problem(seed)
    out = _call(gpu, [a], [b], None, LOOP_R, LOOP_HYP, seed=seed, n_refits=LOOP_REFITS)
    _assert_hypotheses(out, 0, a, b, None, LOOP_R, LOOP_HYP, seed, what=f'loop seed {seed}')
    ref = _assert_final(out, 0, a, b, None, LOOP_R, LOOP_REFITS, what=f'loop seed {seed}')
    print(f'seed {seed}: best {out["best_hyp"][0]} n_updates {out["n_updates"][0]} '
          f'n_inliers {out["n_inliers"][0]} min gap {min(ref["gaps"]):.2e}')
    assert out['n_updates'][0] >= 2 and np.array_equal(out['mask'].astype(bool), planted)


# ---------------------------------------------------------------------------------------------
# 5: degenerate and mixed batches
# ---------------------------------------------------------------------------------------------
def _mixed():
    r = 0.05
    a, b, _, planted = rr.planted_problem(41, 700, 0.5, 0.3 * r, r)
    rng = np.random.default_rng(42)
    w = rng.uniform(0.3, 1.0, 700).astype(np.float32)
    w[rng.permutation(700)[:120]] = np.float32(0.25)       # exactly w_min: not eligible
    w[5] = np.nan
    two = rng.uniform(-1, 1, (2, 3)).astype(np.float32)
    As = [np.zeros((0, 3), np.float32), two, a]
    Bs = [np.zeros((0, 3), np.float32), two + np.float32(0.01), b]
    Ws = [np.zeros(0, np.float32), np.ones(2, np.float32), w]
    return As, Bs, Ws, r, planted


def test_mixed_batch_with_weights(gpu):
    As, Bs, Ws, r, planted = _mixed()
    n_hyp = 300
    out = _call(gpu, As, Bs, Ws, r, n_hyp, seed=9, w_min=0.25)
    assert out['n_eligible'].tolist() == [0, 2, 700 - 121]
    for p in range(3):
        _assert_hypotheses(out, p, As[p], Bs[p], Ws[p], r, n_hyp, 9, w_min=0.25, what=f'mixed pair {p}')
        _assert_final(out, p, As[p], Bs[p], Ws[p], r, 4, w_min=0.25, what=f'mixed pair {p}')
    assert out['best_hyp'][:2].tolist() == [-1, -1] and out['best_hyp'][2] >= 0
    el = rr.eligible(Ws[2], 0.25, 700)
    assert np.array_equal(out['mask'][2:].astype(bool), planted & el)
    # the same rows without weights: everything is eligible
    out = _call(gpu, As, Bs, None, r, n_hyp, seed=9)
    assert out['n_eligible'].tolist() == [0, 2, 700]
    _assert_hypotheses(out, 2, As[2], Bs[2], None, r, n_hyp, 9, what='mixed, w NULL')
    _assert_final(out, 2, As[2], Bs[2], None, r, 4, what='mixed, w NULL')
    assert np.array_equal(out['mask'][2:].astype(bool), planted)


def _mirrored():
    """A thin cloud against its mirror image: the refit's covariance has a negative
    determinant, the reflection branch of the solve."""
    rng = np.random.default_rng(52)
    a = (rng.uniform(-1, 1, (80, 3)) * (1.0, 0.7, 0.01)).astype(np.float32)
    R = rr.rotation(rng.normal(size=3), 25.0)
    b = (a.astype(np.float64) * (1, 1, -1)) @ R.T + rng.uniform(-0.3, 0.3, 3)
    return a, (b + rng.normal(size=b.shape) * 1e-3).astype(np.float32), 0.1


def test_mirrored_pair(gpu):
    a, b, r = _mirrored()
    out = _call(gpu, [a], [b], None, r, 256, seed=4)
    _assert_hypotheses(out, 0, a, b, None, r, 256, 4, what='mirrored')
    ref = _assert_final(out, 0, a, b, None, r, 4, what='mirrored')
    K = ref['mask']
    assert K.sum() >= 40 and out['n_updates'][0] >= 1
    H = (a[K] - a[K].mean(0)).astype(np.float64).T @ (b[K] - b[K].mean(0)).astype(np.float64)
    assert np.linalg.det(H) < 0
    R = out['pose'][0, :, :3].astype(np.float64)
    assert abs(np.linalg.det(R) - 1) < 1e-6


def test_collinear_pair(gpu):
    """Every sample and every refit is rank 1: one of the optimal rotations, finite and proper."""
    t = np.linspace(-1, 1, 60)[:, None]
    a = (t * np.array([1.0, 2.0, -0.5])).astype(np.float32)
    b = (a.astype(np.float64) @ rr.rotation([0, 0, 1], 20.0).T + 0.1).astype(np.float32)
    out = _call(gpu, [a], [b], None, 0.01, 128, seed=1)
    _assert_final(out, 0, a, b, None, 0.01, 4, what='collinear', exact=False)
    assert out['best_hyp'][0] >= 0 and (out['hyp_count'][0] != 0).all()
    for T in [out['pose'][0]] + list(out['hyp_pose'][0]):
        R = T[:, :3].astype(np.float64)
        assert np.isfinite(T).all() and abs(np.linalg.det(R) - 1) < 1e-5
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-5
    assert out['n_inliers'][0] == 60 and np.isfinite(out['rmse'][0]) and out['mask'].all()


def test_no_refits_returns_the_winning_hypothesis(gpu):
    a, b, _ = loop_problem(LOOP_SEEDS[0])
    out = _call(gpu, [a], [b], None, LOOP_R, 64, seed=2, n_refits=0)
    best = int(out['best_hyp'][0])
    assert best >= 0 and out['n_updates'][0] == 0
    assert bit_equal(_t(out['pose'][0]), _t(out['hyp_pose'][0, best]))
    assert out['n_inliers'][0] == out['hyp_count'][0, best] == out['mask'].sum()


# ---------------------------------------------------------------------------------------------
# 6: determinism
# ---------------------------------------------------------------------------------------------
def test_determinism_and_seeds(gpu):
    As, Bs, Ws, r, _ = _mixed()
    one = _call(gpu, As, Bs, Ws, r, 500, seed=123, w_min=0.25)
    two = _call(gpu, As, Bs, Ws, r, 500, seed=123, w_min=0.25)
    other = _call(gpu, As, Bs, Ws, r, 500, seed=124, w_min=0.25)
    for k in KEYS:
        assert bit_equal(_t(one[k]), _t(two[k])), k
    assert not np.array_equal(one['hyp_count'][2], other['hyp_count'][2])
    assert not np.array_equal(one['hyp_count'][2], np.roll(other['hyp_count'][2], 1))


def test_short_workspace_is_refused(gpu):
    from _arena import SENTINEL, Arena
    a, b, _ = loop_problem(LOOP_SEEDS[0])
    need = _need(len(a), 1, 64)
    ar = Arena(gpu)
    da, db, do = ar.put(_t(a)), ar.put(_t(b)), ar.put(_t(rr.offsets([len(a)])))
    ws = ar.bytes(need, name='ws')
    outs = [ar.matrix(1, 12, 12, F32, 'out', 'pose', full=False)] + \
           [ar.vector(1, I32, 'out', f'o{k}', full=False) for k in range(5)]
    rc = _L().fgr_ransac_pose(_p(da), _p(db), None, len(a), _p(do), 1, 0.0, 0.05, 64, 0, 4, _p(ws),
                              need - 16, *(_p(o) for o in outs), None, None, None, _st())
    assert rc == -1 and b'fgr_ransac_pose: workspace' in _L().fgr_last_error()
    torch.cuda.synchronize()
    ar.check()
    for o in outs:
        assert bool((o.contiguous().view(torch.int32) == SENTINEL).all())
    assert not bool(ws.any())


# ---------------------------------------------------------------------------------------------
# 7-9: fgreg.robust
# ---------------------------------------------------------------------------------------------
def _dev(xs, gpu):
    return [_t(x).to(gpu) for x in xs]


def test_python_api_matches_the_abi(gpu):
    import fgreg
    As, Bs, Ws, r, _ = _mixed()
    out = fgreg.ransac(_dev(As, gpu), _dev(Bs, gpu), _dev(Ws, gpu), inlier_dist=r, n_hyp=300,
                       w_min=0.25, seed=9, mask=True, hypotheses=True)
    ref = _call(gpu, As, Bs, Ws, r, 300, seed=9, w_min=0.25)
    assert set(out) == {'pose', 'n_inliers', 'n_eligible', 'inlier_rmse', 'best_hyp', 'n_updates',
                        'mask', 'hyp_pose', 'hyp_count'}
    for k, rk in (('pose', 'pose'), ('n_inliers', 'n_inliers'), ('n_eligible', 'n_eligible'),
                  ('inlier_rmse', 'rmse'), ('best_hyp', 'best_hyp'), ('n_updates', 'n_updates'),
                  ('hyp_pose', 'hyp_pose'), ('hyp_count', 'hyp_count')):
        assert bit_equal(out[k].cpu(), _t(ref[rk])), k
    assert [len(x) for x in out['mask']] == [0, 2, 700] and out['mask'][2].dtype == torch.bool
    assert np.array_equal(torch.cat(out['mask']).cpu().numpy(), ref['mask'].astype(bool))
    plain = fgreg.ransac(_dev(As, gpu)[2], _dev(Bs, gpu)[2], inlier_dist=r, n_hyp=64)
    assert set(plain) == {'pose', 'n_inliers', 'n_eligible', 'inlier_rmse', 'best_hyp', 'n_updates'}
    assert tuple(plain['pose'].shape) == (1, 3, 4) and int(plain['n_eligible'][0]) == 700
    with pytest.raises(fgreg.FgrError):
        fgreg.ransac([_t(x) for x in As], [_t(x) for x in Bs], inlier_dist=r)
    with pytest.raises(fgreg.FgrError):
        fgreg.ransac(_dev(As, gpu), _dev(Bs, gpu), inlier_dist=-1.0)


def test_graph_capture(gpu):
    """fgreg.ransac in one torch.cuda.graph on one stream, replayed with refreshed inputs: the
    eager call's bits."""
    import fgreg
    probs = [loop_problem(s)[:2] for s in LOOP_SEEDS[:2]]
    sa, sb = torch.empty(300, 3, device=gpu), torch.empty(300, 3, device=gpu)
    sw = torch.ones(300, device=gpu)
    call = lambda: fgreg.ransac(sa, sb, sw, inlier_dist=LOOP_R, n_hyp=300, seed=5, w_min=0.5,
                                mask=True, hypotheses=True)
    flat = lambda o: [o[k] for k in ('pose', 'n_inliers', 'n_eligible', 'inlier_rmse', 'best_hyp',
                                     'n_updates', 'hyp_pose', 'hyp_count')] + list(o['mask'])
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


def test_ransac_outputs_assembles_the_pose_stage_rows(gpu):
    """The small ModelNet forward fixture's outputs, inlier_dist = 1e3 and one refit: every row
    is an inlier, so the pose is the unweighted Kabsch over the assembled rows -- fgr_procrustes
    with unit weights and no threshold on rows assembled here, and numpy's."""
    import fgreg
    from conftest import loss_fixture
    _, pred, _, _, _, _, _, _ = loss_fixture(gpu)
    out = fgreg.ransac_outputs(pred, 1e3, n_hyp=64, n_refits=1, mask=True)
    B = len(pred['src_kp'])
    assert tuple(out['pose'].shape) == (B, 3, 4)
    for p in range(B):
        a = torch.cat([pred['src_kp'][p], pred['tgt_kp_warped'][p][-1]], 0).contiguous()
        b = torch.cat([pred['src_kp_warped'][p][-1], pred['tgt_kp'][p]], 0).contiguous()
        n = a.shape[0]
        assert int(out['n_eligible'][p]) == int(out['n_inliers'][p]) == n and bool(out['mask'][p].all())
        assert int(out['n_updates'][p]) == 1
        w = torch.ones(n, device=gpu)
        T = torch.empty(3, 4, device=gpu)
        _ok(_L().fgr_procrustes(_p(a), _p(b), _p(w), 1, n, -1.0, _p(T), _st()), 'fgr_procrustes')
        got = out['pose'][p].cpu().numpy()
        _check('pose', _pose_err(got, T.cpu().numpy()), f'ransac_outputs pair {p} vs fgr_procrustes')
        _check('pose', _pose_err(got, rr.kabsch(a.cpu().numpy(), b.cpu().numpy())),
               f'ransac_outputs pair {p} vs numpy')
    # another layer assembles other rows
    first = fgreg.ransac_outputs(pred, 1e3, layer=0, n_hyp=64, n_refits=1)
    assert not bit_equal(first['pose'], out['pose'])


def test_end_to_end_into_icp(gpu):
    """Planted 30 %-inlier correspondences: RANSAC returns the planted set, and ICP on the clouds
    started from its pose converges onto the true pose."""
    import fgreg
    r = 0.05
    a, b, truth, planted = rr.planted_problem(3, 400, 0.3, 0.2 * r, r)
    out = fgreg.ransac(_t(a).to(gpu), _t(b).to(gpu), inlier_dist=r, n_hyp=512, seed=1, mask=True)
    assert np.array_equal(out['mask'][0].cpu().numpy(), planted)
    assert int(out['n_inliers'][0]) == 120
    assert np.abs(out['pose'][0].cpu().numpy() - truth).max() < 5e-3
    tgt = (a.astype(np.float64) @ truth[:, :3].T + truth[:, 3]).astype(np.float32)
    ref = fgreg.icp([_t(a).to(gpu)], [_t(tgt).to(gpu)], out['pose'], 0.05)
    assert float(ref['fitness'][0]) == 1.0 and 1 <= int(ref['n_iters'][0]) < 30
    assert np.abs(ref['pose'][0].cpu().numpy() - truth).max() < 1e-5
    assert float(ref['inlier_rmse'][0]) < 1e-5
