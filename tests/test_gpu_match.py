"""The feature matcher (csrc/match.hip: fgr_feature_nn, fgr_match_pairs) against the numpy
restatement tests/_match_ref.py (pinned on the CPU by tests/test_match_ref.py), through the C ABI
with every operand carved out of a guarded arena (tests/_arena.py) -- each call runs on a clean
and on a poisoned arena with bit-identical results -- and through fgreg.match.

Indices are compared exactly. A row may be excused only if its fp64 gap between best and
second-best score is below twice the asserted score bound and the key the kernel chose scores
within that bound of the best; at most 1 % of a case's rows. With the seeded recipe no gap is
below 1e-5 (test_match_ref.py), so nothing is excused there. best / second are compared at
BOUNDS['score'], relative to |q| max|k|: the worst error measured on the MI355X against the fp64
restatement, times <= 4, never looser than the family ceiling 1e-4 of test_gpu_tail_kernels.py.

  family                                                    measured   asserted   ceiling
  score  best / second, both metrics, d 32 .. 512 (the
         worst: EUCLID distances at d 512)                  1.03e-06   4.0e-06    1e-4

The DOT scores stay below 4.7e-07 at every width; the EUCLID figures carry the fp32 sums |k|^2
and |q|^2 (512 terms at the worst). Twice the asserted bound is below the recipe's smallest gap.

Everything discrete downstream (weights, counts, the fp32 written-out inlier test on inputs
whose residuals all keep 1e-3 r2 away from the radius, asserted first) is compared exactly.
"""
import functools

import numpy as np
import pytest
import torch

import _match_ref as mr
from _arena import assert_both_equal, bit_equal, run_both
from test_match_ref import CASES, case_inputs

pytestmark = pytest.mark.gpu
F32, I32, I64 = torch.float32, torch.int32, torch.int64

BOUNDS = {'score': 4.0e-6}
POSE_BOUND = 2.3e-7         # test_gpu_ransac.py BOUNDS['pose']
MAX_EXCUSED = 0.01


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


def _tables(ns, nt):
    B = len(ns)
    off = mr.offsets(list(ns) + list(nt))
    kv_seg = np.array([(c + B) % (2 * B) for c in range(2 * B)], np.int32)
    return off, kv_seg, mr.offsets([a + b for a, b in zip(ns, nt)])


def _nn(gpu, feats, ns, nt, metric, queries=None, with_second=True):
    """fgr_feature_nn on the packed batch (rows [src clouds ; tgt clouds]) on a clean and a
    poisoned arena -> nn, best, second as numpy arrays."""
    off, kv_seg, _ = _tables(ns, nt)
    n, d = feats.shape

    def fn(ar):
        dk = ar.put(_t(feats), name='k')
        dq = dk if queries is None else ar.put(_t(queries), name='q')
        do, ds = ar.put(_t(off), name='off'), ar.put(_t(kv_seg), name='kv_seg')
        nn, best = ar.vector(n, I32, 'out', 'nn'), ar.vector(n, F32, 'out', 'best')
        second = ar.vector(n, F32, 'out', 'second') if with_second else None
        _ok(_L().fgr_feature_nn(_p(dq), _p(dk), d, n, n, _p(do), _p(do), _p(ds), len(kv_seg),
                                max(list(ns) + list(nt)), metric, _p(nn), _p(best), _p(second),
                                _st()), 'fgr_feature_nn')
        return (nn, best, second) if with_second else (nn, best)

    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    return tuple(t.cpu().numpy() for t in clean)


def _assert_nn(got, feats, ns, nt, metric, ref, what, queries=None):
    """Indices exactly (but for excused near-ties), best / second at BOUNDS['score']."""
    nn, best, second = got
    r_nn, r_best, r_second, gap, scale = ref
    off = mr.offsets(list(ns) + list(nt))
    B = len(ns)
    qs = feats if queries is None else queries
    differs = nn != r_nn
    if differs.any():
        exc = np.zeros(len(nn), bool)
        for c in range(2 * B):
            o = (c + B) % (2 * B)
            lo, hi = off[c], off[c + 1]
            if hi > lo and off[o + 1] > off[o]:
                _, e = mr.excused(qs[lo:hi], feats[off[o]:off[o + 1]], metric, nn[lo:hi], BOUNDS['score'])
                exc[lo:hi] = e
        assert not (differs & ~exc).any(), (what, np.flatnonzero(differs & ~exc)[:5])
        assert exc.sum() <= MAX_EXCUSED * len(nn), (what, int(exc.sum()))
    for name, g, r in (('best', best, r_best), ('second', second, r_second)):
        fin = np.isfinite(r)
        assert np.array_equal(g[~fin], r[~fin].astype(np.float32)), (what, name)     # +-inf exactly
        if fin.any():
            assert np.isfinite(g[fin]).all()
            err = np.abs(g[fin].astype(np.float64) - r[fin]) / np.maximum(scale[fin], 1e-300)
            _check('score', err.max(), f'{what} {name}')


# ---------------------------------------------------------------------------------------------
# 1: indices and scores against fp64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', [mr.DOT, mr.EUCLID])
@pytest.mark.parametrize('d,ns,nt', CASES)
def test_indices_and_scores(gpu, d, ns, nt, metric):
    feats, ref = case_inputs(d, ns, nt)
    got = _nn(gpu, feats, ns, nt, metric)
    _assert_nn(got, feats, ns, nt, metric, ref[metric], f'd {d} B {len(ns)} metric {metric}')
    nn = got[0]
    off = mr.offsets(list(ns) + list(nt))
    for c in range(2 * len(ns)):                # local indices of the opposite cloud
        klen = (list(ns) + list(nt))[(c + len(ns)) % (2 * len(ns))]
        seg = nn[off[c]:off[c + 1]]
        assert ((seg >= 0) & (seg < klen)).all()
    if metric == mr.EUCLID:
        assert (got[1] >= 0).all() and (got[2] >= got[1]).all()
    else:
        assert (got[2] <= got[1]).all()


def test_other_widths_and_no_second(gpu):
    """d = 96, 160, 288 run in a register image wider than the row; second may be NULL."""
    for d in (96, 160, 288):
        src, tgt, _ = mr.descriptors(d, 70, 66, d)
        feats = np.concatenate([src, tgt])
        ref = mr.packed_nn(feats, (70,), (66,), mr.EUCLID)
        _assert_nn(_nn(gpu, feats, (70,), (66,), mr.EUCLID), feats, (70,), (66,), mr.EUCLID, ref, f'd {d}')
    nn, best = _nn(gpu, feats, (70,), (66,), mr.EUCLID, with_second=False)
    full = _nn(gpu, feats, (70,), (66,), mr.EUCLID)
    assert np.array_equal(nn, full[0]) and bit_equal(_t(best), _t(full[1]))


def test_bad_arguments_are_refused(gpu):
    L = _L()
    assert [L.fgr_feature_nn_supported(d) for d in (0, 16, 32, 48, 64, 512, 544)] == [0, 0, 1, 0, 1, 1, 0]
    x = torch.zeros(8, 48, device=gpu)
    off = _t(np.array([0, 4, 8], np.int64)).to(gpu)
    seg = _t(np.array([1, 0], np.int32)).to(gpu)
    nn, best = torch.full((8,), 7, dtype=I32, device=gpu), torch.full((8,), 7.0, device=gpu)
    for d, metric in ((48, 1), (32, 2)):
        rc = L.fgr_feature_nn(_p(x), _p(x), d, 8, 8, _p(off), _p(off), _p(seg), 2, 4, metric, _p(nn),
                              _p(best), None, _st())
        assert rc == -1 and b'fgr_feature_nn' in L.fgr_last_error()
    rc = L.fgr_match_pairs(_p(nn), _p(best), None, _p(x), 8, _p(off), _p(off), 1, 3, 0.0, None, 0.0,
                           _p(x), _p(x), _p(best), _p(nn), None, _st())
    assert rc == -1 and b'fgr_match_pairs' in L.fgr_last_error()
    torch.cuda.synchronize()
    assert bool((nn == 7).all()) and bool((best == 7).all())


# ---------------------------------------------------------------------------------------------
# 2: the tie rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', [mr.DOT, mr.EUCLID])
def test_the_lowest_index_wins_ties(gpu, metric):
    """Bit-identical key rows at j and j + 1, j and j + 16, j and j + 64, and at the first and
    the last key of a 129-key segment, each the best match of one query."""
    rng = np.random.default_rng(0)
    k = rng.standard_normal((129, 64)).astype(np.float32)
    q = (3 * k[[5, 40, 10, 0]]).astype(np.float32)
    k[6], k[56], k[74], k[128] = k[5], k[40], k[10], k[0]
    feats = np.concatenate([q, k])
    nn, best, second = _nn(gpu, feats, (4,), (129,), metric)
    assert nn[:4].tolist() == [5, 40, 10, 0]
    assert bit_equal(_t(best[:4]), _t(second[:4]))              # the duplicate is the second best
    ref = mr.packed_nn(feats, (4,), (129,), metric)
    assert np.array_equal(ref[0][:4], [5, 40, 10, 0])
    # the key side: rows 5 / 6 (and the other pairs) see the same queries and answer alike
    for a, b in ((5, 6), (40, 56), (10, 74), (0, 128)):
        assert nn[4 + a] == nn[4 + b] and best[4 + a] == best[4 + b]


def test_all_zero_descriptors_give_index_zero(gpu):
    feats = np.zeros((65 + 130, 32), np.float32)
    for metric in (mr.DOT, mr.EUCLID):
        nn, best, second = _nn(gpu, feats, (65,), (130,), metric)
        assert (nn == 0).all() and (best == 0).all() and (second == 0).all()


# ---------------------------------------------------------------------------------------------
# 3: degenerate segments
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pairs_problem():
    """Three pairs, d 32: descriptors of the recipe; target points are the copied source points
    under the pair's pose, jittered well inside the radius or displaced far beyond it."""
    ns, nt, r = (77, 65, 129), (130, 63, 17), 0.1
    rng = np.random.default_rng(77)
    src_f, tgt_f, src_x, tgt_x, poses = [], [], [], [], []
    for p, (a, b) in enumerate(zip(ns, nt)):
        s, t, pick = mr.descriptors(500 + p, a, b, 32)
        ang = np.deg2rad(20.0 + 10 * p)
        R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
        tr = np.array([0.1 * p, -0.2, 0.3])
        xs = rng.uniform(-1, 1, (a, 3)).astype(np.float32)
        xt = xs[pick].astype(np.float64) @ R.T + tr + rng.normal(0, 0.01, (b, 3))
        xt[rng.random(b) < 0.3] += 0.5
        src_f.append(s); tgt_f.append(t); src_x.append(xs); tgt_x.append(xt.astype(np.float32))
        poses.append(np.concatenate([R, tr[:, None]], 1).astype(np.float32))
    return ns, nt, r, np.concatenate(src_f + tgt_f), np.concatenate(src_x + tgt_x), np.stack(poses)


def _pairs(gpu, nn, best, second, xyz, ns, nt, mode, max_ratio=0.0, poses=None, r=0.0):
    """fgr_match_pairs on a clean and a poisoned arena -> a, b, w, n_match, n_inlier (or None)."""
    off, _, out_off = _tables(ns, nt)
    n, B = len(nn), len(ns)

    def fn(ar):
        dn, db, ds = ar.put(_t(nn), name='nn'), ar.put(_t(best), name='best'), ar.put(_t(second), name='second')
        dx = ar.put(_t(xyz), name='xyz')
        do, doo = ar.put(_t(off), name='off'), ar.put(_t(out_off), name='out_off')
        dp = ar.put(_t(poses.reshape(B, 12)), name='pose') if poses is not None else None
        a, b = ar.matrix(n, 3, 3, F32, 'out', 'a'), ar.matrix(n, 3, 3, F32, 'out', 'b')
        w, nm = ar.vector(n, F32, 'out', 'w'), ar.vector(B, I32, 'out', 'n_match')
        ni = ar.vector(B, I32, 'out', 'n_inlier') if poses is not None else None
        _ok(_L().fgr_match_pairs(_p(dn), _p(db), _p(ds), _p(dx), n, _p(do), _p(doo), B, mode, max_ratio,
                                 _p(dp), r, _p(a), _p(b), _p(w), _p(nm), _p(ni), _st()), 'fgr_match_pairs')
        return (a, b, w, nm) + ((ni,) if ni is not None else ())

    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    out = [t.cpu().numpy() for t in clean]
    return out + [None] * (5 - len(out))


def _assert_pairs(got, nn, best, second, xyz, ns, nt, mode, max_ratio=0.0, poses=None, r=0.0):
    a, b, w, nm, ni = got
    off, _, out_off = _tables(ns, nt)
    B = len(ns)
    for p in range(B):
        s, t = slice(off[p], off[p + 1]), slice(off[B + p], off[B + p + 1])
        ra, rb, rw, rn = mr.match_pairs(nn[s], nn[t], xyz[s], xyz[t], mode, max_ratio, best[s], second[s],
                                        best[t], second[t])
        o = slice(out_off[p], out_off[p + 1])
        assert np.array_equal(a[o], ra) and np.array_equal(b[o], rb), p
        assert np.array_equal(w[o], rw) and nm[p] == rn, (p, mode, max_ratio)
        if poses is not None:
            cnt, gap = mr.inliers_f32(ra, rb, rw, poses[p], r)
            assert gap >= 1e-3, (p, gap)                        # the precondition, not a skip
            assert ni[p] == cnt == mr.inliers(ra, rb, rw, poses[p], r), (p, ni[p], cnt)


def test_an_empty_target_cloud(gpu):
    ns, nt = (20, 30, 17), (25, 0, 40)
    rng = np.random.default_rng(4)
    feats = np.concatenate([mr.descriptors(40 + p, a, max(b, 1), 32)[i][:(a, b)[i]]
                            for i in (0, 1) for p, (a, b) in enumerate(zip(ns, nt))])
    xyz = rng.uniform(-1, 1, (len(feats), 3)).astype(np.float32)
    ref = mr.packed_nn(feats, ns, nt, mr.EUCLID)
    got = _nn(gpu, feats, ns, nt, mr.EUCLID)
    _assert_nn(got, feats, ns, nt, mr.EUCLID, ref, 'empty target')
    nn, best, second = got
    assert (nn[20:50] == -1).all() and np.isposinf(best[20:50]).all() and np.isposinf(second[20:50]).all()
    dot = _nn(gpu, feats, ns, nt, mr.DOT)
    assert (dot[0][20:50] == -1).all() and np.isneginf(dot[1][20:50]).all()
    for mode in (mr.SRC, mr.MUTUAL, mr.BILATERAL):
        res = _pairs(gpu, nn, best, second, xyz, ns, nt, mode)
        _assert_pairs(res, nn, best, second, xyz, ns, nt, mode)
        a, b, w, nm, _ = res
        assert nm[1] == 0 and not w[45:75].any() and not b[45:75].any() and nm[0] > 0 and nm[2] > 0
    # the other pairs are what they are without the empty one
    keep = np.r_[0:20, 50:67, 67:92, 92:132]
    alone = _nn(gpu, feats[keep], (20, 17), (25, 40), mr.EUCLID)
    for g, x in zip(got, alone):
        assert bit_equal(_t(g[keep]), _t(x))


def test_one_key_segments(gpu):
    src, tgt, _ = mr.descriptors(8, 1, 65, 64)
    feats = np.concatenate([src, tgt])
    for metric, inf in ((mr.DOT, -np.inf), (mr.EUCLID, np.inf)):
        got = _nn(gpu, feats, (1,), (65,), metric)
        _assert_nn(got, feats, (1,), (65,), metric, mr.packed_nn(feats, (1,), (65,), metric), 'one key')
        assert (got[0][1:] == 0).all() and (got[2][1:] == inf).all() and np.isfinite(got[1]).all()
        assert np.isfinite(got[2][0])


# ---------------------------------------------------------------------------------------------
# 4: scale invariance
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,ns,nt', [CASES[2], CASES[4]])
def test_scale_invariance(gpu, d, ns, nt):
    """Every row times 2^6 and 2^-6: the same indices, best and second exactly 2^+-12 times the
    unscaled ones. Fails if the fp16 split is not scaled per row."""
    feats, _ = case_inputs(d, ns, nt)
    for metric in (mr.DOT, mr.EUCLID):
        nn, best, second = _nn(gpu, feats, ns, nt, metric)
        for e in (6, -6):
            s_nn, s_best, s_second = _nn(gpu, np.ldexp(feats, e), ns, nt, metric)
            assert np.array_equal(s_nn, nn), (metric, e)
            assert bit_equal(_t(s_best), _t(np.ldexp(best, 2 * e))), (metric, e)
            assert bit_equal(_t(s_second), _t(np.ldexp(second, 2 * e))), (metric, e)


# ---------------------------------------------------------------------------------------------
# 5: fgr_match_pairs from the device's own neighbours
# ---------------------------------------------------------------------------------------------
def test_match_pairs_modes_ratio_and_inliers(gpu):
    ns, nt, r, feats, xyz, poses = _pairs_problem()
    nn, best, second = _nn(gpu, feats, ns, nt, mr.EUCLID)
    _assert_nn((nn, best, second), feats, ns, nt, mr.EUCLID, mr.packed_nn(feats, ns, nt, mr.EUCLID), 'pairs')
    seen = set()
    for mode in (mr.SRC, mr.MUTUAL, mr.BILATERAL):
        for ratio in (0.0, 0.9):
            res = _pairs(gpu, nn, best, second, xyz, ns, nt, mode, ratio, poses, r)
            _assert_pairs(res, nn, best, second, xyz, ns, nt, mode, ratio, poses, r)
            assert (res[4] <= res[3]).all() and (res[4] > 0).all()
            seen.add(tuple(res[3].tolist()))
        plain = _pairs(gpu, nn, best, second, xyz, ns, nt, mode)        # without a pose
        assert plain[4] is None
    assert len(seen) == 6                   # every mode and the ratio test change the counts


# ---------------------------------------------------------------------------------------------
# 6: fgreg.match
# ---------------------------------------------------------------------------------------------
def _dev(xs, gpu):
    return [_t(x).to(gpu) for x in xs]


def _split(x, ns, nt):
    off = mr.offsets(list(ns) + list(nt))
    B = len(ns)
    return [x[off[c]:off[c + 1]] for c in range(B)], [x[off[B + c]:off[B + c + 1]] for c in range(B)]


def test_match_features_matches_the_abi(gpu):
    import fgreg
    ns, nt, r, feats, xyz, poses = _pairs_problem()
    fs, ft = _split(feats, ns, nt)
    xs, xt = _split(xyz, ns, nt)
    out = fgreg.match_features(_dev(fs, gpu), _dev(ft, gpu), _dev(xs, gpu), _dev(xt, gpu), mode='bilateral',
                               max_ratio=0.9, pose=_t(poses).to(gpu), inlier_dist=r)
    assert set(out) == {'a', 'b', 'w', 'nn_src', 'nn_tgt', 'score_src', 'score_tgt', 'n_matches',
                        'n_inliers', 'inlier_ratio'}
    nn, best, second = _nn(gpu, feats, ns, nt, mr.EUCLID)
    a, b, w, nm, ni = _pairs(gpu, nn, best, second, xyz, ns, nt, mr.BILATERAL, 0.9, poses, r)
    n_s = sum(ns)
    for key, want in (('a', a), ('b', b), ('w', w), ('nn_src', nn[:n_s]), ('nn_tgt', nn[n_s:]),
                      ('score_src', best[:n_s]), ('score_tgt', best[n_s:])):
        assert bit_equal(torch.cat(out[key]).cpu(), _t(want)), key
    assert [len(x) for x in out['a']] == [s + t for s, t in zip(ns, nt)]
    assert [len(x) for x in out['nn_tgt']] == list(nt)
    assert np.array_equal(out['n_matches'].cpu().numpy(), nm) and np.array_equal(out['n_inliers'].cpu().numpy(), ni)
    assert np.allclose(out['inlier_ratio'].cpu().numpy(), ni / np.maximum(nm, 1), rtol=1e-6, atol=0)
    fmr = fgreg.feature_match_recall(out['inlier_ratio'], 0.05)
    assert float(fmr) == float((ni / np.maximum(nm, 1) > 0.05).mean())
    one = fgreg.match_features(_dev(fs, gpu)[0], _dev(ft, gpu)[0], _dev(xs, gpu)[0], _dev(xt, gpu)[0])
    assert set(one) == {'a', 'b', 'w', 'nn_src', 'nn_tgt', 'score_src', 'score_tgt', 'n_matches'}
    assert bit_equal(one['nn_src'][0].cpu(), _t(nn[:ns[0]]))
    with pytest.raises(fgreg.FgrError):                     # host tensors
        fgreg.match_features([_t(x) for x in fs], [_t(x) for x in ft], [_t(x) for x in xs], [_t(x) for x in xt])
    with pytest.raises(fgreg.FgrError):                     # d = 48
        fgreg.match_features(torch.zeros(9, 48, device=gpu), torch.zeros(7, 48, device=gpu),
                             torch.zeros(9, 3, device=gpu), torch.zeros(7, 3, device=gpu))
    with pytest.raises(fgreg.FgrError):
        fgreg.match_features(_dev(fs, gpu), _dev(ft, gpu), _dev(xs, gpu), _dev(xt, gpu), metric='bilinear')


@functools.lru_cache(maxsize=None)
def _forward(gpu):
    """A seeded ModelNet forward of two pairs -> (model, outputs)."""
    import fgreg
    from fgreg.synthetic import make_batch
    torch.manual_seed(0)
    np.random.seed(0)
    model = fgreg.RegTR(fgreg.config.get('modelnet')).eval().to(gpu)
    src, tgt, _ = make_batch('modelnet', 2)
    batch = {'src_xyz': _dev(src, gpu), 'tgt_xyz': _dev(tgt, gpu)}
    with torch.no_grad():
        out = model(batch)
    torch.cuda.synchronize()
    return model, out


def _same(x, y):
    assert set(x) == set(y)
    for k in x:
        xs, ys = (x[k], y[k]) if isinstance(x[k], list) else ([x[k]], [y[k]])
        assert len(xs) == len(ys) and all(bit_equal(a, b) for a, b in zip(xs, ys)), k


def test_match_outputs_on_a_forward(gpu):
    import fgreg
    from fgreg import linear, loss, match
    model, out = _forward(gpu)
    B = len(out['src_kp'])
    assert B == 2
    fs, ft = [f[-1] for f in out['src_feat']], [f[-1] for f in out['tgt_feat']]
    _same(fgreg.match_outputs(out), fgreg.match_features(fs, ft, out['src_kp'], out['tgt_kp']))
    _same(fgreg.match_outputs(out, layer=0, mode='src', metric='dot'),
          fgreg.match_features([f[0] for f in out['src_feat']], [f[0] for f in out['tgt_feat']],
                               out['src_kp'], out['tgt_kp'], mode='src', metric='dot'))
    _same(fgreg.match_outputs(out, features='un'),
          fgreg.match_features(list(out['src_feat_un']), list(out['tgt_feat_un']), out['src_kp'], out['tgt_kp']))
    # with the model: the bilinear form it was trained under = 'dot' on X W_sym by hand
    for features, crit, (s, t) in (('cond', model.feature_criterion, (fs, ft)),
                                   ('un', model.feature_criterion_un,
                                    (list(out['src_feat_un']), list(out['tgt_feat_un'])))):
        got = fgreg.match_outputs(out, model=model, features=features)
        _same(got, fgreg.match_features(s, t, out['src_kp'], out['tgt_kp'], metric='bilinear', W=crit.W))
        X = torch.cat(s + t, 0).contiguous()
        with linear.mode_scope('f16x3'):
            Q = linear.linear(X, loss._w_sym(crit.W))
        ns, nt = [len(x) for x in s], [len(x) for x in t]
        off, kv_seg, _ = match._tables(ns, nt, X.device)
        nn, best, second = match.feature_nn(Q, X, off, off, kv_seg, max(ns + nt), 0)
        assert bit_equal(torch.cat(got['nn_src'] + got['nn_tgt']), nn)
        assert bit_equal(torch.cat(got['score_src'] + got['score_tgt']), best)
        ref = mr.packed_nn(X.cpu().numpy(), ns, nt, mr.DOT, queries=Q.cpu().numpy())
        _assert_nn((nn.cpu().numpy(), best.cpu().numpy(), second.cpu().numpy()), X.cpu().numpy(), ns, nt,
                   mr.DOT, ref, f'bilinear {features}', queries=Q.cpu().numpy())
    # the same in bf16 mode: the matcher's products stay f16x3
    fgreg.set_precision('bf16')
    try:
        again = fgreg.match_outputs(out, model=model)
    finally:
        fgreg.set_precision('fp32')
    _same(again, fgreg.match_outputs(out, model=model))


def test_register_features(gpu):
    import fgreg
    model, out = _forward(gpu)
    reg = fgreg.register_features(out, 0.1, model=model, n_hyp=256, seed=3)
    m = reg['matches']
    _same(m, fgreg.match_outputs(out, model=model))
    hand = fgreg.ransac(m['a'], m['b'], m['w'], inlier_dist=0.1, n_hyp=256, seed=3)
    assert set(reg) == set(hand) | {'matches'}
    for k in hand:
        assert bit_equal(reg[k], hand[k]), k
    assert np.array_equal(reg['n_eligible'].cpu().numpy(), m['n_matches'].cpu().numpy())


def test_register_features_recovers_a_planted_pose(gpu):
    """One synthetic pair whose descriptors are right for 60 % of the rows (the others are
    random): the mutual matches carry the pose."""
    import fgreg
    from test_gpu_icp import _pose_err
    rng = np.random.default_rng(12)
    n, d = 300, 64
    src, _, _ = mr.descriptors(3, n, 1, d)
    perm = rng.permutation(n)
    right = rng.random(n) < 0.6
    tgt = src[perm] + rng.standard_normal((n, d)) * (0.2 / np.sqrt(d))
    tgt[~right] = rng.standard_normal((int((~right).sum()), d))
    tgt = (tgt / np.linalg.norm(tgt, axis=1, keepdims=True)).astype(np.float32)
    ang = np.deg2rad(35.0)
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1.0, 0], [-np.sin(ang), 0, np.cos(ang)]])
    truth = np.concatenate([R, np.array([[0.3], [-0.2], [0.1]])], 1)
    xs = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    xt = (xs[perm].astype(np.float64) @ R.T + truth[:, 3]).astype(np.float32)
    outputs = {'src_feat': [_t(src[None]).to(gpu)], 'tgt_feat': [_t(tgt[None]).to(gpu)],
               'src_kp': [_t(xs).to(gpu)], 'tgt_kp': [_t(xt).to(gpu)]}
    reg = fgreg.register_features(outputs, 0.05, n_hyp=512, seed=1, pose=_t(truth.astype(np.float32)).to(gpu))
    m = reg['matches']
    hand = fgreg.ransac(m['a'], m['b'], m['w'], inlier_dist=0.05, n_hyp=512, seed=1)
    assert _pose_err(reg['pose'][0].cpu().numpy(), hand['pose'][0].cpu().numpy()) <= POSE_BOUND
    n_match, n_inl = int(m['n_matches'][0]), int(m['n_inliers'][0])
    assert n_match >= 0.5 * n and 0.5 * n <= n_inl <= n_match
    assert int(reg['n_inliers'][0]) >= n_inl
    assert np.abs(reg['pose'][0].cpu().numpy() - truth).max() < 1e-5
    assert float(fgreg.feature_match_recall(m['inlier_ratio'])) == 1.0


def test_graph_capture(gpu):
    """match_features in one torch.cuda.graph, replayed with refreshed inputs after one eager
    call: the eager call's bits."""
    import fgreg
    ns, nt, r, feats, xyz, poses = _pairs_problem()
    other = np.ascontiguousarray(feats[::-1])
    sf = torch.empty(len(feats), 32, device=gpu)
    sx = _t(xyz).to(gpu)
    gt = _t(poses).to(gpu)
    fs, ft = _split(sf, ns, nt)
    xs, xt = _split(sx, ns, nt)
    call = lambda: fgreg.match_features(fs, ft, xs, xt, max_ratio=0.9, pose=gt, inlier_dist=r)
    flat = lambda o: [t for k in sorted(o) for t in (o[k] if isinstance(o[k], list) else [o[k]])]
    eager = []
    for x in (feats, other):
        sf.copy_(_t(x))
        eager.append([t.clone() for t in flat(call())])
    torch.cuda.synchronize()
    assert not all(bit_equal(x, y) for x, y in zip(*eager))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = flat(call())
    for which in (1, 0):
        sf.copy_(_t((feats, other)[which]))
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(eager[which], cap):
            assert bit_equal(x, y)
