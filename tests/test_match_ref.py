"""Pins tests/_match_ref.py (the numpy restatement the GPU tests compare csrc/match.hip with)
to the reference's matching utilities (models/ransaclib/registration_utils.py, recorded by
tests/golden/make_match_golden.py into tests/golden/match_ref.npz), and asserts the near-tie
condition for every input tests/test_gpu_match.py takes from the seeded recipe.

Naming: the reference's `ref` is our target and its `src` our source. It orders mutual pairs by
ref index and stacks bilateral rows [ref; src], so pairs are compared as sets (mutual) and
multisets (bilateral) of (source, target) indices."""
import functools
import os

import numpy as np
import pytest

import _match_ref as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'match_ref.npz')

# the shapes of test_gpu_match.py's first test: (d, source lengths, target lengths). Every
# length of {1, 15, 16, 17, 63, 64, 65, 129, 200} occurs, as queries and as keys.
CASES = [
    (32, (65,), (63,)),
    (64, (129,), (17,)),
    (256, (200,), (64,)),
    (512, (16,), (129,)),
    (32, (1, 15, 200), (64, 65, 17)),
    (64, (63, 129, 16), (1, 200, 15)),
    (256, (17, 64, 65), (129, 1, 63)),
    (512, (15, 1, 64), (16, 17, 65)),
]
MIN_GAP = 1e-5          # no recipe row is nearer to a tie than this (relative to |q| max|k|)


@functools.lru_cache(maxsize=None)
def case_inputs(d, ns, nt):
    """-> feats (rows [src clouds ; tgt clouds]) fp32 and, per metric, the restatement's
    (nn, best, second, gap, scale). Computed once and shared; callers must not modify it."""
    src, tgt = [], []
    for p, (a, b) in enumerate(zip(ns, nt)):
        s, t, _ = mr.descriptors(1000 * d + 10 * p + len(ns), a, b, d)
        src.append(s)
        tgt.append(t)
    feats = np.concatenate(src + tgt)
    feats.setflags(write=False)
    return feats, {m: mr.packed_nn(feats, ns, nt, m) for m in (mr.DOT, mr.EUCLID)}


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLDEN))


def _fixture_nn(gold):
    nn_src = mr.feature_nn(gold['src_feat'], gold['tgt_feat'], mr.EUCLID)
    nn_tgt = mr.feature_nn(gold['tgt_feat'], gold['src_feat'], mr.EUCLID)
    return nn_src, nn_tgt


def test_fixture_is_the_recipe(gold):
    s, t, _ = mr.descriptors(20240, 77, 130, 32)
    assert np.array_equal(s, gold['src_feat']) and np.array_equal(t, gold['tgt_feat'])


def test_one_way_neighbours(gold):
    (nn_src, *_), (nn_tgt, *_) = _fixture_nn(gold)
    assert np.array_equal(gold['oneway_ref'], np.arange(130))
    assert np.array_equal(nn_tgt, gold['oneway_src'])              # every target row's source
    assert np.array_equal(gold['oneway_swapped_ref'], np.arange(77))
    assert np.array_equal(nn_src, gold['oneway_swapped_src'])      # every source row's target


@pytest.mark.parametrize('mode,name', [(mr.SRC, 'oneway_swapped'), (mr.MUTUAL, 'mutual'),
                                       (mr.BILATERAL, 'bilateral')])
def test_modes_and_inlier_ratio(gold, mode, name):
    (nn_src, *_), (nn_tgt, *_) = _fixture_nn(gold)
    a, b, w, n = mr.match_pairs(nn_src, nn_tgt, gold['src_xyz'], gold['tgt_xyz'], mode)
    got = mr.index_pairs(nn_src, nn_tgt, w)
    if name == 'oneway_swapped':           # called with ref = our source
        want = list(zip(gold[name + '_ref'].tolist(), gold[name + '_src'].tolist()))
    else:
        want = list(zip(gold[name + '_src'].tolist(), gold[name + '_ref'].tolist()))
    assert n == len(want) == len(got)
    if mode == mr.MUTUAL:
        assert len(set(got)) == len(got) and set(got) == set(want)
    else:
        assert sorted(got) == sorted(want)
    # the rows are the pairs' points
    on = w > 0
    assert np.array_equal(a[on], gold['src_xyz'][[p[0] for p in got]])
    assert np.array_equal(b[on], gold['tgt_xyz'][[p[1] for p in got]])
    pose, r = gold['transform'][:3], float(gold['radius'])
    assert mr.inliers(a, b, w, pose, r) / n == pytest.approx(float(gold[name + '_inlier_ratio']), abs=1e-12)
    cnt32, gap = mr.inliers_f32(a, b, w, pose.astype(np.float32), r)
    assert gap >= 1e-3 and cnt32 == mr.inliers(a, b, w, pose, r)


def test_mode_weights():
    s, t, _ = mr.descriptors(5, 40, 50, 32)
    xs, xt = np.zeros((40, 3), np.float32), np.ones((50, 3), np.float32)
    nn_s, bs, ss, _ = mr.feature_nn(s, t, mr.EUCLID)
    nn_t, bt, st, _ = mr.feature_nn(t, s, mr.EUCLID)
    _, _, w_src, n_src = mr.match_pairs(nn_s, nn_t, xs, xt, mr.SRC)
    _, _, w_mut, n_mut = mr.match_pairs(nn_s, nn_t, xs, xt, mr.MUTUAL)
    _, _, w_bi, n_bi = mr.match_pairs(nn_s, nn_t, xs, xt, mr.BILATERAL)
    assert n_src == 40 and w_src[:40].all() and not w_src[40:].any()
    assert n_bi == 90 and w_bi.all()
    assert 0 < n_mut < 40 and not w_mut[40:].any()
    assert all(nn_t[nn_s[i]] == i for i in np.flatnonzero(w_mut))
    kw = dict(best_src=bs, second_src=ss, best_tgt=bt, second_tgt=st)
    _, _, w_r, n_r = mr.match_pairs(nn_s, nn_t, xs, xt, mr.BILATERAL, 0.9, **kw)
    keep = np.concatenate([bs, bt]).astype(np.float32) < np.float32(0.81) * np.concatenate([ss, st]).astype(np.float32)
    assert 0 < n_r < 90 and np.array_equal(w_r > 0, keep)
    # an empty opposite cloud: no neighbour, weight 0
    e = np.zeros((0, 32), np.float32)
    nn_e, be, se, _ = mr.feature_nn(s, e, mr.EUCLID)
    assert (nn_e == -1).all() and np.isinf(be).all() and np.isinf(se).all()
    assert mr.match_pairs(nn_e, np.zeros(0, np.int32), xs, np.zeros((0, 3)), mr.BILATERAL)[3] == 0


def test_the_lowest_index_wins_ties():
    rng = np.random.default_rng(0)
    k = rng.standard_normal((129, 32)).astype(np.float32)
    q = (3 * k[[5, 40, 10, 0]]).astype(np.float32)
    k[6], k[56], k[74], k[128] = k[5], k[40], k[10], k[0]
    for metric in (mr.DOT, mr.EUCLID):
        nn, best, second, gap = mr.feature_nn(q, k, metric)
        assert nn.tolist() == [5, 40, 10, 0] and (gap == 0).all() and np.array_equal(best, second)
    nn, best, second, _ = mr.feature_nn(np.zeros((3, 32)), np.zeros((7, 32)), mr.EUCLID)
    assert (nn == 0).all() and (best == 0).all() and (second == 0).all()
    nn, best, second, _ = mr.feature_nn(q, k[:1], mr.DOT)
    assert (nn == 0).all() and np.isneginf(second).all() and np.isfinite(best).all()


def test_euclid_score_is_the_nearest_key():
    s, t, _ = mr.descriptors(9, 30, 45, 64)
    t = (t * np.linspace(0.5, 2.0, 45)[:, None]).astype(np.float32)      # norms differ
    d2 = ((s[:, None, :].astype(np.float64) - t[None].astype(np.float64)) ** 2).sum(-1)
    nn, best, second, _ = mr.feature_nn(s, t, mr.EUCLID)
    assert np.array_equal(nn, d2.argmin(1))
    assert np.allclose(best, d2.min(1), rtol=0, atol=1e-12)
    assert np.allclose(second, np.sort(d2, 1)[:, 1], rtol=0, atol=1e-12)


@pytest.mark.parametrize('d,ns,nt', CASES + [(256, (600,), (580,)), (256, (77,), (130,))])
def test_no_recipe_row_is_near_a_tie(d, ns, nt):
    """The near-tie condition of test_gpu_match.py: a row may be excused from exact index
    equality only if its fp64 gap is below twice the asserted score bound. With the recipe no
    gap comes near it, so the reference alone excuses nothing."""
    _, ref = case_inputs(d, ns, nt)
    for metric, (nn, best, second, gap, scale) in ref.items():
        many = np.isfinite(gap)
        assert (gap[many] >= MIN_GAP * scale[many]).all(), (metric, float((gap[many] / scale[many]).min()))
