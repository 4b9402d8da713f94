"""CPU: pins tests/_ransac_ref.py, the numpy restatement that tests/test_gpu_ransac.py holds the
RANSAC kernels to -- the hash against plain Python integers, the ranks' statistics, a planted
problem with a known answer, the corner cases of the state machine -- and the argument checks
of fgr_ransac_pose / fgr_ransac_workspace, which need no GPU."""
import ctypes

import numpy as np

import _ransac_ref as rr

LOOP_SEEDS = (5, 9, 16, 24, 29, 32)        # test_gpu_ransac.py's refit-loop inputs
LOOP_M, LOOP_FRAC, LOOP_R, LOOP_HYP, LOOP_REFITS = 300, 0.6, 0.05, 8, 8


def loop_problem(seed):
    a, b, _, planted = rr.planted_problem(seed, LOOP_M, LOOP_FRAC, 0.9 * LOOP_R, LOOP_R)
    return a, b, planted


def _hash_int(seed, head, q, k):
    M = 0xFFFFFFFF
    x = seed ^ ((head * 0x9E3779B9) & M)
    x ^= (q * 0x85EBCA6B) & M
    x = ((x ^ (x >> 16)) * 0x7FEB352D) & M
    x ^= (k * 0xC2B2AE35) & M
    x = ((x ^ (x >> 15)) * 0x846CA68B) & M
    return x ^ (x >> 16)


def test_hash_matches_plain_integers():
    args = np.random.default_rng(0).integers(0, 2 ** 32, (1000, 4))
    for s, h, q, k in args.tolist():
        assert int(rr.hash32(s, h, q, k)) == _hash_int(s, h, q, k)
    # broadcast over the hypothesis index, as ranks() uses it
    got = rr.hash32(7, 2, 3, np.arange(50))
    assert got.tolist() == [_hash_int(7, 2, 3, k) for k in range(50)]


def test_hash_matches_the_dropout_restatement():
    """The same function as fgreg.autograd's restatement of common.h attn_drop_hash: an entry is
    dropped iff hash < p * 2^32."""
    from fgreg import autograd
    h = rr.hash32(11, 3, np.arange(5)[:, None], np.arange(40)[None, :])
    drop = autograd.attn_drop_mask(11, 0.25, 3, np.arange(5), np.arange(40))
    assert np.array_equal(drop, h < np.uint64(int(0.25 * 2 ** 32)))


def test_rank_statistics():
    m, n_hyp = 100, 65536
    rk = rr.ranks(0, 0, n_hyp, m)
    assert rk.min() == 0 and rk.max() == m - 1
    hist = np.bincount(rk.ravel(), minlength=m)
    want = 3 * n_hyp / m                                   # 1966 a bin, sigma 44
    assert np.abs(hist - want).max() < 6 * np.sqrt(want)
    share = 1.0 - rr.valid_ranks(rk, m).mean()
    expect = 1.0 - (m - 1) * (m - 2) / m ** 2
    print(f'repeated-rank share {share:.4f} expected {expect:.4f}')
    assert abs(share - expect) <= 0.25 * expect
    # another pair and another seed draw other samples
    assert not np.array_equal(rk, rr.ranks(0, 1, n_hyp, m))
    assert not np.array_equal(rk, rr.ranks(1, 0, n_hyp, m))


def test_planted_pose_is_recovered():
    r = 0.05
    a, b, truth, planted = rr.planted_problem(3, 400, 0.3, 0.2 * r, r)
    assert planted.sum() == 120
    out = rr.ransac(a, b, None, r, 512, seed=1)
    assert np.array_equal(out['mask'], planted) and out['n_inliers'] == 120
    assert out['n_eligible'] == 400 and out['best_hyp'] >= 0
    assert out['hyp_count'][out['best_hyp']] == out['hyp_count'].max()
    assert np.abs(out['pose'] - truth).max() < 5e-3, np.abs(out['pose'] - truth).max()
    assert out['rmse'] < 0.2 * r


def test_too_few_eligible_rows():
    rng = np.random.default_rng(4)
    for m in (0, 2):
        a = rng.uniform(-1, 1, (m, 3))
        out = rr.ransac(a, a, None, 0.1, 16)
        assert out['best_hyp'] == -1 and (out['hyp_count'] == -1).all()
        assert np.array_equal(out['pose'], rr.EYE) and out['n_inliers'] == 0
        assert out['rmse'] == 0.0 and out['n_updates'] == 0 and not out['mask'].any()
        assert np.array_equal(out['hyp_pose'], np.tile(rr.EYE, (16, 1, 1)))


def test_all_ranks_repeat():
    m, n_hyp = 3, 4
    seed = next(s for s in range(200) if not rr.valid_ranks(rr.ranks(s, 0, n_hyp, m), m).any())
    a = np.random.default_rng(5).uniform(-1, 1, (m, 3))
    out = rr.ransac(a, a, None, 0.1, n_hyp, seed=seed)
    assert out['best_hyp'] == -1 and out['n_eligible'] == 3 and (out['hyp_count'] == -1).all()


def test_weight_threshold_is_strict():
    r = 0.05
    a, b, _, planted = rr.planted_problem(6, 60, 0.8, 0.1 * r, r)
    w = np.full(60, 0.7, np.float32)
    cut = np.flatnonzero(planted)[:5]
    w[cut] = np.float32(0.25)                              # exactly w_min: not eligible
    out = rr.ransac(a, b, w, r, 64, w_min=0.25)
    assert out['n_eligible'] == 55 and not out['mask'][cut].any()
    want = planted.copy()
    want[cut] = False
    assert np.array_equal(out['mask'], want)
    assert rr.ransac(a, b, w, r, 64, w_min=0.2)['n_eligible'] == 60
    w[0] = np.nan
    assert rr.ransac(a, b, w, r, 64, w_min=0.2)['n_eligible'] == 59


def test_mirrored_cloud_takes_the_reflection_fix():
    rng = np.random.default_rng(7)
    a = rng.uniform(-1, 1, (50, 3))
    R = rr.rotation([1, -2, 0.5], 30.0)
    b = (a * (1, 1, -1)) @ R.T + 0.2
    H = (a - a.mean(0)).T @ (b - b.mean(0))
    assert np.linalg.det(H) < 0
    T = rr.kabsch(a, b)
    assert abs(np.linalg.det(T[:, :3]) - 1) < 1e-12
    assert np.abs(T[:, :3].T @ T[:, :3] - np.eye(3)).max() < 1e-12
    # a proper rotation cannot fit a mirror image, and the unfixed solution would
    assert np.abs(a @ T[:, :3].T + T[:, 3] - b).max() > 0.1
    U, _, Vt = np.linalg.svd(H)
    assert np.linalg.det(Vt.T @ U.T) < 0
    # the whole call stays finite and proper on it
    out = rr.ransac(a, b, None, 0.3, 64, seed=2)
    assert out['best_hyp'] >= 0 and abs(np.linalg.det(out['pose'][:, :3].astype(np.float64)) - 1) < 1e-5


def test_collinear_points():
    t = np.linspace(-1, 1, 40)[:, None]
    a = t * np.array([1.0, 2.0, -0.5])
    b = a @ rr.rotation([0, 0, 1], 20.0).T + 0.1
    T = rr.kabsch(a, b)
    assert np.isfinite(T).all() and abs(np.linalg.det(T[:, :3]) - 1) < 1e-9
    assert np.abs(a @ T[:, :3].T + T[:, 3] - b).max() < 1e-9     # one of the optimal rotations
    out = rr.ransac(a, b, None, 0.01, 32, seed=1)
    assert out['best_hyp'] >= 0 and np.isfinite(out['pose']).all() and out['n_inliers'] == 40


def test_selection_takes_the_first_maximum():
    assert rr.select([-1, 3, 7, 7, 2]) == 2 and rr.select([-1, -1]) == -1 and rr.select([-1, 0]) == 1


def test_refit_stops_as_stated():
    r = 0.05
    a, b, truth, planted = rr.planted_problem(8, 100, 0.7, 0.05 * r, r)
    T = truth.astype(np.float32)
    c = rr.count(T, a, b, r)
    assert c == 70
    assert rr.refit(a, b, T, c, r, 0)['n_updates'] == 0
    assert np.array_equal(rr.refit(a, b, T, c, r, 0)['pose'], T)
    one = rr.refit(a, b, T, c, r, 5)
    assert one['n_updates'] == 1 and one['n_inliers'] == 70      # c' == c: adopted, then stop
    # a winner with two inliers cannot be refitted
    far = np.concatenate([truth[:, :3], truth[:, 3:] + 10.0], 1).astype(np.float32)
    b2 = b.copy()
    b2[:2] = rr.transform32(far, a[:2])
    two = rr.refit(a, b2, far, 2, r, 5)
    assert two['n_updates'] == 0 and two['n_inliers'] == 2 and np.array_equal(two['pose'], far)


def test_loop_problem_meets_its_precondition():
    """The refit-loop inputs of test_gpu_ransac.py: m = 300, 60 % planted with noise <= 0.9 r,
    n_hyp = 8. On each seed the restatement alone adopts at least 2 refits, ends on the planted
    set, and no pose it scores has a row closer than 1e-3 r2 to the radius."""
    for seed in LOOP_SEEDS:
        a, b, planted = loop_problem(seed)
        out = rr.ransac(a, b, None, LOOP_R, LOOP_HYP, seed=seed, n_refits=LOOP_REFITS)
        assert out['n_updates'] >= 2, (seed, out['n_updates'])
        assert np.array_equal(out['mask'], planted), seed
        assert min(out['gaps']) >= 1e-3, (seed, out['gaps'])


def _lib():
    import fgreg
    return fgreg.load()


def test_ransac_argument_errors_need_no_gpu():
    """Every refusal is FGR_E_ARG (-1) with the entry point's name in fgr_last_error(), before
    anything is launched: the pointers here are host addresses that are never read."""
    L = _lib()
    f = ctypes.c_float
    nb = ctypes.c_size_t(0)
    assert L.fgr_ransac_workspace(100, 2, 1000, nb) == 0 and nb.value > 0
    need = nb.value
    for bad in ((-1, 2, 1000), (1 << 31, 2, 1000), (100, 0, 1000), (100, 65536, 1000),
                (100, 2, 0), (100, 2, (1 << 20) + 1)):
        assert L.fgr_ransac_workspace(*bad, nb) == -1, bad
        assert b'fgr_ransac_workspace' in L.fgr_last_error()
    assert L.fgr_ransac_workspace(100, 2, 1000, None) == -1
    assert L.fgr_ransac_workspace(0, 1, 1, nb) == 0 and L.fgr_ransac_workspace(100, 65535, 1 << 20, nb) == 0

    host = (ctypes.c_char * 4096)()
    ptr = (ctypes.addressof(host) + 255) & ~255            # never dereferenced
    good = dict(a=ptr, b=ptr, w=None, n_tot=100, off=ptr, n_pairs=2, w_min=f(0.0),
                inlier_dist=f(0.1), n_hyp=1000, seed=0, n_refits=4, ws=ptr, ws_bytes=need,
                pose=ptr, n_inliers=ptr, inlier_rmse=ptr, n_eligible=ptr, best_hyp=ptr,
                n_updates=ptr, inlier_mask=None, hyp_pose=None, hyp_count=None, stream=None)
    cases = [dict(n_pairs=0), dict(n_pairs=65536), dict(n_hyp=0), dict(n_hyp=(1 << 20) + 1),
             dict(n_refits=-1), dict(inlier_dist=f(0.0)), dict(inlier_dist=f(-1.0)),
             dict(inlier_dist=f(float('nan'))), dict(inlier_dist=f(float('inf'))),
             dict(n_tot=-1), dict(n_tot=1 << 31), dict(ws_bytes=need - 1), dict(ws_bytes=0)]
    cases += [{k: None} for k in ('a', 'b', 'off', 'ws', 'pose', 'n_inliers', 'inlier_rmse',
                                  'n_eligible', 'best_hyp', 'n_updates')]
    for case in cases:
        rc = L.fgr_ransac_pose(*{**good, **case}.values())
        assert rc == -1, (case, rc)
        assert b'fgr_ransac_pose' in L.fgr_last_error(), (case, L.fgr_last_error())
    rc = L.fgr_ransac_pose(*{**good, 'ws_bytes': need - 1}.values())
    assert rc == -1 and b'fgr_ransac_pose: workspace' in L.fgr_last_error()
