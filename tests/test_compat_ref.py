"""CPU: pins tests/_compat_ref.py, the numpy restatement that tests/test_gpu_compat.py holds the
spatial-compatibility kernels to -- the bit matrix, c and s against a dense integer S @ S, the
symmetry, the tie rules, invalid seeds, the planted recovery at 3, 5 and 10 % inliers before and
after the refits, the margins of the inputs the GPU test compares exactly -- and the argument
checks of fgr_compat_pose / fgr_compat_workspace, which need no GPU."""
import ctypes
import functools

import numpy as np
import pytest

import _compat_ref as cr
import _ransac_ref as rr

# the planted inputs: 600 rows in a unit cube, noise sigma 0.005, both distances 0.03
PROTO_M, PROTO_SIGMA, PROTO_DIST, PROTO_SEEDS, PROTO_K = 600, 0.005, 0.03, 32, 16
PROTO = [(pct, n) for pct in (3, 5, 10) for n in range(4)]
SHAPE_M = (0, 1, 2, 3, 63, 64, 65, 129, 300)
SHAPE_DIST, SHAPE_SEEDS, SHAPE_K = 0.05, 8, 6
# a refit-loop comparison needs every row's d2 at least this far (relative) from r2, as
# test_gpu_ransac.py; a first-order bit needs | |la - lb| - compat_dist | of at least one fp32
# ulp of compat_dist (both sides run the same correctly rounded fp32 operations, so any margin
# above zero keeps the bits equal; one ulp also covers a last-bit difference in a square root)
D2_MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def proto_problem(pct, n):
    return cr.planted_unit(10 * pct + n, PROTO_M, pct / 100.0, PROTO_SIGMA, PROTO_DIST)


@functools.lru_cache(maxsize=None)
def proto_reference(pct, n, n_refits=4):
    a, b, _, _ = proto_problem(pct, n)
    return cr.compat(a, b, None, PROTO_DIST, PROTO_DIST, PROTO_SEEDS, PROTO_K, n_refits)


@functools.lru_cache(maxsize=None)
def shape_problem(m):
    """Half planted, so that both dense and sparse rows of bits occur."""
    if m == 0:
        z = np.zeros((0, 3), np.float32)
        return z, z.copy()
    a, b, _, _ = cr.planted_unit(200 + m, m, 0.5, PROTO_SIGMA, SHAPE_DIST)
    return a, b


def sc_margin(a, b, compat_dist):
    g = cr.length_gaps(a, b).astype(np.float64)
    off = ~np.eye(len(g), dtype=bool)
    return float(np.abs(g[off] - float(np.float32(compat_dist))).min()) if off.any() else np.inf


def _dense(S):
    Si = S.astype(np.int64)
    c = Si @ Si
    return c, (Si * c).sum(1)


@pytest.mark.parametrize('m', SHAPE_M)
def test_bits_c_and_s_match_the_dense_product(m):
    a, b = shape_problem(m)
    S = cr.first_order(a, b, SHAPE_DIST)
    bits = cr.pack_bits(S)
    assert bits.shape == (m, (m + 63) // 64) and bits.dtype == np.uint64
    c, s = cr.second_order(bits)
    cd, sd = _dense(S)
    assert np.array_equal(c, cd) and np.array_equal(s, sd) and s.dtype == np.int32
    if m:
        # every bit where it belongs, none past m
        j = np.arange(bits.shape[1] * 64)
        back = ((bits[:, j // 64] >> (j % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)
        assert np.array_equal(back[:, :m], S) and not back[:, m:].any()
    if m >= 63:
        assert S.any() and not S.all() and s.max() > 0


def test_first_order_is_symmetric_strict_and_nan_free():
    a, b = shape_problem(129)
    S = cr.first_order(a, b, SHAPE_DIST)
    assert np.array_equal(S, S.T) and not S.diagonal().any()
    la, lb = cr.lengths32(a), cr.lengths32(b)
    assert np.array_equal(la, la.T) and la.dtype == np.float32
    # strict: a pair exactly at the distance is not compatible
    p = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    q = np.array([[0, 0, 0], [1.5, 0, 0]], np.float32)
    assert not cr.first_order(p, q, 0.5).any() and cr.first_order(p, q, 0.5000001)[0, 1]
    # a NaN coordinate makes its row and column 0
    a2 = a.copy()
    a2[7, 1] = np.nan
    S2 = cr.first_order(a2, b, SHAPE_DIST)
    assert not S2[7].any() and not S2[:, 7].any()
    keep = np.arange(129) != 7
    assert np.array_equal(S2[keep][:, keep], S[keep][:, keep])


def test_tie_rules():
    assert cr.seed_ranks([5, 9, 9, 1, 9], 3).tolist() == [1, 2, 4]
    assert cr.seed_ranks([5, 9, 9, 1, 9], 10).tolist() == [1, 2, 4, 0, 3]
    assert cr.seed_ranks([0, 0, 0], 2).tolist() == [0, 1]
    S = np.ones((6, 6), bool)
    np.fill_diagonal(S, False)
    S[0, 5] = S[5, 0] = False
    c = np.zeros((6, 6), np.int64)
    c[2] = [4, 7, 0, 7, 4, 4]
    assert cr.consensus(S, c, 2, 4).tolist() == [0, 1, 2, 3]        # 7, 7, then the lowest 4
    assert cr.consensus(S, c, 2, 3).tolist() == [1, 2, 3]
    assert cr.consensus(S, c, 2, 16).tolist() == [0, 1, 2, 3, 4, 5]  # k above the neighbourhood
    assert cr.consensus(S, c, 0, 16).tolist() == [0, 1, 2, 3, 4]     # 5 is not compatible with 0
    # duplicate rows: every score ties, the seeds are the lowest ranks in order
    base = np.random.default_rng(3).uniform(0, 1, (5, 3)).astype(np.float32)
    a = np.tile(base, (4, 1))
    out = cr.compat(a, a + np.float32(0.25), None, 0.01, 0.01, n_seeds=7, k=4, n_refits=0)
    assert len(set(out['row_score'].tolist())) == 1 and out['seed_row'].tolist() == list(range(7))
    assert out['members'][0].tolist() == [0, 1, 2, 3] and out['best_seed'] == 0
    assert out['n_inliers'] == 20


def test_invalid_seeds():
    rng = np.random.default_rng(4)
    for m in (0, 1, 2):
        a = rng.uniform(0, 1, (m, 3)).astype(np.float32)
        out = cr.compat(a, a, None, 0.05, 0.05, n_seeds=4)
        assert out['best_seed'] == -1 and (out['seed_count'] == -1).all() and out['n_eligible'] == m
        assert out['seed_row'].tolist() == list(range(m)) + [-1] * (4 - m)
        assert np.array_equal(out['pose'], cr.EYE) and out['n_inliers'] == 0 and out['rmse'] == 0.0
        assert np.array_equal(out['seed_pose'], np.tile(cr.EYE, (4, 1, 1))) and not out['mask'].any()
    # no compatible rows: b stretches every length by 3
    a = rng.uniform(0, 1, (40, 3)).astype(np.float32)
    out = cr.compat(a, 3 * a, None, 1e-4, 0.05, n_seeds=8)
    assert (out['row_score'] == 0).all() and out['best_seed'] == -1
    assert out['seed_row'].tolist() == list(range(8)) and (out['seed_count'] == -1).all()
    # one compatible partner only: two members, still invalid
    b = 3 * a
    b[:2] = a[:2]
    out = cr.compat(a, b, None, 1e-4, 0.05, n_seeds=8)
    assert out['best_seed'] == -1 and out['row_score'][:2].tolist() == [0, 0]
    # weights: ineligible rows score -1 and are never seeds
    w = np.ones(40, np.float32)
    w[[3, 9]] = 0.0
    w[5] = np.nan
    out = cr.compat(a, a, w, 0.05, 0.05, n_seeds=40)
    assert out['n_eligible'] == 37 and (out['row_score'][[3, 5, 9]] == -1).all()
    assert set(out['seed_row'][:37].tolist()) == set(range(40)) - {3, 5, 9}
    assert (out['seed_row'][37:] == -1).all() and not out['mask'][[3, 5, 9]].any()


@pytest.mark.parametrize('pct,n', PROTO)
def test_planted_recovery(pct, n):
    """Every planted row in the mask, rotation within 1 degree and translation within 0.02, of
    the winning seed's pose before any refit and of the refitted pose."""
    a, b, truth, planted = proto_problem(pct, n)
    assert planted.sum() == round(PROTO_M * pct / 100)
    out = proto_reference(pct, n)
    T0, c0 = out['first']
    assert out['best_seed'] >= 0
    before = rr.d2_rows(T0, a, b) < rr.r2_of(PROTO_DIST)
    for what, T, mask in (('before', T0, before), ('after', out['pose'], out['mask'])):
        rot, tr = cr.pose_errors(T, truth)
        print(f'{pct} % input {n} {what}: rot {rot:.3f} deg, trans {tr:.4f}, inliers {mask.sum()} '
              f'planted {planted.sum()}')
        assert mask[planted].all(), (what, np.flatnonzero(planted & ~mask))
        assert rot < 1.0 and tr < 0.02, (what, rot, tr)
    assert c0 == before.sum() and out['n_inliers'] == out['mask'].sum() >= c0


def test_margins_of_the_exactly_compared_inputs():
    """The inputs tests/test_gpu_compat.py compares discretely: no length difference within one
    fp32 ulp of compat_dist, and no row of a pose the refit loop scores within D2_MARGIN of r2."""
    for pct, n in PROTO:
        a, b, _, _ = proto_problem(pct, n)
        assert sc_margin(a, b, PROTO_DIST) >= np.spacing(np.float32(PROTO_DIST)), (pct, n)
        out = proto_reference(pct, n)
        assert min(out['gaps']) >= D2_MARGIN, (pct, n, out['gaps'])
    for m in SHAPE_M:
        a, b = shape_problem(m)
        assert sc_margin(a, b, SHAPE_DIST) >= np.spacing(np.float32(SHAPE_DIST)), m
        out = cr.compat(a, b, None, SHAPE_DIST, SHAPE_DIST, SHAPE_SEEDS, SHAPE_K)
        assert out['best_seed'] >= 0 or m < 63            # m = 3 plants two rows: no valid seed
        if out['best_seed'] >= 0:
            assert min(out['gaps']) >= D2_MARGIN, (m, out['gaps'])


def _lib():
    import fgreg
    return fgreg.load()


def bad_arguments(need, ptr):
    """(good, cases): the arguments of a valid call and every refused variation of it."""
    f = ctypes.c_float
    good = dict(a=ptr, b=ptr, w=None, n_tot=100, off=ptr, n_pairs=2, max_len=60, w_min=f(0.0),
                compat_dist=f(0.1), inlier_dist=f(0.1), n_seeds=16, k=8, n_refits=4, ws=ptr,
                ws_bytes=need, pose=ptr, n_inliers=ptr, inlier_rmse=ptr, n_eligible=ptr,
                best_seed=ptr, n_updates=ptr, inlier_mask=None, row_score=None, seed_row=None,
                seed_pose=None, seed_count=None, stream=None)
    cases = [dict(n_pairs=0), dict(n_pairs=65536), dict(n_tot=-1), dict(n_tot=1 << 31),
             dict(max_len=-1), dict(max_len=8193), dict(n_seeds=0), dict(n_seeds=1025),
             dict(k=2), dict(k=257), dict(n_refits=-1), dict(ws_bytes=need - 1), dict(ws_bytes=0),
             dict(ws=ptr + 8)]
    for key in ('compat_dist', 'inlier_dist'):
        cases += [{key: f(v)} for v in (0.0, -1.0, float('nan'), float('inf'))]
    cases += [{key: None} for key in ('a', 'b', 'off', 'ws', 'pose', 'n_inliers', 'inlier_rmse',
                                      'n_eligible', 'best_seed', 'n_updates')]
    return good, cases


def test_compat_argument_errors_need_no_gpu():
    """Every refusal is FGR_E_ARG (-1) with the entry point's name in fgr_last_error(), before
    anything is launched: the pointers here are host addresses that are never read."""
    L = _lib()
    nb = ctypes.c_size_t(0)
    assert L.fgr_compat_workspace(100, 2, 60, 16, nb) == 0 and nb.value > 0
    need = nb.value
    for bad in ((-1, 2, 60, 16), (1 << 31, 2, 60, 16), (100, 0, 60, 16), (100, 65536, 60, 16),
                (100, 2, -1, 16), (100, 2, 8193, 16), (100, 2, 60, 0), (100, 2, 60, 1025)):
        assert L.fgr_compat_workspace(*bad, nb) == -1, bad
        assert b'fgr_compat_workspace' in L.fgr_last_error()
    assert L.fgr_compat_workspace(100, 2, 60, 16, None) == -1
    assert L.fgr_compat_workspace(0, 1, 0, 1, nb) == 0
    assert L.fgr_compat_workspace(100000, 65535, 8192, 1024, nb) == 0
    # a function of its four arguments only, growing with each
    for more in ((101, 2, 60, 16), (100, 3, 60, 16), (100, 2, 8192, 16), (100, 2, 60, 1024)):
        assert L.fgr_compat_workspace(*more, nb) == 0 and nb.value >= need, more
    host = (ctypes.c_char * 4096)()
    ptr = (ctypes.addressof(host) + 255) & ~255            # never dereferenced
    good, cases = bad_arguments(need, ptr)
    for case in cases:
        rc = L.fgr_compat_pose(*{**good, **case}.values())
        assert rc == -1, (case, rc)
        assert b'fgr_compat_pose' in L.fgr_last_error(), (case, L.fgr_last_error())
    rc = L.fgr_compat_pose(*{**good, 'ws_bytes': need - 1}.values())
    assert rc == -1 and b'fgr_compat_pose: workspace' in L.fgr_last_error()
