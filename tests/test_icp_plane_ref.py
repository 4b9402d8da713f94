"""CPU: the numpy restatement tests/_icp_plane_ref.py (the reference of the GPU tests of
fgr_estimate_normals and fgr_icp_plane) against analytic answers, and the conditions the GPU
tests rely on, asserted on the restatement alone: the normals inputs are mostly comparable, the
whole-loop seeds stay away from a different discrete result, the benefit seeds show the benefit.
"""
import functools

import numpy as np
import pytest

import _icp_plane_ref as pr
import _icp_ref as ir

F32 = np.float32


# ---------------------------------------------------------------------------------------------
# normals
# ---------------------------------------------------------------------------------------------
def test_normals_of_an_exact_plane():
    """z = 0.5 exactly: every d has dz = 0, so the covariance's z row is exactly 0 and the
    normal is (0, 0, -1) towards the origin, (0, 0, 1) towards a viewpoint above. A tilted plane
    is exact up to the fp32 rounding of its coordinates (2^-24 * 2 off the plane over a
    neighbourhood 0.3 wide: 1e-6)."""
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.uniform(0, 1, (200, 2)), np.full((200, 1), 0.5)], 1).astype(F32)
    ref = pr.normals(pts, 0.3)
    assert ref['valid'].all() and (ref['count'] >= 3).all()
    assert np.abs(ref['normals'] - [0, 0, -1]).max() <= 1e-12
    up = pr.normals(pts, 0.3, view=[0.5, 0.5, 3.0])
    assert np.abs(up['normals'] - [0, 0, 1]).max() <= 1e-12
    R = ir.rotation([1, 2, 3], 40.0)
    tilted = (pts.astype(np.float64) @ R.T).astype(F32)
    want = -R[:, 2] if (R[:, 2] @ -tilted[0]) < 0 else R[:, 2]
    assert np.abs(pr.normals(tilted, 0.3)['normals'] - want).max() <= 2e-6


def test_normals_of_a_sphere_within_the_curvature_bound():
    """Points on a sphere of radius R about c: a neighbour at chord d <= rho lies |d|^2 / (2 R)
    <= h = rho^2 / (2 R) below the tangent plane, so the variance along the radial direction u
    is <= h^2 / 4. With n the eigenvector of l0 and u = cos(t) n + sin(t) m,
    var(u) >= sin(t)^2 l1, hence sin(t) <= h / (2 sqrt(l1))."""
    rng = np.random.default_rng(1)
    R, rho, c = 1.0, 0.3, np.array([0.2, -0.1, 3.0])
    u = rng.normal(size=(1500, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pts = (c + R * u).astype(F32)
    ref = pr.normals(pts, rho, view=c)                      # inward: -u
    assert ref['valid'].all() and (ref['count'] >= 5).all()
    radial = (c - pts.astype(np.float64))
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    sin_t = np.linalg.norm(np.cross(ref['normals'].astype(np.float64), radial), axis=1)
    bound = rho ** 2 / (2 * R) / (2 * np.sqrt(ref['evals'][:, 1])) + 1e-6
    assert (sin_t <= bound).all(), float((sin_t / bound).max())
    assert ((ref['normals'] * radial).sum(1) > 0).all()


def test_normals_sign_rule_and_validity():
    rng = np.random.default_rng(2)
    pts = pr.patch(120, 9)
    view = np.array([0.1, 0.2, 6.0], F32)           # beyond the patch, seen from the origin
    a, b = pr.normals(pts, 0.4), pr.normals(pts, 0.4, view=view)
    assert a['valid'].all()
    assert ((a['normals'] * -pts).sum(1) > 0).all()
    assert ((b['normals'] * (view - pts)).sum(1) > 0).all()
    assert np.array_equal(a['normals'], -b['normals'])      # the other side: the same bits, flipped
    assert np.abs(np.linalg.norm(a['normals'].astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22
    # n . (view - p) exactly 0: the plane z = 0 through the viewpoint -> first non-zero positive
    flat = np.concatenate([rng.uniform(-1, 1, (50, 2)), np.zeros((50, 1))], 1).astype(F32)
    assert np.array_equal(pr.normals(flat, 0.8)['normals'], np.tile(F32([0, 0, 1]), (50, 1)))
    # fewer than 3 neighbours: zero and invalid
    iso = pr.normals_cases()['isolated'][0][0]
    ref = pr.normals(iso, 0.4)
    assert ref['count'][17] == 1 and (ref['count'][18:20] == 2).all()
    assert not ref['valid'][17:20].any() and not ref['normals'][17:20].any()
    assert ref['valid'].sum() == len(iso) - 3


@pytest.mark.parametrize('name', list(pr.normals_cases()))
def test_normals_cases_are_comparable(name):
    """The condition of the GPU comparison: >= 90 % of every cloud's valid normals pass the
    eigen-gap and sign-margin filter, so the filter cannot hide a failure."""
    clouds, radius, view = pr.normals_cases()[name]
    for c, cloud in enumerate(clouds):
        ref = pr.normals(cloud, radius, None if view is None else view[c])
        n_valid = int(ref['valid'].sum())
        assert n_valid == (0 if len(cloud) < 3 else n_valid)
        if n_valid:
            assert pr.comparable(ref).sum() >= 0.9 * n_valid, (name, c)
    if name.startswith('lattice'):
        med = np.median(pr.normals(clouds[0], radius)['count'])
        assert (4 <= med <= 8) if radius < 0.2 else (35 <= med <= 45)


# ---------------------------------------------------------------------------------------------
# point-to-plane ICP
# ---------------------------------------------------------------------------------------------
def test_terms_match_the_definition():
    src, tgt, pose0, _, r = pr.room_problem(1, 300, 40)
    nrm = pr.normals(tgt, 0.15)['normals']
    nrm[::7] = 0                                            # zero normals mixed in
    idx0, d2, _ = pr.associate(src, tgt, pose0, r)
    idx = pr.inliers(idx0, nrm)
    assert (idx0 >= 0).sum() > (idx >= 0).sum() > 10
    n, sd2, srho2, A, g = pr.terms(src, tgt, nrm, pose0, idx, d2)
    q = pr.transform32(pose0, src).astype(np.float64)
    A2, g2, s2 = np.zeros((6, 6)), np.zeros(6), 0.0
    for i in np.flatnonzero(idx >= 0):
        nn, s = nrm[idx[i]].astype(np.float64), tgt[idx[i]].astype(np.float64)
        J = np.concatenate([nn, np.cross(q[i], nn)])
        rho = nn @ (q[i] - s)
        A2 += np.outer(J, J)
        g2 += J * rho
        s2 += rho * rho
    assert n == (idx >= 0).sum() and np.allclose(A, A2, rtol=1e-12, atol=1e-14)
    assert np.allclose(g, g2, rtol=1e-12, atol=1e-14) and np.isclose(srho2, s2, rtol=1e-12)
    # the update is the Gauss-Newton step: it lowers the linearised plane residual
    st = pr.step(src, tgt, nrm, pose0, idx, d2)
    assert st['status'] is None
    _, _, after, _, _ = pr.terms(src, tgt, nrm, st['pose'].astype(F32), idx, d2)
    assert after < 0.2 * srho2
    # dR is orthogonal in fp64; pose0's entries were rounded to fp32 (<= 2^-25 each, 3 terms, twice)
    R = st['pose'][:, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() <= 6 * 2.0 ** -25


def test_plane_only_stops_as_singular():
    src, tgt, nrm, pose0, r = pr.plane_only(0)
    out = pr.icp_plane(src, tgt, nrm, pose0, r)
    assert out['status'] == pr.SINGULAR and out['n_iters'] == 0
    assert np.array_equal(out['pose'], pose0) and out['fitness'] == 1.0
    assert np.isclose(out['plane_rmse'], 0.01, rtol=1e-5) and out['rmse'] >= out['plane_rmse']
    assert np.linalg.matrix_rank(out['info']) == 3 and out['info'][0, 0] == 0
    # two parallel planes are singular too
    tgt2 = np.concatenate([tgt, tgt + F32([0, 0, 0.5])])
    src2 = np.concatenate([src, src + F32([0, 0, 0.5])])
    assert pr.icp_plane(src2, tgt2, np.concatenate([nrm, nrm]), pose0, r)['status'] == pr.SINGULAR
    assert (pr.CONVERGED, pr.MAX_ITERS, pr.FEW_INLIERS, pr.SINGULAR) == (0, 1, 2, 3)
    few = pr.icp_plane(src[:5], tgt, nrm, pose0, r)
    assert few['status'] == pr.FEW_INLIERS and few['n_iters'] == 0


@functools.lru_cache(maxsize=None)
def _loop(seed):
    src, tgt, pose0, truth, r = pr.room_problem(seed, *pr.LOOP_SIZES)
    nrm = pr.normals(tgt, pr.LOOP_NORMAL_RADIUS)['normals']
    return src, tgt, nrm, pose0, truth, r, pr.icp_plane(src, tgt, nrm, pose0, r)


@pytest.mark.parametrize('seed', pr.LOOP_SEEDS)
def test_room_loop_converges_away_from_discrete_changes(seed):
    src, tgt, nrm, pose0, truth, r, out = _loop(seed)
    assert out['status'] == pr.CONVERGED and 3 <= out['n_iters'] <= 8
    assert np.min(out['gaps']) >= 4e-5 * r, out['gaps']
    rot, trans = pr.pose_errors(out['pose'], truth)
    rot0, trans0 = pr.pose_errors(pose0, truth)
    assert abs(rot0 - 4.0) < 1e-3 and rot < 0.6 and trans < 0.005 and trans < trans0
    assert np.linalg.cond(out['info']) < 100                # the issue's experiment saw 45
    assert out['fitness'] > 0.95 and out['plane_rmse'] < out['rmse']


@pytest.mark.parametrize('seed', pr.BENEFIT_SEEDS)
def test_benefit_seeds_show_a_factor_of_four(seed):
    """After 10 updates from the same start, the point-to-plane error is at most a quarter of
    the point-to-point one, in rotation and in translation (the GPU test asserts a third)."""
    src, tgt, pose0, truth, r = pr.room_problem(seed)
    nrm = pr.normals(tgt, pr.ROOM_NORMAL_RADIUS)['normals']
    plane = pr.pose_errors(pr.icp_plane(src, tgt, nrm, pose0, r, max_iters=10)['pose'], truth)
    point = pr.pose_errors(ir.icp(src, tgt, pose0, r, max_iters=10)['pose'], truth)
    print(f'seed {seed}: plane {plane} point {point}')
    assert 4 * plane[0] <= point[0] and 4 * plane[1] <= point[1]
