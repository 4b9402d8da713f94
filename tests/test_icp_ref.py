"""CPU: pins tests/_icp_ref.py, the numpy restatement that tests/test_gpu_icp.py holds the ICP
kernels to -- against a known pose, scipy's k-d tree and the information matrix's definition."""
import numpy as np
from scipy.spatial import cKDTree

import _icp_ref as ir


def _cloud(rng, n):
    return rng.uniform(-1.0, 1.0, (n, 3))


def test_noise_free_pair_converges_to_the_known_pose():
    rng = np.random.default_rng(0)
    tgt = _cloud(rng, 400)
    R = ir.rotation([0.3, -1.0, 0.5], 5.0)
    t = np.array([0.02, -0.03, 0.01])
    src = (tgt - t) @ R                                    # R src + t = tgt
    pose0 = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    out = ir.icp(src, tgt, pose0, 0.3, max_iters=50)
    want = np.concatenate([R, t[:, None]], 1)
    assert out['fitness'] == 1.0 and 1 <= out['n_iters'] < 50
    assert np.abs(out['pose'] - want).max() < 1e-6, np.abs(out['pose'] - want).max()
    assert out['rmse'] < 1e-6
    assert np.array_equal(out['idx'], np.arange(400))


def test_nearest_neighbours_match_ckdtree():
    rng = np.random.default_rng(1)
    src, tgt = _cloud(rng, 700).astype(np.float32), _cloud(rng, 900).astype(np.float32)
    pose = np.concatenate([ir.rotation([1, 2, 3], 20.0), [[0.1], [-0.2], [0.05]]], 1).astype(np.float32)
    r = 0.15
    idx, d2, (gap_nn, gap_r) = ir.associate(src, tgt, pose, r)
    assert gap_nn > 1e-6 and gap_r > 1e-6                  # no ties: the answer is unique
    q = ir.transform32(pose, src).astype(np.float64)
    dist, j = cKDTree(tgt.astype(np.float64)).query(q)
    inl = dist < r
    assert 100 < inl.sum() < 700
    assert np.array_equal(idx, np.where(inl, j, -1))
    assert np.allclose(d2[inl], dist[inl] ** 2, rtol=1e-5, atol=0)
    assert np.isinf(d2[~inl]).all()


def test_ties_go_to_the_lowest_index_and_the_radius_is_strict():
    tgt = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 0], [0.5, 0, 0]], np.float32)
    src = np.array([[0, 0, 0], [0.25, 0, 0], [-0.5, 0, 0]], np.float32)
    eye = np.eye(3, 4, dtype=np.float32)
    idx, d2, (gap_nn, _) = ir.associate(src, tgt, eye, 0.5)
    assert idx.tolist() == [1, 1, -1] and gap_nn == 0.0    # duplicates, a midpoint, d2 == r2
    assert d2[0] == 0 and d2[1] == np.float32(0.0625) and np.isinf(d2[2])


def test_information_matches_the_per_point_loop():
    rng = np.random.default_rng(2)
    tgt = _cloud(rng, 50) * 3
    idx = rng.integers(-1, 50, 80).astype(np.int32)
    G, ref = ir.information(tgt, idx), ir.information_loop(tgt, idx)
    n = int((idx >= 0).sum())
    assert np.abs(G - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(G, G.T)
    assert np.array_equal(G[:3, :3], n * np.eye(3)) and G[0, 0] == n


def test_state_machine_corner_cases():
    eye = np.eye(3, 4, dtype=np.float32)
    far = ir.icp(np.zeros((5, 3)), np.full((5, 3), 10.0), eye, 1.0)
    assert far['n_iters'] == 0 and far['fitness'] == 0.0 and far['rmse'] == 0.0
    assert np.array_equal(far['pose'], eye) and len(far['gaps']) == 1
    empty = ir.icp(np.zeros((0, 3)), np.zeros((4, 3)), eye, 1.0)
    assert empty['n_iters'] == 0 and empty['fitness'] == 0.0
    src = np.array([[0, 0, 0], [1, 0, 0], [50, 0, 0]], np.float32)
    two = ir.icp(src, src[:2] + np.float32(0.01), eye, 0.1)
    assert two['n_iters'] == 0 and two['fitness'] == 2 / 3 and np.array_equal(two['pose'], eye)
    rng = np.random.default_rng(3)
    tgt = _cloud(rng, 300)
    capped = ir.icp(tgt @ ir.rotation([0, 0, 1], 3.0).T, tgt, eye, 0.3, max_iters=2)
    assert capped['n_iters'] == 2 and len(capped['gaps']) == 3


def test_loop_problem_meets_its_precondition():
    """The whole-loop inputs of test_gpu_icp.py: 4 to 8 updates, and no pass closer than
    1e-5 r to another discrete result."""
    for seed in (5, 7, 10, 15, 17, 30):
        src, tgt, pose0, r = ir.loop_problem(seed)
        out = ir.icp(src, tgt, pose0, r)
        assert 4 <= out['n_iters'] <= 8 and out['fitness'] == 1.0
        assert np.min(out['gaps']) >= 1e-5 * r
