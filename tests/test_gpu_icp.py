"""The ICP kernels (csrc/icp.hip: fgr_icp, fgr_registration_score) against the numpy restatement
tests/_icp_ref.py (pinned on the CPU by tests/test_icp_ref.py), through the C ABI with every
operand carved out of a guarded arena (tests/_arena.py) -- each call runs on a clean and on a
poisoned arena with bit-identical results and the workspace is exactly fgr_icp_workspace bytes
-- and through fgreg.refine.

Discrete results are compared exactly: idx, d2 (the same fp32 operations in the same order on
both sides), the inlier count, fitness (n / n_src in fp64, rounded once), n_iters, the poses
that must come back unchanged. Values are compared at BOUNDS: worst |got - ref| / max(1, |ref|)
measured on the MI355X against the fp64 restatement fed the kernel's own correspondences, times
<= 4, never looser than 1e-4 for the pose (the family's ceiling, test_gpu_tail_kernels.py) or
1e-10 for the fp64 information matrix. The pose error is |dR| absolute and |dt| / max(1, max|t|).

  family                                         measured   asserted   ceiling
  pose   one solve (60 m lidar pair, mirrored,
         coplanar) and the whole loop            2.98e-08   1.1e-07    1e-4
  rmse   fp64 sqrt(sum d2 / n) stored as fp32    1.48e-08   5.5e-08    1e-4
  info   fp64 sums in block order vs numpy's     4.88e-15   1.9e-14    1e-10

The whole-loop inputs (_icp_ref.loop_problem) are the seeds for which the restatement alone, on
the CPU, takes 4 to 8 updates with every pass at least 2e-5 r away from a different discrete
result (second-nearest minus nearest d2, |d2 - r2|); the test asserts >= 1e-5 r first. The
device's pose differs from numpy's by fp32 rounding of an fp64 solve (1e-7 on coordinates
<= 1), far inside that gap, so n_iters and the final associations must be equal (measured: the
six final poses are bit-equal to the restatement's).
"""
import functools

import numpy as np
import pytest
import torch

import _icp_ref as ir
from _arena import SENTINEL, Arena, assert_both_equal, bit_equal, run_both

pytestmark = pytest.mark.gpu
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
EYE = np.eye(3, 4, dtype=np.float32)

BOUNDS = {'pose': 1.1e-7, 'rmse': 5.5e-8, 'info': 1.9e-14}


def _check(family, err, what=''):
    """Prints the figure (the measurement), then asserts it."""
    err = float(err)
    print(f'MEASURE {family} {err:.3e} bound {BOUNDS[family]:.1e} {what}')
    assert err <= BOUNDS[family], (family, what, err, BOUNDS[family])


def _relmax(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()) if ref.size else 0.0


def _pose_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return max(float(np.abs(got[..., :3] - ref[..., :3]).max()),
               float(np.abs(got[..., 3] - ref[..., 3]).max()) / max(1.0, float(np.abs(ref[..., 3]).max())))


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


def _need(ns, nt, B):
    from fgreg import _lib
    nb = _lib._sz(0)
    _ok(_L().fgr_icp_workspace(ns, nt, B, nb), 'fgr_icp_workspace')
    return nb.value


def _both(fn, gpu):
    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    return tuple(t.cpu().numpy() for t in clean)


class _Geo:
    """The packed geometry of a call and its operands inside an arena."""

    def __init__(self, srcs, tgts, poses):
        self.src, self.so = ir.pack(srcs)
        self.tgt, self.to = ir.pack(tgts)
        self.B = len(srcs)
        self.ns, self.nt = len(self.src), len(self.tgt)
        self.max_len = max(len(s) for s in srcs)
        self.pose = np.asarray(poses, np.float32).reshape(self.B, 12)
        self.need = _need(self.ns, self.nt, self.B)
        assert self.ns > 0 and self.nt > 0

    def put(self, ar):
        self.d = [ar.put(_t(self.src), name='src'), ar.put(_t(self.so), name='src_off'),
                  ar.put(_t(self.tgt), name='tgt'), ar.put(_t(self.to), name='tgt_off'),
                  ar.put(_t(self.pose), name='pose')]
        self.ws = ar.bytes(self.need, name='ws')

    def args(self):
        s, so, t, to, _ = self.d
        return (_p(s), _p(so), self.ns, _p(t), _p(to), self.nt, self.B, self.max_len)


def _score(gpu, srcs, tgts, poses, r):
    """fgr_registration_score with every output -> fitness, rmse, idx, d2, info (numpy)."""
    g = _Geo(srcs, tgts, poses)

    def fn(ar):
        g.put(ar)
        f, e = ar.vector(g.B, F32, 'out', 'fitness'), ar.vector(g.B, F32, 'out', 'rmse')
        idx, d2 = ar.vector(g.ns, I32, 'out', 'idx'), ar.vector(g.ns, F32, 'out', 'd2')
        info = ar.matrix(g.B, 36, 36, F64, 'out', 'info')
        _ok(_L().fgr_registration_score(*g.args(), _p(g.d[4]), r, _p(g.ws), g.need, _p(f), _p(e),
                                        _p(idx), _p(d2), _p(info), _st()), 'fgr_registration_score')
        return f, e, idx, d2, info

    f, e, idx, d2, info = _both(fn, gpu)
    return f, e, idx, d2, info.reshape(g.B, 6, 6)


def _icp(gpu, srcs, tgts, poses, r, max_iters=30, rel_f=1e-6, rel_e=1e-6):
    """fgr_icp -> pose (B, 3, 4), fitness, rmse, n_iters (numpy)."""
    g = _Geo(srcs, tgts, poses)

    def fn(ar):
        g.put(ar)
        po = ar.matrix(g.B, 12, 12, F32, 'out', 'pose_out')
        f, e = ar.vector(g.B, F32, 'out', 'fitness'), ar.vector(g.B, F32, 'out', 'rmse')
        it = ar.vector(g.B, I32, 'out', 'n_iters')
        _ok(_L().fgr_icp(*g.args(), _p(g.d[4]), r, max_iters, rel_f, rel_e, _p(g.ws), g.need,
                         _p(po), _p(f), _p(e), _p(it), _st()), 'fgr_icp')
        return po, f, e, it

    po, f, e, it = _both(fn, gpu)
    return po.reshape(g.B, 3, 4), f, e, it


def _assert_association(gpu, srcs, tgts, poses, r, what=''):
    """idx, d2, inlier count and fitness bit for bit against the restatement; rmse and info at
    their bounds. -> the restatement's per-pair (idx, d2, gaps)."""
    f, e, idx, d2, info = _score(gpu, srcs, tgts, poses, r)
    so = ir.offsets([len(s) for s in srcs])
    refs = []
    for b, (s, t) in enumerate(zip(srcs, tgts)):
        ri, rd, gaps = ir.associate(s, t, poses[b], r)
        gi, gd = idx[so[b]:so[b + 1]], d2[so[b]:so[b + 1]]
        assert np.array_equal(gi, ri), (what, b, np.flatnonzero(gi != ri)[:5])
        assert np.array_equal(gd.view(np.uint32), rd.view(np.uint32)), (what, b)
        n, _, _, _, sd = ir.moments(s, t, ri, rd)
        rf, re = ir.fitness_rmse(n, sd, len(s))
        assert f[b] == np.float32(rf) and info[b, 0, 0] == n, (what, b, f[b], rf, info[b, 0, 0], n)
        _check('rmse', _relmax(e[b:b + 1], [re]), f'{what} pair {b}')
        assert (e[b] == 0) == (n == 0)
        _check('info', _relmax(info[b], ir.information(t, ri)), f'{what} pair {b}')
        assert np.array_equal(info[b], info[b].T)
        refs.append((ri, rd, gaps))
    return refs


def _pose(rng, deg=10.0, trans=0.05):
    R = ir.rotation(rng.normal(size=3), deg)
    return np.concatenate([R, rng.uniform(-trans, trans, (3, 1))], 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# association, exact
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_tgt', [1, 2, 1000])
@pytest.mark.parametrize('n_src', [1, 63, 64, 65, 255, 256, 257, 1000])
def test_association_sizes(gpu, n_src, n_tgt):
    rng = np.random.default_rng(1000 * n_src + n_tgt)
    tgt = rng.uniform(0, 1, (n_tgt, 3)).astype(np.float32)
    src = rng.uniform(0, 1, (n_src, 3)).astype(np.float32)
    src[0] = tgt[0] + np.float32(0.01)                     # always an inlier near the first target
    r = 0.06 if n_tgt == 1000 else 0.4
    (ri, _, _), = _assert_association(gpu, [src], [tgt], [EYE], r, f'{n_src}x{n_tgt} identity')
    assert (ri >= 0).any() and (n_src < 63 or (ri < 0).any())       # inliers and outliers
    _assert_association(gpu, [src], [tgt], [_pose(rng)], r, f'{n_src}x{n_tgt} posed')


def test_association_ragged_pairs(gpu):
    """Three pairs in one call, an empty source and an empty target among them."""
    rng = np.random.default_rng(7)
    srcs = [rng.uniform(0, 1, (n, 3)).astype(np.float32) for n in (300, 0, 70)]
    tgts = [rng.uniform(0, 1, (n, 3)).astype(np.float32) for n in (500, 40, 0)]
    poses = [_pose(rng) for _ in range(3)]
    refs = _assert_association(gpu, srcs, tgts, poses, 0.12, 'ragged')
    assert (refs[0][0] >= 0).sum() > 50 and (refs[2][0] < 0).all()


def test_association_exact_ties(gpu):
    """Exact duplicates and lattice targets with queries at cell centres (eight targets at the
    same d2): the lowest target row wins, whatever order the cells hold their members in."""
    rng = np.random.default_rng(8)
    g = np.arange(6) * 0.25
    lat = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    tgt = np.concatenate([lat, lat])[rng.permutation(2 * len(lat))]
    centres = (lat[rng.choice(len(lat), 100)] + np.float32(0.125)).astype(np.float32)
    src = np.concatenate([centres, lat[:50]])
    (ri, rd, gaps), = _assert_association(gpu, [src], [tgt], [EYE], 0.3, 'ties')
    assert gaps[0] == 0.0 and (ri >= 0).all()
    assert (rd[:100] == np.float32(3 * 0.125 ** 2)).all() and (rd[100:] == 0).all()


def test_association_cell_boundaries_and_outside(gpu):
    """Targets on the grid's cell boundaries (r = 1: cells of edge 1.0625 from the cloud's
    minimum, targets at its multiples); queries inside, outside the bounding box by less and by
    more than r, and very far away."""
    rng = np.random.default_rng(9)
    g = np.arange(5) * np.float32(1.0625)
    tgt = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    inside = rng.uniform(0, 4.25, (200, 3)).astype(np.float32)
    on = tgt[rng.choice(len(tgt), 40)] + rng.uniform(-0.3, 0.3, (40, 3)).astype(np.float32)
    out = np.array([[4.25 + 0.5, 1, 1], [4.25 + 1.5, 1, 1], [-0.5, 2, 2], [-1.5, 2, 2],
                    [2, 2, 4.25 + 0.9], [2, 2, -5], [1e6, 0, 0], [-1e15, 1e15, 0]], np.float32)
    src = np.concatenate([inside, on, out]).astype(np.float32)
    (ri, _, _), = _assert_association(gpu, [src], [tgt], [EYE], 1.0, 'boundaries')
    assert (ri[[241, 243, 245, 246, 247]] == -1).all()
    assert ri[240] >= 0 and ri[242] >= 0 and ri[244] >= 0


def test_association_radius_is_strict(gpu):
    """d2 == r2 exactly (r = 0.5, the query at (0.5, 0, 0), the target at the origin)."""
    f, e, idx, d2, info = _score(gpu, [np.array([[0.5, 0, 0]], np.float32)],
                                 [np.zeros((1, 3), np.float32)], [EYE], 0.5)
    assert idx[0] == -1 and np.isinf(d2[0]) and f[0] == 0 and e[0] == 0 and not info.any()


def test_association_grown_cells(gpu):
    """A target whose grid takes the 1.25x cell-growth path: 1000 points on a line 200 r long,
    along the cube's diagonal (115^3 cells of edge 1.0625 r against a budget of 5024)."""
    rng = np.random.default_rng(10)
    r = 0.05
    u = np.sort(rng.uniform(0, 200 * r, 1000))
    tgt = (u[:, None] * np.ones(3) / np.sqrt(3)).astype(np.float32)
    assert (np.floor(np.ptp(tgt, 0) / np.float32(r * 1.0625)) + 1).prod() > 4 * 1000 + 1024
    src = (tgt[rng.choice(1000, 400)] + rng.normal(0, 0.5 * r, (400, 3))).astype(np.float32)
    (ri, _, _), = _assert_association(gpu, [src], [tgt], [EYE], r, 'line')
    assert 50 < (ri >= 0).sum() < 400


# ---------------------------------------------------------------------------------------------
# one solve
# ---------------------------------------------------------------------------------------------
def _lidar():
    from fgreg.synthetic import lidar_like_pair
    src, tgt, pose = lidar_like_pair(0, n_points=2000)
    return src, tgt, pose, 0.5


def _thin(mirror):
    """The mirrored cloud of test_gpu_tail_kernels.py made thin, so that the nearest target of
    a source point is its own mirror image: det H < 0, the reflection branch."""
    rng = np.random.default_rng(52)
    a = (rng.uniform(-1, 1, (80, 3)) * (1.0, 0.7, 0.01)).astype(np.float32)
    T = _pose(rng, 25.0, 0.3).astype(np.float64)
    b = (a.astype(np.float64) * (1, 1, -1 if mirror else 1)) @ T[:, :3].T + T[:, 3]
    return a, (b + rng.normal(size=b.shape) * 1e-3).astype(np.float32), T.astype(np.float32), 0.1


def _coplanar(tilt):
    rng = np.random.default_rng(51)
    a = rng.uniform(-1, 1, (60, 3))
    a[:, 2] = 0.0
    if tilt:
        a = a @ ir.rotation([1, 2, 3], 33.0).T + 0.3
    a = a.astype(np.float32)
    T = _pose(rng, 25.0, 0.3).astype(np.float64)
    b = (a.astype(np.float64) @ T[:, :3].T + T[:, 3] + rng.normal(size=a.shape) * 0.01).astype(np.float32)
    return a, b, T.astype(np.float32), 0.1


SOLVE_CASES = {'lidar-60m': _lidar, 'mirrored': lambda: _thin(True), 'thin': lambda: _thin(False),
               'coplanar': lambda: _coplanar(False), 'coplanar-tilted': lambda: _coplanar(True)}


@pytest.mark.parametrize('name', list(SOLVE_CASES))
def test_one_solve(gpu, name):
    """max_iters = 1: pass 0 associates under the given pose and solves, pass 1 scores the
    result. The restatement is fed the kernel's own correspondences (checked exact first)."""
    src, tgt, pose0, r = SOLVE_CASES[name]()
    (idx, d2, _), = _assert_association(gpu, [src], [tgt], [pose0], r, name)
    n, sp, ss, sps, _ = ir.moments(src, tgt, idx, d2)
    assert n >= 30
    if name == 'mirrored':
        assert np.linalg.det(sps - np.outer(sp, ss) / n) < 0
    want, _, _ = ir.solve(src, tgt, idx, d2)
    pose, f, e, it = _icp(gpu, [src], [tgt], [pose0], r, max_iters=1)
    assert it[0] == 1
    _check('pose', _pose_err(pose[0], want), name)
    R = pose[0, :, :3].astype(np.float64)
    assert abs(np.linalg.det(R) - 1) < 1e-6 and np.abs(R.T @ R - np.eye(3)).max() < 1e-6
    # the reported fitness and rmse belong to the returned pose
    f1, e1, *_ = _score(gpu, [src], [tgt], [pose[0]], r)
    assert f1[0] == f[0] and e1[0] == e[0]


# ---------------------------------------------------------------------------------------------
# the whole loop
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loop_ref(seed):
    src, tgt, pose0, r = ir.loop_problem(seed)
    return src, tgt, pose0, r, ir.icp(src, tgt, pose0, r)


@pytest.mark.parametrize('seed', [5, 7, 10, 15, 17, 30])
def test_whole_loop(gpu, seed):
    src, tgt, pose0, r, ref = _loop_ref(seed)
    assert np.min(ref['gaps']) >= 1e-5 * r, ref['gaps']     # the precondition, not a skip
    assert 4 <= ref['n_iters'] <= 8
    pose, f, e, it = _icp(gpu, [src], [tgt], [pose0], r)
    print(f'seed {seed}: n_iters {it[0]} (restatement {ref["n_iters"]})')
    assert it[0] == ref['n_iters']
    _, _, idx, _, _ = _score(gpu, [src], [tgt], [pose[0]], r)
    assert np.array_equal(idx, ref['idx'])
    assert f[0] == np.float32(ref['fitness'])
    _check('pose', _pose_err(pose[0], ref['pose']), f'loop seed {seed}')
    _check('rmse', _relmax(e, [ref['rmse']]), f'loop seed {seed}')


def _exact_pair():
    rng = np.random.default_rng(77)
    tgt = rng.uniform(0, 1, (300, 3)).astype(np.float32)
    return tgt[::2].copy(), tgt


def test_freezing(gpu):
    """Two pairs in one call: one done after 2 passes (an exact copy under the identity:
    fitness 1 and rmse 0 twice), one that needs more. The early pair's outputs are bit-identical
    to running it alone with max_iters = 100."""
    a_src, a_tgt = _exact_pair()
    b_src, b_tgt, b_pose, r, ref = _loop_ref(5)
    both = _icp(gpu, [a_src, b_src], [a_tgt, b_tgt], [EYE, b_pose], r)
    alone = _icp(gpu, [a_src], [a_tgt], [EYE], r, max_iters=100)
    assert both[3].tolist() == [1, ref['n_iters']] and alone[3][0] == 1
    for x, y in zip(both, alone):
        assert bit_equal(_t(x[0:1]), _t(y[0:1]))
    assert both[1][0] == 1.0 and both[2][0] == 0.0
    b_alone = _icp(gpu, [b_src], [b_tgt], [b_pose], r)
    for x, y in zip(both, b_alone):
        assert bit_equal(_t(x[1:2]), _t(y[0:1]))


def test_degenerate(gpu):
    rng = np.random.default_rng(12)
    r = 0.1
    pose0 = _pose(rng)
    src = rng.uniform(0, 1, (100, 3)).astype(np.float32)
    far = (src + np.float32(10 * r) * 3).astype(np.float32)          # clouds >= 10 r apart
    pose, f, e, it = _icp(gpu, [src], [far], [EYE], r)
    assert np.array_equal(pose[0], EYE) and f[0] == 0 and e[0] == 0 and it[0] == 0
    # exactly two inliers: too few to solve, the fitness is still reported
    tgt = np.concatenate([ir.transform32(pose0, src[:2]) + np.float32(0.01),
                          rng.uniform(5, 6, (20, 3)).astype(np.float32)])
    assert (ir.associate(src, tgt, pose0, r)[0] >= 0).sum() == 2
    pose, f, e, it = _icp(gpu, [src], [tgt], [pose0], r)
    assert np.array_equal(pose[0], pose0) and it[0] == 0
    assert f[0] == np.float32(2 / 100) and 0.015 < e[0] < 0.02


def test_graph_capture_and_repeat(gpu):
    """fgr_icp makes no host readback, allocation or sync: it can be captured into a graph, and
    replays and repeated eager calls give the eager call's bits."""
    src, tgt, pose0, r, ref = _loop_ref(7)
    B = 1
    d = lambda a: _t(a).to(gpu)
    s, t, po = d(src), d(tgt), d(pose0.reshape(1, 12))
    so, to = d(ir.offsets([len(src)])), d(ir.offsets([len(tgt)]))
    need = _need(len(src), len(tgt), B)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    outs = lambda: (torch.zeros(B, 12, device=gpu), torch.zeros(B, device=gpu),
                    torch.zeros(B, device=gpu), torch.zeros(B, dtype=I32, device=gpu))

    def call(o):
        _ok(_L().fgr_icp(_p(s), _p(so), len(src), _p(t), _p(to), len(tgt), B, len(src), _p(po), r,
                         30, 1e-6, 1e-6, _p(ws), need, *(_p(x) for x in o), _st()), 'fgr_icp')

    eager, again = outs(), outs()
    call(eager)
    call(again)
    torch.cuda.synchronize()
    assert int(eager[3][0]) == ref['n_iters']
    for x, y in zip(eager, again):
        assert bit_equal(x, y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    cap = outs()
    with torch.cuda.stream(side):
        call(cap)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(cap)
    for _ in range(2):
        for x in cap:
            x.zero_()
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(eager, cap):
            assert bit_equal(x, y)


def test_short_workspace_is_refused(gpu):
    """ws_bytes - 16 (passed as a smaller number): FGR_E_WORKSPACE from both entry points, every
    output and the workspace still untouched."""
    src, tgt, pose0, r, _ = _loop_ref(5)
    g = _Geo([src], [tgt], [pose0])
    ar = Arena(gpu)
    g.put(ar)
    outs = [ar.matrix(1, 12, 12, F32, 'out', 'pose_out', full=False),
            ar.vector(1, F32, 'out', 'fitness', full=False), ar.vector(1, F32, 'out', 'rmse', full=False),
            ar.vector(1, I32, 'out', 'n_iters', full=False),
            ar.vector(g.ns, I32, 'out', 'idx', full=False), ar.vector(g.ns, F32, 'out', 'd2', full=False),
            ar.matrix(1, 36, 36, F64, 'out', 'info', full=False)]
    po, f, e, it, idx, d2, info = outs
    rc = _L().fgr_icp(*g.args(), _p(g.d[4]), r, 30, 1e-6, 1e-6, _p(g.ws), g.need - 16, _p(po),
                      _p(f), _p(e), _p(it), _st())
    assert rc == -3 and b'fgr_icp: workspace' in _L().fgr_last_error()
    rc = _L().fgr_registration_score(*g.args(), _p(g.d[4]), r, _p(g.ws), g.need - 16, _p(f), _p(e),
                                     _p(idx), _p(d2), _p(info), _st())
    assert rc == -3 and b'fgr_registration_score: workspace' in _L().fgr_last_error()
    torch.cuda.synchronize()
    ar.check()
    for o in outs:
        assert bool((o.contiguous().view(torch.int32) == SENTINEL).all())
    assert not bool(g.ws.any())
    assert _L().fgr_icp(*g.args(), _p(g.d[4]), -1.0, 30, 1e-6, 1e-6, _p(g.ws), g.need, _p(po),
                        _p(f), _p(e), _p(it), _st()) == -1


# ---------------------------------------------------------------------------------------------
# fgreg.refine
# ---------------------------------------------------------------------------------------------
def test_python_api_matches_the_abi(gpu):
    """Ragged lists, B = 3: fgreg.refine.icp / score return the ABI call's bits."""
    import fgreg
    rng = np.random.default_rng(21)
    tgts = [rng.uniform(0, 1, (n, 3)).astype(np.float32) for n in (400, 150, 260)]
    poses = np.stack([_pose(rng, 4.0, 0.02) for _ in range(3)])
    srcs = []
    for t, T, n in zip(tgts, poses, (300, 150, 77)):
        Ti = np.linalg.inv(np.vstack([T.astype(np.float64), [0, 0, 0, 1]]))[:3]
        srcs.append((t[:n].astype(np.float64) @ Ti[:, :3].T + Ti[:, 3] +
                     rng.normal(0, 0.002, (n, 3))).astype(np.float32))
    start = np.stack([EYE] * 3)
    r = 0.08
    dv = lambda xs: [_t(x).to(gpu) for x in xs]
    out = fgreg.icp(dv(srcs), dv(tgts), _t(start).to(gpu), r, information=True)
    pose, f, e, it = _icp(gpu, srcs, tgts, start, r)
    assert set(out) == {'pose', 'fitness', 'inlier_rmse', 'n_iters', 'information'}
    assert out['n_iters'].dtype == torch.int32 and (it >= 2).all()
    for got, want in ((out['pose'], pose), (out['fitness'], f), (out['inlier_rmse'], e),
                      (out['n_iters'], it)):
        assert bit_equal(got.cpu(), _t(want))
    sc = fgreg.score(dv(srcs), dv(tgts), out['pose'], r, information=True, correspondences=True)
    f2, e2, idx, d2, info = _score(gpu, srcs, tgts, pose, r)
    assert bit_equal(sc['fitness'].cpu(), _t(f2)) and bit_equal(sc['inlier_rmse'].cpu(), _t(e2))
    assert bit_equal(sc['fitness'].cpu(), _t(f))            # of the returned pose
    assert bit_equal(torch.cat(sc['idx']).cpu(), _t(idx)) and bit_equal(torch.cat(sc['d2']).cpu(), _t(d2))
    assert [len(x) for x in sc['idx']] == [300, 150, 77]
    assert bit_equal(sc['information'].cpu(), _t(info)) and bit_equal(out['information'].cpu(), _t(info))
    with pytest.raises(fgreg.FgrError):
        fgreg.icp([_t(s) for s in srcs], [_t(t) for t in tgts], _t(start), r)


def test_refine_outputs_lowers_the_pose_error(gpu):
    """A ModelNet synthetic batch, the ground-truth pose perturbed by 4 degrees and 0.03:
    refine_outputs from outputs['pose'][-1] lowers both errors of every pair."""
    import fgreg
    from fgreg.synthetic import make_batch
    src, tgt, gt = make_batch('modelnet', 3)
    rng = np.random.default_rng(31)
    start = []
    for T in gt.astype(np.float64):
        dR = ir.rotation(rng.normal(size=3), 4.0)
        start.append(np.concatenate([dR @ T[:, :3], (dR @ T[:, 3] + rng.uniform(-0.03, 0.03, 3))[:, None]], 1))
    start = np.stack(start).astype(np.float32)
    batch = {'src_xyz': [_t(s).to(gpu) for s in src], 'tgt_xyz': [_t(t).to(gpu) for t in tgt]}
    outputs = {'pose': _t(np.stack([np.stack([EYE] * 3), start])).to(gpu)}
    out = fgreg.refine_outputs(batch, outputs, 0.1)
    pose = out['pose'].cpu().numpy().astype(np.float64)

    def errs(P):
        rot = [np.degrees(np.arccos(np.clip((np.trace(p[:, :3] @ g[:, :3].T) - 1) / 2, -1, 1)))
               for p, g in zip(P, gt.astype(np.float64))]
        return np.array(rot), np.linalg.norm(P[:, :, 3] - gt[:, :, 3], axis=1)

    (r0, t0), (r1, t1) = errs(start.astype(np.float64)), errs(pose)
    print('rotation error', r0, '->', r1, 'translation error', t0, '->', t1)
    assert (r1 < r0).all() and (t1 < t0).all()
    assert (out['n_iters'].cpu().numpy() >= 1).all() and (out['fitness'].cpu().numpy() > 0.3).all()
