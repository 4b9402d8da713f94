"""The normals and point-to-plane ICP kernels (csrc/normals.hip: fgr_estimate_normals,
csrc/icp.hip: fgr_icp_plane) against the numpy restatement tests/_icp_plane_ref.py (pinned on
the CPU by tests/test_icp_plane_ref.py), through the C ABI with every operand carved out of a
guarded arena (tests/_arena.py) -- each call runs on a clean and on a poisoned arena with
bit-identical results and the workspace is exactly the *_workspace() bytes -- and through
fgreg.refine.

Discrete results are compared exactly: n_valid and which normals are zero, the inlier count,
fitness (n / n_src in fp64, rounded once), n_iters, status, the final associations, the poses
that must come back unchanged. Values are compared at BOUNDS: worst |got - ref| / max(1, |ref|)
measured on the MI355X against the fp64 restatement, times <= 4, never looser than the ceiling.

  family                                         measured   asserted   ceiling
  normal  |n - n_ref|max where the restatement's
          eigen-gap >= 0.05 and the sign margin
          >= 1e-6 (fp64 moments over a gap of
          0.05, then one fp32 store)             0 (1742 rows
                                                 bit-equal)  0          1e-6
  pose    one update and the whole loop          2.96e-08   1.1e-07    1e-4
  rmse    inlier_rmse, plane_rmse (fp64 sqrt,
          stored as fp32)                        1.76e-09   7.0e-09    1e-4
  info    fp64 sums in block order vs numpy's    1.24e-15   4.9e-15    1e-10

The normals are an fp64 eigenvector on both sides, equal to about 1e-15, rounded once to fp32:
every compared component came out bit-equal, so the bound is 0. The six whole-loop poses are
bit-equal to the restatement's too; the pose figure comes from the single updates.

The normals inputs (_icp_plane_ref.normals_cases) are chosen so that the filter keeps >= 90 % of
every cloud's valid normals; the test asserts that first. The whole-loop inputs are the seeds
for which the restatement alone keeps every pass >= 4e-5 r from a different discrete result;
the test asserts >= 1e-5 r first, then n_iters, status and the final associations must be
equal. The benefit inputs are seeds whose restatement shows a factor >= 4 (CPU test); the
device is asked for a factor of 3.
"""
import functools

import numpy as np
import pytest
import torch

import _icp_plane_ref as pr
import _icp_ref as ir
from _arena import SENTINEL, Arena, assert_both_equal, bit_equal, run_both

pytestmark = pytest.mark.gpu
F32, F64, I32 = torch.float32, torch.float64, torch.int32

BOUNDS = {'normal': 0.0, 'pose': 1.1e-7, 'rmse': 7.0e-9, 'info': 4.9e-15}


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


def _need(name, *args):
    from fgreg import _lib
    nb = _lib._sz(0)
    _ok(getattr(_L(), name)(*args, nb), name)
    return nb.value


def _both(fn, gpu):
    clean, poisoned = run_both(fn, gpu)
    assert_both_equal(clean, poisoned)
    return tuple(t.cpu().numpy() for t in clean)


def _normals(gpu, clouds, radius, view=None):
    """fgr_estimate_normals -> normals (N, 3), n_valid (n_clouds) (numpy)."""
    pts, off = ir.pack(clouds)
    n, nc = len(pts), len(clouds)
    need = _need('fgr_estimate_normals_workspace', n, nc)

    def fn(ar):
        d_pts, d_off = ar.put(_t(pts), name='pts'), ar.put(_t(off), name='off')
        d_view = None if view is None else ar.put(_t(np.asarray(view, np.float32)), name='view')
        ws = ar.bytes(need, name='ws')
        out = ar.matrix(n, 3, 3, F32, 'out', 'normals')
        nv = ar.vector(nc, I32, 'out', 'n_valid')
        _ok(_L().fgr_estimate_normals(_p(d_pts), _p(d_off), n, nc, radius, _p(d_view), _p(ws), need,
                                      _p(out), _p(nv), _st()), 'fgr_estimate_normals')
        return out, nv

    return _both(fn, gpu)


class _Geo:
    """The packed geometry of a plane call and its operands inside an arena."""

    def __init__(self, srcs, tgts, nrms, poses):
        self.src, self.so = ir.pack(srcs)
        self.tgt, self.to = ir.pack(tgts)
        self.nrm, _ = ir.pack(nrms)
        self.B = len(srcs)
        self.ns, self.nt = len(self.src), len(self.tgt)
        self.max_len = max(len(s) for s in srcs)
        self.pose = np.asarray(poses, np.float32).reshape(self.B, 12)
        self.need = _need('fgr_icp_plane_workspace', self.ns, self.nt, self.B)
        assert self.ns > 0 and self.nt > 0 and len(self.nrm) == self.nt

    def put(self, ar):
        self.d = [ar.put(_t(self.src), name='src'), ar.put(_t(self.so), name='src_off'),
                  ar.put(_t(self.tgt), name='tgt'), ar.put(_t(self.to), name='tgt_off'),
                  ar.put(_t(self.nrm), name='tgt_normals'), ar.put(_t(self.pose), name='pose')]
        self.ws = ar.bytes(self.need, name='ws')

    def args(self):
        s, so, t, to, n, _ = self.d
        return (_p(s), _p(so), self.ns, _p(t), _p(to), self.nt, _p(n), self.B, self.max_len)


OUTS = ('pose', 'fitness', 'rmse', 'plane_rmse', 'n_iters', 'status', 'info')


def _plane(gpu, srcs, tgts, nrms, poses, r, max_iters=30, rel_f=1e-6, rel_e=1e-6):
    """fgr_icp_plane with every output -> dict of numpy arrays (pose (B, 3, 4), info (B, 6, 6))."""
    g = _Geo(srcs, tgts, nrms, poses)

    def fn(ar):
        g.put(ar)
        po = ar.matrix(g.B, 12, 12, F32, 'out', 'pose_out')
        f, e, pe = (ar.vector(g.B, F32, 'out', k) for k in ('fitness', 'rmse', 'plane_rmse'))
        it, st = ar.vector(g.B, I32, 'out', 'n_iters'), ar.vector(g.B, I32, 'out', 'status')
        info = ar.matrix(g.B, 36, 36, F64, 'out', 'info')
        _ok(_L().fgr_icp_plane(*g.args(), _p(g.d[5]), r, max_iters, rel_f, rel_e, _p(g.ws), g.need,
                               _p(po), _p(f), _p(e), _p(pe), _p(it), _p(st), _p(info), _st()),
            'fgr_icp_plane')
        return po, f, e, pe, it, st, info

    out = dict(zip(OUTS, _both(fn, gpu)))
    out['pose'], out['info'] = out['pose'].reshape(g.B, 3, 4), out['info'].reshape(g.B, 6, 6)
    return out


def _device_idx(gpu, srcs, tgts, poses, r):
    """The association of the existing fgr_registration_score under `poses` -> packed idx, d2."""
    src, so = ir.pack(srcs)
    tgt, to = ir.pack(tgts)
    B, ns, nt = len(srcs), len(src), len(tgt)
    need = _need('fgr_icp_workspace', ns, nt, B)
    d = lambda a: _t(a).to(gpu)
    ops = [d(src), d(so), d(tgt), d(to), d(np.asarray(poses, np.float32).reshape(B, 12))]
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    f, e = torch.empty(B, device=gpu), torch.empty(B, device=gpu)
    idx, d2 = torch.empty(ns, dtype=I32, device=gpu), torch.empty(ns, device=gpu)
    _ok(_L().fgr_registration_score(_p(ops[0]), _p(ops[1]), ns, _p(ops[2]), _p(ops[3]), nt, B,
                                    max(len(s) for s in srcs), _p(ops[4]), r, _p(ws), need, _p(f),
                                    _p(e), _p(idx), _p(d2), None, _st()), 'fgr_registration_score')
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy()


def _pose(rng, deg=10.0, trans=0.05):
    R = ir.rotation(rng.normal(size=3), deg)
    return np.concatenate([R, rng.uniform(-trans, trans, (3, 1))], 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# normals
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _normals_ref(name):
    clouds, radius, view = pr.normals_cases()[name]
    return [pr.normals(c, radius, None if view is None else view[i]) for i, c in enumerate(clouds)]


@pytest.mark.parametrize('name', list(pr.normals_cases()))
def test_normals(gpu, name):
    clouds, radius, view = pr.normals_cases()[name]
    refs = _normals_ref(name)
    got, n_valid = _normals(gpu, clouds, radius, view)
    off = ir.offsets([len(c) for c in clouds])
    for c, ref in enumerate(refs):
        n = got[off[c]:off[c + 1]]
        keep = pr.comparable(ref)
        assert keep.sum() >= 0.9 * ref['valid'].sum(), (name, c)      # the condition, first
        assert n_valid[c] == ref['valid'].sum(), (name, c, n_valid[c], ref['valid'].sum())
        assert np.array_equal((n == 0).all(1), ~ref['valid']), (name, c)
        if not ref['valid'].any():
            continue
        norm = np.linalg.norm(n[ref['valid']].astype(np.float64), axis=1)
        assert np.abs(norm - 1).max() <= 2.0 ** -22, (name, c, np.abs(norm - 1).max())
        if keep.any():
            _check('normal', np.abs(n[keep].astype(np.float64) - ref['normals'][keep]).max(),
                   f'{name} cloud {c}: {keep.sum()} of {len(n)} rows')
    if name == 'viewpoint':       # the sign is the viewpoint's: the origin gives other normals
        assert not np.array_equal(got, _normals(gpu, clouds, radius)[0])
    if name == 'duplicates':      # copies of one point: the same neighbourhood, the same bits
        assert np.array_equal(got[40:50], got[:10]) and (got[50:54] != 0).any(1).all()


def test_normals_repeat_and_exact_plane(gpu):
    """Two calls give the same bits (the sums are taken in sorted cell order, not in the grid
    build's arrival order), and an exact plane z = 0.5 gives exactly (0, 0, -1): its covariance
    has an exactly zero z row, which the Jacobi sweep leaves alone."""
    cloud = pr.lattice_slab(5)
    a = _normals(gpu, [cloud], 0.36)
    for _ in range(3):
        b = _normals(gpu, [cloud], 0.36)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    rng = np.random.default_rng(0)
    flat = np.concatenate([rng.uniform(0, 1, (300, 2)), np.full((300, 1), 0.5)], 1).astype(np.float32)
    n, nv = _normals(gpu, [flat], 0.3)
    assert nv[0] == 300 and np.array_equal(n, np.tile(np.float32([0, 0, -1]), (300, 1)))
    # n . (view - p) exactly 0 (the plane holds the viewpoint): first non-zero component positive
    n, _ = _normals(gpu, [flat], 0.3, view=np.float32([[0.2, 0.3, 0.5]]))
    assert np.array_equal(n, np.tile(np.float32([0, 0, 1]), (300, 1)))


def test_normals_refusals(gpu):
    """A short workspace is FGR_E_WORKSPACE and bad arguments FGR_E_ARG, outputs untouched."""
    cloud = pr.patch(40, 1)
    pts, off = ir.pack([cloud])
    need = _need('fgr_estimate_normals_workspace', 40, 1)
    ar = Arena(gpu)
    d_pts, d_off = ar.put(_t(pts)), ar.put(_t(off))
    ws = ar.bytes(need, name='ws')
    out = ar.matrix(40, 3, 3, F32, 'out', 'normals', full=False)
    nv = ar.vector(1, I32, 'out', 'n_valid', full=False)
    call = lambda radius, nbytes: _L().fgr_estimate_normals(
        _p(d_pts), _p(d_off), 40, 1, radius, None, _p(ws), nbytes, _p(out), _p(nv), _st())
    assert call(0.4, need - 16) == -3 and b'fgr_estimate_normals: workspace' in _L().fgr_last_error()
    assert call(0.0, need) == -1 and call(float('inf'), need) == -1
    torch.cuda.synchronize()
    ar.check()
    assert bool((out.contiguous().view(torch.int32) == SENTINEL).all()) and not bool(ws.any())


# ---------------------------------------------------------------------------------------------
# one pass
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _room(seed=3, n_tgt=800, n_src=65, radius=0.12):
    src, tgt, pose0, truth, r = pr.room_problem(seed, n_tgt, n_src)
    return src, tgt, pr.normals(tgt, radius)['normals'], pose0, r


def _one_pass_cases():
    src, tgt, nrm, pose0, r = _room()
    cases = {f'n{n}': ([src[:n]], [tgt], [nrm], [pose0], r) for n in (1, 31, 32, 33, 65)}
    s2, t2, n2, p2, _ = _room(4, 500, 50)
    cases['ragged2'] = ([src, s2], [tgt, t2], [nrm, n2], [pose0, p2], r)
    s3, t3, n3, p3, _ = _room(6, 300, 40)
    cases['ragged3-empty-source'] = ([s2[:33], src[:0], s3], [t2, tgt[:50], t3], [n2, nrm[:50], n3],
                                     [p2, pose0, p3], r)
    cases['far-outside'] = ([src + np.float32(50.0), src[:40]], [tgt, tgt], [nrm, nrm], [pose0, pose0], r)
    holes = nrm.copy()
    holes[::3] = 0                                          # a third of the targets without normal
    cases['zero-normals'] = ([src], [tgt], [holes], [pose0], r)
    ps, pt, pn, pp, pr_ = pr.plane_only(0)
    cases['plane-only'] = ([ps, src], [pt, tgt], [pn, nrm], [pp, pose0], pr_)
    return cases


@pytest.mark.parametrize('max_iters', [0, 1])
@pytest.mark.parametrize('name', list(_one_pass_cases()))
def test_one_pass(gpu, name, max_iters):
    """max_iters = 0: pass 0 measures the given pose and stops. max_iters = 1: pass 0 updates,
    pass 1 measures the result. The restatement is fed the associations of the pose each pass
    ran under (the device's own pose for pass 1), checked equal to the device's first."""
    srcs, tgts, nrms, poses, r = _one_pass_cases()[name]
    out = _plane(gpu, srcs, tgts, nrms, poses, r, max_iters=max_iters, rel_f=0.0, rel_e=0.0)
    first = [None] * len(srcs)
    for b, (s, t, n) in enumerate(zip(srcs, tgts, nrms)):
        idx, d2, _ = pr.associate(s, t, poses[b], r)
        first[b] = pr.step(s, t, n, poses[b], pr.inliers(idx, n), d2, 0, max_iters)
    under = [p if st['pose'] is None else out['pose'][b] for b, (p, st) in enumerate(zip(poses, first))]
    dev_idx, dev_d2 = _device_idx(gpu, srcs, tgts, under, r)
    so = ir.offsets([len(s) for s in srcs])
    for b, (s, t, n) in enumerate(zip(srcs, tgts, nrms)):
        what = f'{name} max_iters {max_iters} pair {b}'
        st0 = first[b]
        idx, d2, _ = pr.associate(s, t, under[b], r)       # of the last pass the pair ran
        assert np.array_equal(dev_idx[so[b]:so[b + 1]], idx), what
        assert np.array_equal(dev_d2[so[b]:so[b + 1]].view(np.uint32), d2.view(np.uint32)), what
        if st0['pose'] is None:                            # stopped in pass 0
            assert np.array_equal(out['pose'][b], np.asarray(poses[b], np.float32)), what
            assert out['n_iters'][b] == 0 and out['status'][b] == st0['status'], what
            last = st0
        else:
            assert max_iters == 1 and out['n_iters'][b] == 1, what
            _check('pose', _pose_err(out['pose'][b], st0['pose']), what)
            last = pr.step(s, t, n, out['pose'][b], pr.inliers(idx, n), d2, 1, 1)
            assert out['status'][b] == last['status'], what
        assert out['fitness'][b] == np.float32(last['fitness']), what
        assert round(np.trace(out['info'][b][:3, :3])) == last['n'], what
        _check('rmse', _relmax([out['rmse'][b], out['plane_rmse'][b]], [last['rmse'], last['plane_rmse']]), what)
        _check('info', _relmax(out['info'][b], last['info']), what)
        assert np.array_equal(out['info'][b], out['info'][b].T), what
        assert (out['rmse'][b] == 0) == (last['n'] == 0), what
    st = out['status'].tolist()
    if name == 'plane-only':
        assert st[0] == pr.SINGULAR and st[1] == pr.MAX_ITERS
    if name == 'far-outside':
        assert st[0] == pr.FEW_INLIERS and out['fitness'][0] == 0 and not out['info'][0].any()
    if name == 'ragged3-empty-source':
        assert st[1] == pr.FEW_INLIERS and out['fitness'][1] == 0 and st[0] == st[2] == pr.MAX_ITERS
    if name == 'n1':
        assert st == [pr.FEW_INLIERS]
    if name in ('n31', 'n32', 'n33', 'n65', 'zero-normals', 'ragged2'):
        assert set(st) == {pr.MAX_ITERS} and (out['fitness'] > 0.5).all()
    if name == 'zero-normals':
        assert out['fitness'][0] < 0.8                      # the zero normals took inliers away


# ---------------------------------------------------------------------------------------------
# the whole loop
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loop_ref(seed):
    src, tgt, pose0, truth, r = pr.room_problem(seed, *pr.LOOP_SIZES)
    nrm = pr.normals(tgt, pr.LOOP_NORMAL_RADIUS)['normals']
    return src, tgt, nrm, pose0, r, pr.icp_plane(src, tgt, nrm, pose0, r)


@pytest.mark.parametrize('seed', pr.LOOP_SEEDS)
def test_whole_loop(gpu, seed):
    src, tgt, nrm, pose0, r, ref = _loop_ref(seed)
    assert np.min(ref['gaps']) >= 1e-5 * r, ref['gaps']     # the precondition, not a skip
    assert ref['status'] == pr.CONVERGED and ref['n_iters'] >= 3
    out = _plane(gpu, [src], [tgt], [nrm], [pose0], r)
    print(f'seed {seed}: n_iters {out["n_iters"][0]} (restatement {ref["n_iters"]})')
    assert out['n_iters'][0] == ref['n_iters'] and out['status'][0] == ref['status']
    idx, _ = _device_idx(gpu, [src], [tgt], [out['pose'][0]], r)
    assert np.array_equal(pr.inliers(idx, nrm), ref['idx'])
    assert out['fitness'][0] == np.float32(ref['fitness'])
    _check('pose', _pose_err(out['pose'][0], ref['pose']), f'loop seed {seed}')
    _check('rmse', _relmax([out['rmse'][0], out['plane_rmse'][0]], [ref['rmse'], ref['plane_rmse']]),
           f'loop seed {seed}')
    _check('info', _relmax(out['info'][0], ref['info']), f'loop seed {seed}')
    # <= 30 fp32 stores of a 3-term product
    R = out['pose'][0, :, :3].astype(np.float64)
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-5


def test_freezing(gpu):
    """Three pairs in one call -- one singular in pass 0, two that converge after different
    numbers of updates: each pair's outputs are bit-identical to running it alone."""
    a = _loop_ref(pr.LOOP_SEEDS[0])
    b = _loop_ref(pr.LOOP_SEEDS[1])
    ps, pt, pn, pp, _ = pr.plane_only(1)
    r = a[4]
    pairs = [(ps, pt, pn, pp), a[:4], b[:4]]
    both = _plane(gpu, *(list(x) for x in zip(*pairs)), r)
    assert both['status'].tolist() == [pr.SINGULAR, pr.CONVERGED, pr.CONVERGED]
    assert both['n_iters'].tolist() == [0, a[5]['n_iters'], b[5]['n_iters']]
    for i, p in enumerate(pairs):
        alone = _plane(gpu, [p[0]], [p[1]], [p[2]], [p[3]], r, max_iters=30 + 10 * i)
        for k in OUTS:
            assert bit_equal(_t(both[k][i:i + 1]), _t(alone[k])), (i, k)


def test_short_workspace_is_refused(gpu):
    src, tgt, nrm, pose0, r, _ = _loop_ref(pr.LOOP_SEEDS[0])
    g = _Geo([src], [tgt], [nrm], [pose0])
    ar = Arena(gpu)
    g.put(ar)
    outs = [ar.matrix(1, 12, 12, F32, 'out', 'pose_out', full=False)] + \
           [ar.vector(1, F32, 'out', k, full=False) for k in ('fitness', 'rmse', 'plane_rmse')] + \
           [ar.vector(1, I32, 'out', k, full=False) for k in ('n_iters', 'status')] + \
           [ar.matrix(1, 36, 36, F64, 'out', 'info', full=False)]
    call = lambda dist, nbytes: _L().fgr_icp_plane(*g.args(), _p(g.d[5]), dist, 30, 1e-6, 1e-6, _p(g.ws),
                                                   nbytes, *(_p(o) for o in outs), _st())
    assert call(r, g.need - 16) == -3 and b'fgr_icp_plane: workspace' in _L().fgr_last_error()
    assert call(-1.0, g.need) == -1
    torch.cuda.synchronize()
    ar.check()
    for o in outs:
        assert bool((o.contiguous().view(torch.int32) == SENTINEL).all())
    assert not bool(g.ws.any())


# ---------------------------------------------------------------------------------------------
# the benefit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', pr.BENEFIT_SEEDS)
def test_plane_beats_point_on_the_room(gpu, seed):
    """max_iters = 10 from the same start: the point-to-plane error against the generator's
    truth is at most a third of point-to-point's, in rotation and in translation (the
    restatement alone shows a quarter on these seeds: tests/test_icp_plane_ref.py)."""
    import fgreg
    src, tgt, pose0, truth, r = pr.room_problem(seed)
    S, T, P = [_t(src).to(gpu)], [_t(tgt).to(gpu)], _t(pose0[None]).to(gpu)
    plane = fgreg.icp(S, T, P, r, max_iters=10, method='point_to_plane',
                      normal_radius=pr.ROOM_NORMAL_RADIUS)
    point = fgreg.icp(S, T, P, r, max_iters=10)
    ep = pr.pose_errors(plane['pose'][0].cpu().numpy(), truth)
    eq = pr.pose_errors(point['pose'][0].cpu().numpy(), truth)
    print(f'seed {seed}: plane {ep} after {int(plane["n_iters"][0])}, point {eq} after '
          f'{int(point["n_iters"][0])}')
    assert 3 * ep[0] <= eq[0] and 3 * ep[1] <= eq[1]


# ---------------------------------------------------------------------------------------------
# fgreg.refine
# ---------------------------------------------------------------------------------------------
def _ragged():
    a, b = _room(4, 500, 50), _room(6, 300, 40)
    return [a[0], b[0]], [a[1], b[1]], np.stack([a[3], b[3]]), a[4]


def test_python_api_matches_the_abi(gpu):
    import fgreg
    srcs, tgts, poses, r = _ragged()
    dv = lambda xs: [_t(x).to(gpu) for x in xs]
    view = np.float32([[0.0, 0.0, 0.1], [0.2, 0.0, 0.0]])
    est = fgreg.estimate_normals(dv(tgts), 0.12, view=_t(view).to(gpu))
    n, nv = _normals(gpu, tgts, 0.12, view)
    assert set(est) == {'normals', 'n_valid'} and [len(x) for x in est['normals']] == [500, 300]
    assert bit_equal(torch.cat(est['normals']).cpu(), _t(n)) and bit_equal(est['n_valid'].cpu(), _t(nv))
    assert est['n_valid'].dtype == torch.int32
    # normal_radius = normals first (viewpoint: the origin), then tgt_normals
    nrm0 = fgreg.estimate_normals(dv(tgts), 0.12)['normals']
    P = _t(poses).to(gpu)
    auto = fgreg.icp(dv(srcs), dv(tgts), P, r, method='point_to_plane', normal_radius=0.12, information=True)
    given = fgreg.icp(dv(srcs), dv(tgts), P, r, method='point_to_plane', tgt_normals=nrm0, information=True)
    assert set(auto) == {'pose', 'fitness', 'inlier_rmse', 'n_iters', 'plane_rmse', 'status',
                         'tgt_normals', 'information'}
    abi = _plane(gpu, srcs, tgts, [x.cpu().numpy() for x in nrm0], poses, r)
    for k, a in (('pose', 'pose'), ('fitness', 'fitness'), ('inlier_rmse', 'rmse'), ('plane_rmse', 'plane_rmse'),
                 ('n_iters', 'n_iters'), ('status', 'status'), ('information', 'info')):
        assert bit_equal(auto[k].cpu(), given[k].cpu()) and bit_equal(auto[k].cpu(), _t(abi[a])), k
    for x, y in zip(auto['tgt_normals'], nrm0):
        assert bit_equal(x, y)
    assert (abi['n_iters'] >= 2).all() and auto['status'].dtype == torch.int32
    via = fgreg.refine_outputs({'src_xyz': dv(srcs), 'tgt_xyz': dv(tgts)}, {'pose': P[None]}, r,
                               method='point_to_plane', normal_radius=0.12)
    assert bit_equal(via['pose'], auto['pose'])
    # the default is the untouched point-to-point path: a direct fgr_icp call's bits
    default = fgreg.icp(dv(srcs), dv(tgts), P, r)
    src, so = ir.pack(srcs)
    tgt, to = ir.pack(tgts)
    need = _need('fgr_icp_workspace', len(src), len(tgt), 2)
    d = lambda x: _t(x).to(gpu)
    ops = [d(src), d(so), d(tgt), d(to), d(poses.reshape(2, 12))]
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    o = (torch.empty(2, 12, device=gpu), torch.empty(2, device=gpu), torch.empty(2, device=gpu),
         torch.empty(2, dtype=I32, device=gpu))
    _ok(_L().fgr_icp(_p(ops[0]), _p(ops[1]), len(src), _p(ops[2]), _p(ops[3]), len(tgt), 2, 50,
                     _p(ops[4]), r, 30, 1e-6, 1e-6, _p(ws), need, *(_p(x) for x in o), _st()), 'fgr_icp')
    assert set(default) == {'pose', 'fitness', 'inlier_rmse', 'n_iters'}
    for k, x in zip(('pose', 'fitness', 'inlier_rmse', 'n_iters'), o):
        assert bit_equal(default[k].reshape(x.shape), x), k
    with pytest.raises(ValueError):
        fgreg.icp(dv(srcs), dv(tgts), P, r, method='plane')
    with pytest.raises(ValueError):
        fgreg.icp(dv(srcs), dv(tgts), P, r, method='point_to_plane')
    with pytest.raises(fgreg.FgrError):
        fgreg.estimate_normals([_t(t) for t in tgts], 0.12)
    with pytest.raises(fgreg.FgrError):
        fgreg.icp([_t(s) for s in srcs], [_t(t) for t in tgts], _t(poses), r, method='point_to_plane',
                  tgt_normals=[x.cpu() for x in nrm0])


def test_graph_capture(gpu):
    """Normals and the plane loop make no host readback, allocation or sync: one capture, and
    the replay gives the eager call's bits."""
    src, tgt, _, pose0, r, _ = _loop_ref(pr.LOOP_SEEDS[2])
    d = lambda a: _t(a).to(gpu)
    s, t, po = d(src), d(tgt), d(pose0.reshape(1, 12))
    so, to = d(ir.offsets([len(src)])), d(ir.offsets([len(tgt)]))
    need_n = _need('fgr_estimate_normals_workspace', len(tgt), 1)
    need = _need('fgr_icp_plane_workspace', len(src), len(tgt), 1)
    ws_n = torch.empty(need_n, dtype=torch.uint8, device=gpu)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    outs = lambda: (torch.zeros(len(tgt), 3, device=gpu), torch.zeros(1, dtype=I32, device=gpu),
                    torch.zeros(1, 12, device=gpu), torch.zeros(1, device=gpu), torch.zeros(1, device=gpu),
                    torch.zeros(1, device=gpu), torch.zeros(1, dtype=I32, device=gpu),
                    torch.zeros(1, dtype=I32, device=gpu), torch.zeros(1, 36, dtype=F64, device=gpu))

    def call(o):
        _ok(_L().fgr_estimate_normals(_p(t), _p(to), len(tgt), 1, pr.LOOP_NORMAL_RADIUS, None, _p(ws_n),
                                      need_n, _p(o[0]), _p(o[1]), _st()), 'fgr_estimate_normals')
        _ok(_L().fgr_icp_plane(_p(s), _p(so), len(src), _p(t), _p(to), len(tgt), _p(o[0]), 1, len(src),
                               _p(po), r, 30, 1e-6, 1e-6, _p(ws), need, *(_p(x) for x in o[2:]), _st()),
            'fgr_icp_plane')

    eager = outs()
    call(eager)
    torch.cuda.synchronize()
    assert int(eager[6][0]) >= 3 and int(eager[7][0]) == pr.CONVERGED and int(eager[1][0]) > 900
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    cap = outs()
    with torch.cuda.stream(side):
        call(cap)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(cap)
    for x in cap:
        x.zero_()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, cap):
        assert bit_equal(x, y)
