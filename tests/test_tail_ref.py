"""CPU checks of tests/_tail_ref.py, the fp64 references and input generators that
tests/test_gpu_tail_kernels.py holds the loss / pose kernels to:

1. the references are pinned to what the project already trusts: oracle/loss_oracle.py on the
   golden loss fixture (1e-6 relative: the oracle is float32, that is its own rounding), the
   reference project's Procrustes outputs (tests/golden/procrustes.npz, the bound of
   test_gpu_kernels.test_procrustes_vs_reference) and loss_oracle.pose_errors;
2. the conditions the generators promise hold for every parametrised case of the GPU file:
   the margins around r_p / r_n, a kept row in every pair meant to be finite, a selected row
   and column in the circle cases, exactness of the float32 distance form on the lattice.
"""
import functools

import numpy as np
import pytest
import torch

import _tail_ref as tr
import loss_oracle as lo
from conftest import golden, loss_fixture

TOL = 1e-4          # test_gpu_kernels.TOL, the Procrustes bound


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


@functools.lru_cache(maxsize=None)
def _fixture():
    cfg, pred, batch, losses, metrics, _, W, W_un = loss_fixture('cpu')
    B = len(pred['src_kp'])
    a_xyz = [lo.rigid_apply(batch['pose'][b], pred['src_kp'][b]) for b in range(B)]
    return cfg, pred, batch, W_un, a_xyz, B


def test_infonce_rows_reduces_to_oracle():
    cfg, pred, batch, W_un, a_xyz, B = _fixture()
    A, P = pred['src_feat_un'], pred['tgt_feat_un']
    ws = torch.triu(W_un) + torch.triu(W_un).t()
    a_off = tr.offsets([len(a) for a in A])
    p_off = tr.offsets([len(p) for p in P])
    logits = ((torch.cat(A) @ ws) @ torch.cat(P).t()).double().numpy()
    _, mask, _, got = tr.infonce_rows(logits, torch.cat(a_xyz), torch.cat(pred['tgt_kp']), a_off,
                                      p_off, cfg.r_p, cfg.r_n)
    want = float(torch.stack([lo.infonce_pair(W_un, A[b], P[b], a_xyz[b], pred['tgt_kp'][b],
                                              cfg.r_p, cfg.r_n) for b in range(B)]).mean())
    assert mask.any() and _rel(got, want) <= 1e-6, (got, want)


def test_circle_lines_reduces_to_oracle():
    cfg, pred, batch, _, a_xyz, B = _fixture()
    A, P = pred['src_feat_un'], pred['tgt_feat_un']
    a_off = tr.offsets([len(a) for a in A])
    p_off = tr.offsets([len(p) for p in P])
    _, got = tr.circle_lines(torch.cat(A), torch.cat(P), torch.cat(a_xyz),
                             torch.cat(pred['tgt_kp']), a_off, p_off, cfg.r_p, cfg.r_n)
    want = float(torch.stack([lo.circle_pair(A[b], P[b], a_xyz[b], pred['tgt_kp'][b], cfg.r_p,
                                             cfg.r_n) for b in range(B)]).mean())
    assert np.isfinite(want) and _rel(got, want) <= 1e-6, (got, want)


def test_infonce_dlogits_is_the_softmax_form():
    """Autograd of the restatement against the closed form of include/fgreg.h:
    g w_i (softmax_ij - [j == positive]) on the row's pair block, 0 elsewhere."""
    x = tr.infonce_inputs('lattice-p1-a0')
    args = (x['logits'], x['axyz'], x['pxyz'], x['a_off'], x['p_off'])
    pos, mask, _, _ = tr.infonce_rows(*args)
    dl = tr.infonce_dlogits(*args, g=tr.INFONCE_G)
    n_pairs = len(x['a_off']) - 1
    for i in range(len(pos)):
        b = int(np.searchsorted(x['a_off'], i, 'right') - 1)
        w = mask[i] / (mask[x['a_off'][b]:x['a_off'][b + 1]].sum() * n_pairs)
        p0, p1 = int(x['p_off'][b]), int(x['p_off'][b + 1])
        d = tr.point_dist(x['axyz'][i:i + 1], x['pxyz'][p0:p1])[0]
        live = ~(d < tr.R_N)
        live[pos[i] - p0] = True
        l = np.where(live, x['logits'][i, p0:p1].astype(np.float64), -np.inf)
        sm = np.exp(l - l.max())
        sm /= sm.sum()
        sm[pos[i] - p0] -= 1.0
        want = np.zeros(x['n_cols'])
        want[p0:p1] = tr.INFONCE_G * w * sm
        assert np.abs(dl[i] - want).max() <= 1e-12, i


@pytest.mark.parametrize('case', ['regular', 'reflection', 'allzero', 'threshold'])
def test_kabsch_vs_reference(case):
    g = golden('procrustes')
    a, b, w = (g[f'{case}_{k}'] for k in 'abw')
    for thr, key in ((0.85, 'fast'), (-1.0, 'full')):
        want = g[f'{case}_{key}']
        got = np.stack([tr.kabsch(a[i], b[i], w[i], thr) for i in range(len(a))])
        assert np.abs(got[..., :3] - want[..., :3]).max() < TOL
        assert np.abs(got[..., 3] - want[..., 3]).max() < TOL * max(1.0, np.abs(want[..., 3]).max())


def test_se3_compare_vs_oracle():
    rng = np.random.default_rng(5)
    gt = np.stack([tr.random_pose(rng) for _ in range(4)]).astype(np.float32)
    pred = np.stack([[tr.random_pose(rng, 40.0) for _ in range(4)] for _ in range(3)])
    pred = np.concatenate([pred[..., :3] @ gt[None, ..., :3].astype(np.float64),
                           pred[..., 3:]], -1).astype(np.float32)
    c, deg, trans = tr.se3_compare(pred, gt)
    rot, tn = lo.pose_errors(torch.from_numpy(pred), torch.from_numpy(gt))
    assert np.abs(deg - rot.numpy()).max() <= 1e-3
    assert np.abs(c - np.cos(np.radians(rot.numpy().astype(np.float64)))).max() <= 2e-6
    assert np.abs(trans - tn.numpy()).max() <= 1e-5 * max(1.0, float(tn.max()))


def _cdist_mm_f32(a, p):
    """The kernels' float32 distance: sqrt(max(-2 a.p + |a|^2 + |p|^2, 1e-30)), the five terms
    accumulated in that order (csrc/loss.hip cdist_mm; no fused multiply-add matters where
    every product is exact)."""
    f = np.float32
    a, p = a.astype(f)[:, None, :], p.astype(f)[None, :, :]
    a2 = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
    p2 = (p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2]
    t = (f(-2) * a[..., 0]) * p[..., 0]
    t = t + (f(-2) * a[..., 1]) * p[..., 1]
    t = t + (f(-2) * a[..., 2]) * p[..., 2]
    t = (t + a2) + p2
    return np.sqrt(np.maximum(t, f(1e-30)))


def test_lattice_distance_form_is_exact():
    axyz, pxyz = tr.lattice_clouds(7, [200], [300])
    d32 = _cdist_mm_f32(axyz, pxyz)
    d64 = tr.point_dist(axyz, pxyz)
    nz = d64 > 0                                   # 0 becomes sqrt(1e-30): either side of nothing
    assert np.array_equal(d32[nz], d64[nz].astype(np.float32)) and d32[~nz].max() < 1e-14
    assert np.abs(d64 - tr.R_P).min() >= 0.005 and np.abs(d64 - tr.R_N).min() >= 0.006


def _pairs(x):
    for b in range(len(x['a_off']) - 1):
        yield b, slice(*map(int, x['a_off'][b:b + 2])), slice(*map(int, x['p_off'][b:b + 2]))


@pytest.mark.parametrize('name', list(tr.INFONCE_CASES))
def test_infonce_case_conditions(name):
    x = tr.infonce_inputs(name)                    # the continuous generator asserts its own
    pos, mask, rl, s = tr.infonce_rows(x['logits'], x['axyz'], x['pxyz'], x['a_off'], x['p_off'])
    for b, sa, sp in _pairs(x):
        if sa.stop == sa.start or sp.stop == sp.start:
            continue
        d = tr.point_dist(x['axyz'][sa], x['pxyz'][sp])
        assert np.abs(d - tr.R_P).min() > 1e-4 and np.abs(d - tr.R_N).min() > 1e-4
        if x['kind'] == 'lattice':
            assert np.abs(d - tr.R_P).min() >= 0.005 and np.abs(d - tr.R_N).min() >= 0.006
        elif d.shape[1] > 1:
            srt = np.sort(d, 1)
            assert (srt[:, 1] - srt[:, 0]).min() > 1e-5
        if b in x['finite']:
            assert mask[sa].any(), f'pair {b}: no kept row'
        if x['modes'][b] == 'far':
            assert not mask[sa].any() and not (d < tr.R_N).any()
        if x['modes'][b] == 'inside':
            assert (d < tr.R_N).all() and np.abs(rl[sa]).max() == 0.0
    n_pairs = len(x['a_off']) - 1
    assert np.isfinite(s) == (len(x['finite']) == n_pairs)
    assert np.isfinite(x['logits'][:, :int(x['p_off'][-1])]).all()
    if name == 'pm80':
        assert np.abs(x['logits'][:, :int(x['p_off'][-1])]).max() == np.float32(80.0)


def test_lattice_cases_keep_and_tie():
    """Over the lattice cases' finite pairs: about 80 % of the rows kept, about a quarter with an
    exactly tied nearest positive (so the lowest-index rule is exercised)."""
    kept = tied = rows = 0
    for name in tr.INFONCE_CASES:
        x = tr.infonce_inputs(name)
        if x['kind'] != 'lattice' or set(x['modes']) != {'near'}:
            continue
        _, mask, _, _ = tr.infonce_rows(x['logits'], x['axyz'], x['pxyz'], x['a_off'], x['p_off'])
        for b, sa, sp in _pairs(x):
            if b in x['finite']:
                d = tr.point_dist(x['axyz'][sa], x['pxyz'][sp])
                tied += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
                kept += int(mask[sa].sum())
                rows += sa.stop - sa.start
    assert 0.7 <= kept / rows <= 0.9 and 0.15 <= tied / rows <= 0.4, (kept, tied, rows)


@pytest.mark.parametrize('name', list(tr.CIRCLE_CASES))
def test_circle_case_conditions(name):
    x = tr.circle_inputs(name)
    lines, s = tr.circle_lines(x['af'], x['pf'], x['axyz'], x['pxyz'], x['a_off'], x['p_off'])
    assert np.isfinite(s) == x['finite']
    fd = np.concatenate([f.ravel() for f in tr.pair_cdist(x['af'], x['pf'], x['a_off'], x['p_off'])])
    if name != 'empty-side':
        assert (fd < tr.CIRCLE_POS).any() and (fd > tr.CIRCLE_NEG).any()     # both margins
    for b, (row, rs, col, cs) in enumerate(lines):
        ok = rs.any() and cs.any()
        if x['finite']:
            assert ok, f'pair {b}: nothing selected'
            # one line weighs at least 1/8 of one of its means in the small pairs
            assert name != 'small' or min(rs.sum(), cs.sum()) <= 8
    if name == 'long':                             # selected lines in the reduction's last wave
        assert lines[0][1][960:].any() and lines[1][3][960:].any()
    if name == 'mix':                              # NaN by the (1, 1) pair alone
        assert [bool(l[1].any() and l[3].any()) for l in lines] == [False, True, True, True, True]
    if name == 'no-negative':
        assert lines[0][1].any() and lines[0][3].any() and not lines[1][1].any()
