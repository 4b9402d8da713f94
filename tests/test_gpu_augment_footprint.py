"""Memory footprint of fgr_augment_pairs (include/fgreg.h), called through ctypes with every
operand carved out of a guarded arena (tests/_arena.py): strided inputs with poisoned pad
columns (xyz rows of ld 4, a correspondence table of ld C + 3), guarded outputs, a workspace of
exactly fgr_augment_workspace_bytes bytes prefilled with 0x00 and with 0xFF. Each case runs clean
and poisoned (run_both) and the two results must be bit-identical; the clean one is held to
train_augment_host within one float32 ulp (tests/_augment.py)."""
import random

import numpy as np
import pytest
import torch

import _augment as A
from _arena import Arena, assert_both_equal, bit_equal, run_both
from fgreg import augment

pytestmark = pytest.mark.gpu
F32, I64, I32, U8 = torch.float32, torch.int64, torch.int32, torch.uint8
SIZES = [(300, 257), (64, 1), (513, 130)]         # (source, target) points of the three pairs
MAX_PTS = 280                                      # kept rows: 280 257 64 1 280 130 = 1012 = 4 * 253
N_CORR = [1100, 40, 0]                             # pair 0: two scan chunks; pair 2: none


def _L():
    from fgreg import _lib
    return _lib.load()


def _p(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope='module')
def batch():
    """Three synthetic pairs with their draws (small / source / swap, large / target, none /
    swap) and the host pipeline's outputs."""
    samples, draws = [], []
    modes = [('small', True, True), ('large', False, False), ('none', None, True)]
    for b, ((ns, nt), nc) in enumerate(zip(SIZES, N_CORR)):
        rng = np.random.default_rng(70 + b)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        pose = np.concatenate([q * np.sign(np.linalg.det(q)), rng.uniform(-1, 1, (3, 1))], 1)
        samples.append({
            'src_xyz': torch.from_numpy(rng.uniform(-3, 3, (ns, 3)).astype(np.float32)),
            'tgt_xyz': torch.from_numpy(rng.uniform(-3, 3, (nt, 3)).astype(np.float32)),
            'src_overlap': torch.from_numpy(rng.random(ns) < 0.5),
            'tgt_overlap': torch.from_numpy(rng.random(nt) < 0.5),
            'correspondences': torch.from_numpy(np.stack([rng.integers(0, ns, nc),
                                                          rng.integers(0, nt, nc)]).astype(np.int64)),
            'pose': torch.from_numpy(pose.astype(np.float32))})
        mode, source, swap = modes[b]
        torch.manual_seed(b)
        np.random.seed(b)
        random.seed(b)
        d = augment.draw_train_augment(ns, nt, mode, MAX_PTS)
        d['swap'] = swap
        if source is not None:
            d['perturb_source'] = source
        draws.append(d)
    host = [augment.train_augment_host(s, d, 0.005) for s, d in zip(samples, draws)]
    return samples, draws, host


def _call(ar, samples, draws, scale=0.005, short=0, corrs=None):
    """Packs the batch as fgreg.augment does, every operand in the arena -> (rc, outputs)."""
    from fgreg import _lib
    B = len(samples)
    ns = [len(s[k]) for s in samples for k in ('src_xyz', 'tgt_xyz')]
    perms = [np.asarray(d[k], np.int32) for d in draws for k in ('src_idx', 'tgt_idx')]
    ms = [len(p) for p in perms]
    corrs = corrs or [s['correspondences'] for s in samples]
    c_tot = sum(c.shape[1] for c in corrs)
    n_tot, m_tot = sum(ns), sum(ms)
    assert m_tot % 4 == 0                      # the overlap bytes are guarded in 32-bit words
    cum = lambda v: torch.tensor(np.concatenate([[0], np.cumsum(v)]), dtype=I64)
    flags = torch.zeros(B, dtype=I32)
    perturb = torch.zeros(B, 12)
    for b, d in enumerate(draws):
        if d['perturb'] is not None:
            perturb[b] = torch.from_numpy(d['perturb']).reshape(12)
            flags[b] = 1 | (2 if d['perturb_source'] else 0) | (4 if d['mode'] == 'small' else 0)
        flags[b] |= 8 if d['swap'] else 0
    xyz = ar.put(torch.cat([s[k] for s in samples for k in ('src_xyz', 'tgt_xyz')]), ld=4, name='xyz')
    ov = ar.put(torch.cat([s[k] for s in samples for k in ('src_overlap', 'tgt_overlap')]).to(U8),
                name='overlap')
    corr = ar.put(torch.cat(corrs, dim=1), ld=c_tot + 3, name='corr')
    noise = ar.put(torch.cat([d[k] * scale for d in draws for k in ('noise_src', 'noise_tgt')]),
                   name='noise')
    in_off, out_off = ar.put(cum(ns), name='in_off'), ar.put(cum(ms), name='out_off')
    corr_off = ar.put(cum([c.shape[1] for c in corrs]), name='corr_off')
    pose = ar.put(torch.stack([s['pose'].reshape(12) for s in samples]), name='pose')
    pert, fl = ar.put(perturb, name='perturb'), ar.put(flags, name='flags')
    perm = ar.put(torch.from_numpy(np.concatenate(perms)), name='perm')
    xyz_out = ar.matrix(m_tot, 3, 3, F32, 'out', name='xyz_out')
    ov_out = ar.vector(m_tot // 4, I32, 'out', name='overlap_out')
    corr_out = ar.matrix(2, c_tot, c_tot + 3, I64, 'out', name='corr_out', full=False)
    n_corr = ar.vector(B, I32, 'out', name='n_corr')
    pose_out = ar.matrix(B, 12, 12, F32, 'out', name='pose_out')
    nb = _lib._sz(0)
    _lib.check(_L().fgr_augment_workspace_bytes(n_tot, B, nb), 'fgr_augment_workspace_bytes')
    assert nb.value == B * 2 * 12 * 8 + n_tot * 4
    ws = ar.bytes(nb.value, name='ws')
    rc = _L().fgr_augment_pairs(_p(xyz), 4, _p(in_off), n_tot, _p(ov), _p(corr), c_tot + 3,
                                _p(corr_off), _p(pose), _p(pert), _p(fl), _p(perm), _p(out_off),
                                max(ms), _p(noise), B, _p(xyz_out), _p(ov_out), _p(corr_out),
                                _p(n_corr), _p(pose_out), _p(ws), nb.value - short,
                                torch.cuda.current_stream().cuda_stream)
    return rc, (xyz_out, ov_out.view(U8), corr_out, n_corr, pose_out), ws


def _unpack(outs, draws, b):
    """Pair b's sample dict out of the packed outputs (post-swap order)."""
    xyz_out, ov_out, corr_out, n_corr, pose_out = (t.cpu() for t in outs)
    ms = [len(d[k]) for d in draws for k in ('src_idx', 'tgt_idx')]
    o = sum(ms[:2 * b])
    m_s, m_t = (ms[2 * b + 1], ms[2 * b]) if draws[b]['swap'] else (ms[2 * b], ms[2 * b + 1])
    co = sum(N_CORR[:b])
    return {'src_xyz': xyz_out[o:o + m_s], 'tgt_xyz': xyz_out[o + m_s:o + m_s + m_t],
            'src_overlap': ov_out[o:o + m_s].bool(), 'tgt_overlap': ov_out[o + m_s:o + m_s + m_t].bool(),
            'correspondences': corr_out[:, co:co + max(int(n_corr[b]), 0)],
            'pose': pose_out[b].reshape(3, 4)}


def test_augment_pairs_footprint(gpu, batch):
    samples, draws, host = batch

    def run(ar):
        rc, outs, _ = _call(ar, samples, draws)
        assert rc == 0, _L().fgr_last_error()
        return outs
    clean, poisoned = run_both(run, gpu)
    assert_both_equal(clean, poisoned)
    assert bool((clean[1] <= 1).all())                   # every overlap byte was written
    assert clean[3].tolist() == [h['correspondences'].shape[1] for h in host]
    for b in range(len(samples)):
        A.check_vs_host(_unpack(clean, draws, b), host[b], f'pair {b}')


def test_out_of_range_correspondence_is_reported_not_read(gpu, batch):
    """A source index one past its cloud in pair 1 (the packed tables go on after it, so the
    address is allocated memory): n_corr[1] = -1, no guard byte touched, the other pairs and
    every other output as in the clean run."""
    samples, draws, host = batch
    bad = [s['correspondences'].clone() for s in samples]
    bad[1][0, 7] = SIZES[1][0]
    outs = []
    for corrs in (None, bad):
        ar = Arena(gpu, poison=True)
        rc, out, _ = _call(ar, samples, draws, corrs=corrs)
        assert rc == 0, _L().fgr_last_error()
        torch.cuda.synchronize()
        ar.check()
        outs.append(tuple(t.clone() for t in out))
    good, got = outs
    assert got[3].tolist() == [good[3][0].item(), -1, good[3][2].item()]
    for i in (0, 1, 4):                                   # xyz, overlap, pose: all pairs
        assert bit_equal(good[i], got[i]), i
    n0 = N_CORR[0]
    assert bit_equal(good[2][:, :n0], got[2][:, :n0])     # pair 0's correspondences
    for b in (0, 2):
        A.check_vs_host(_unpack(got, draws, b), host[b], f'pair {b}')


def test_augment_pairs_refuses_short_workspace(gpu, batch):
    samples, draws, _ = batch
    ar = Arena(gpu, poison=True)
    rc, outs, ws = _call(ar, samples, draws, short=4)
    torch.cuda.synchronize()
    assert rc != 0
    msg = _L().fgr_last_error()
    assert b'fgr_augment_pairs' in msg and b'workspace' in msg
    for r in ar.regions:
        r.full = False
    ar.check()
    assert bool(torch.isnan(outs[0]).all()) and bool((ws == 0xFF).all())
