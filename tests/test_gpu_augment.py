"""GPU: the 3DMatch / MCD training augmentations (fgreg/augment.py over csrc/augment.hip,
fgr_augment_pairs) against train_augment_host, the float64 chain with the same draws -- itself
pinned to the reference's transform objects by tests/test_augment.py -- within one float32
ulp element by element, integer fields exact; and the fixture's cases against the reference's
own outputs within 16 * 2^-24 * S (tests/_augment.py states both bounds)."""
import os
import random

import numpy as np
import pytest
import torch

import _augment as A
from _arena import bit_equal
from fgreg import augment

pytestmark = pytest.mark.gpu


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


def _sample(seed, n_src, n_tgt, n_corr, idx=0):
    """A synthetic sample dict (CPU tensors): clouds in a 6 m box, a random rigid pose, random
    overlap flags and n_corr random correspondence columns."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    pose = np.concatenate([q, rng.uniform(-1, 1, (3, 1))], 1).astype(np.float32)
    corr = np.stack([rng.integers(0, n_src, n_corr), rng.integers(0, n_tgt, n_corr)])
    return {'src_xyz': torch.from_numpy(rng.uniform(-3, 3, (n_src, 3)).astype(np.float32)),
            'tgt_xyz': torch.from_numpy(rng.uniform(-3, 3, (n_tgt, 3)).astype(np.float32)),
            'src_overlap': torch.from_numpy(rng.random(n_src) < 0.4),
            'tgt_overlap': torch.from_numpy(rng.random(n_tgt) < 0.6),
            'correspondences': torch.from_numpy(corr.astype(np.int64)),
            'pose': torch.from_numpy(pose), 'idx': idx, 'src_path': f's{idx}.pth',
            'tgt_path': f't{idx}.pth', 'overlap_p': 0.25 + idx}


def _draws(seed, s, mode, source=None, swap=None, max_pts=30000, shuffle=True):
    """draw_train_augment under a seed, with the two flags forced where given."""
    _seed(seed)
    d = augment.draw_train_augment(len(s['src_xyz']), len(s['tgt_xyz']), mode, max_pts, shuffle)
    if source is not None and mode != 'none':
        d['perturb_source'] = source
    if swap is not None:
        d['swap'] = swap
    return d


def _check(gpu, samples, draws, scale=0.005, what=''):
    out = augment.train_augment_gpu(samples, augment_noise=scale, draws=draws, device=gpu)
    assert len(out) == len(samples)
    for b, (o, s, d) in enumerate(zip(out, samples, draws)):
        assert all(o[k].is_cuda for k in A.FLOAT_KEYS + A.EXACT_KEYS)
        A.check_vs_host(o, augment.train_augment_host(s, d, scale), f'{what} pair {b}')
    return out


@pytest.mark.parametrize('swap', [False, True])
@pytest.mark.parametrize('source', [True, False])
@pytest.mark.parametrize('mode', ['none', 'small', 'large'])
def test_every_branch(gpu, mode, source, swap):
    s = _sample(1, 1000, 900, 400)
    _check(gpu, [s], [_draws(2, s, mode, source, swap)], what=f'{mode} {source} {swap}')


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1023, 1024, 1025])
def test_wave_and_chunk_edges(gpu, n):
    """Cloud sizes at the wave (64), the gather tile (256 | 1024) and the scan chunk (1024)
    edges, as source and as target, with as many correspondence columns."""
    for k, (ns, nt) in enumerate([(n, 130), (130, n)]):
        s = _sample(10 + n, ns, nt, n)
        _check(gpu, [s], [_draws(n + k, s, 'small', bool(k), bool(k))], what=f'n {n}')


def test_ragged_batch(gpu):
    """B = 3 in one call, every pair with its own sizes, mode and flags."""
    samples = [_sample(20, 1000, 300, 500, 0), _sample(21, 65, 1025, 70, 1), _sample(22, 1, 64, 9, 2)]
    draws = [_draws(3, samples[0], 'small', False, True), _draws(4, samples[1], 'large', True, False),
             _draws(5, samples[2], 'none', None, True, max_pts=40)]
    out = _check(gpu, samples, draws, what='ragged')
    assert [o['idx'] for o in out] == [0, 1, 2]
    assert out[0]['src_path'] == 't0.pth' and out[1]['src_path'] == 's1.pth'


def test_truncation_drops_columns(gpu):
    """max_pts 700 of 1000: ShufflePoints truncates, correspondences to cut points go."""
    s = _sample(30, 1000, 1000, 600)
    d = _draws(6, s, 'small', True, True, max_pts=700)
    out = _check(gpu, [s], [d], what='max_pts 700')[0]
    assert out['src_xyz'].shape == (700, 3) and 0 < out['correspondences'].shape[1] < 600


@pytest.mark.parametrize('n_corr', [0, 2500])
def test_correspondence_counts(gpu, n_corr):
    """0 columns (a null table) and 2500: three scan chunks with a partial last one."""
    s = _sample(40, 700, 650, n_corr)
    out = _check(gpu, [s], [_draws(7, s, 'large', False, True, max_pts=600)], what=f'{n_corr}')[0]
    assert out['correspondences'].shape[0] == 2
    assert (out['correspondences'].shape[1] > 0) == (n_corr > 0)


def test_all_correspondences_dropped(gpu):
    s = _sample(41, 1000, 1000, 300)
    s['correspondences'][0] = 700 + s['correspondences'][0] % 300      # only rows that are cut
    out = _check(gpu, [s], [_draws(8, s, 'small', True, False, max_pts=700, shuffle=False)])[0]
    assert out['correspondences'].shape == (2, 0)


@pytest.mark.parametrize('scale', [0.005, 0.0])
def test_no_shuffle_and_no_noise(gpu, scale):
    """shuffle=False (identity permutations, truncated); augment_noise = 0 passes no noise."""
    s = _sample(42, 900, 1000, 400)
    _check(gpu, [s], [_draws(9, s, 'small', False, False, max_pts=950, shuffle=False)], scale)
    _check(gpu, [s], [_draws(9, s, 'none', None, True)], scale)


CASES, _ = A.cases()


@pytest.mark.parametrize('k', range(len(CASES)), ids=[f"{k}-{c['mode']}" for k, c in enumerate(CASES)])
def test_fixture_cases_vs_reference(gpu, k):
    """The reference's own outputs (threedmatch_augment.npz), with the recorded draws."""
    c = CASES[k]
    out = augment.train_augment_gpu([c['sample']], augment_noise=c['scale'], draws=[c['draws']],
                                    device=gpu)[0]
    A.check_vs_reference(out, c['ref'], c['sample'], f'case {k}')
    assert out['idx'] == k and out['overlap_p'] == c['sample']['overlap_p']


def test_fixture_batch_from_the_seed(gpu):
    """draws=None: one set per sample, in sample order, from the global generators -- the
    first case's seed reproduces the reference's sample end to end."""
    c = CASES[0]
    _seed(c['seed'])
    out = augment.train_augment_gpu([c['sample']], c['mode'], c['scale'], c['max_pts'],
                                    c['shuffle'], device=gpu)[0]
    A.check_vs_reference(out, c['ref'], c['sample'], 'seeded')


def test_deterministic(gpu):
    samples = [_sample(50, 1025, 1000, 1500, 0), _sample(51, 300, 700, 200, 1)]
    draws = [_draws(11, samples[0], 'small', True, True, max_pts=900),
             _draws(12, samples[1], 'small', False, False)]
    a = augment.train_augment_gpu(samples, draws=draws, device=gpu)
    b = augment.train_augment_gpu(samples, draws=draws, device=gpu)
    for x, y in zip(a, b):
        for k in A.FLOAT_KEYS + A.EXACT_KEYS:
            assert bit_equal(x[k], y[k]), k


def test_input_kinds_agree(gpu):
    """Host NumPy arrays, host tensors and device tensors give the same result."""
    s = _sample(60, 800, 750, 300)
    d = _draws(13, s, 'small', True, True, max_pts=600)
    tensor_keys = A.FLOAT_KEYS + A.EXACT_KEYS
    kinds = [{k: (v.numpy() if k in tensor_keys else v) for k, v in s.items()}, s,
             {k: (v.to(gpu) if k in tensor_keys else v) for k, v in s.items()}]
    outs = [augment.train_augment_gpu([x], draws=[d], device=gpu)[0] for x in kinds]
    A.check_vs_host(outs[1], augment.train_augment_host(s, d, 0.005), 'host tensors')
    for o in (outs[0], outs[2]):
        for k in tensor_keys:
            assert torch.equal(o[k], outs[1][k]), k


def test_bad_permutation_is_refused(gpu):
    s = _sample(61, 100, 100, 10)
    d = _draws(14, s, 'none')
    d['src_idx'] = np.array([0, 1, 1])
    with pytest.raises(ValueError, match='distinct'):
        augment.train_augment_gpu([s], draws=[d], device=gpu)
    d['src_idx'] = np.array([0, 100])
    with pytest.raises(ValueError, match='distinct'):
        augment.train_augment_gpu([s], draws=[d], device=gpu)


def test_loader_with_transforms(gpu, tmp_path):
    """ThreeDMatchPairs(..., transforms=TrainAugment(...)) on temporary fragment files: the
    host pipeline applied to the un-augmented sample; without transforms, today's output."""
    from fgreg import data
    from fgreg.synthetic import lowoverlap_pair
    infos = {'rot': [], 'trans': [], 'src': [], 'tgt': [], 'overlap': []}
    for i in range(2):
        src, tgt, pose, f = lowoverlap_pair(i, n_points=3000, overlap=(0.5, 0.7))
        sp, tp = f'frag_{i}_a.npy', f'frag_{i}_b.npy'
        np.save(os.path.join(tmp_path, sp), src)
        np.save(os.path.join(tmp_path, tp), tgt[:2500])
        infos['rot'].append(pose[:, :3].astype(np.float64))
        infos['trans'].append(pose[:, 3:].astype(np.float64))
        infos['src'].append(sp)
        infos['tgt'].append(tp)
        infos['overlap'].append(f)
    plain = data.ThreeDMatchPairs(str(tmp_path), infos, overlap_radius=0.15, device=gpu)
    aug = data.ThreeDMatchPairs(str(tmp_path), infos, overlap_radius=0.15, device=gpu,
                                transforms=augment.TrainAugment('small', 0.005, max_pts=2800))
    again = data.ThreeDMatchPairs(str(tmp_path), infos, overlap_radius=0.15, device=gpu,
                                  transforms=None)
    for i in range(2):
        base = plain[i]
        assert base['correspondences'].shape[1] > 50
        _seed(100 + i)
        got = aug[i]
        _seed(100 + i)
        d = augment.draw_train_augment(3000, 2500, 'small', 2800)
        A.check_vs_host(got, augment.train_augment_host(base, d, 0.005), f'loader {i}')
        assert got['src_xyz'].is_cuda and got['src_xyz'].shape[0] in (2800, 2500)
        same = again[i]
        assert list(same) == list(base)
        for k, v in base.items():
            assert torch.equal(same[k], v) if torch.is_tensor(v) else same[k] == v, k


def test_one_training_step(gpu):
    """A collated augmented B = 2 batch through model.train() forward, compute_loss and
    backward: a finite loss and a finite gradient for every trainable parameter."""
    import fgreg
    import fgreg.config as fc
    from conftest import is_trainable
    from fgreg.loss import compute_loss_train
    from fgreg.synthetic import make_batch
    torch.manual_seed(0)
    np.random.seed(0)
    model = fgreg.RegTR(fc.get('modelnet')).to(gpu).train()
    src, tgt, pose = make_batch('modelnet', 2)
    samples = []
    for b in range(2):
        n = min(len(src[b]), len(tgt[b]))
        samples.append({'src_xyz': torch.from_numpy(src[b]).to(gpu),
                        'tgt_xyz': torch.from_numpy(tgt[b]).to(gpu),
                        'src_overlap': torch.ones(len(src[b]), dtype=torch.bool),
                        'tgt_overlap': torch.arange(len(tgt[b])) % 3 != 0,
                        'correspondences': torch.arange(n // 2).repeat(2, 1),
                        'pose': torch.from_numpy(np.asarray(pose[b], np.float32)), 'idx': b})
    _seed(3)
    batch = augment.train_batch_gpu(samples, perturb_pose='small', augment_noise=0.005,
                                    max_pts=700, device=gpu)
    assert batch['pose'].shape == (2, 3, 4) and batch['pose'].is_cuda
    assert [len(x) for x in batch['src_xyz']] == [700, 700] and batch['idx'] == [0, 1]
    out = model(batch)
    loss = compute_loss_train(model, out, batch)['total']
    loss.backward()
    assert bool(torch.isfinite(loss.detach()))
    n = 0
    for k, p in model.named_parameters():
        if is_trainable(k):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
            n += 1
    assert n > 100
