"""CPU: the host side of the 3DMatch / MCD training augmentations (fgreg/augment.py) against
the reference's own RigidPerturb -> Jitter -> ShufflePoints -> RandomSwap objects, recorded in
tests/golden/threedmatch_augment.npz (golden/make_golden_augment.py): the draws taken from the
three global generators, and the float64 host pipeline that checks the kernels."""
import random

import numpy as np
import pytest
import torch

import _augment as A
from fgreg import augment

CASES, TORCH_VERSION = A.cases()
IDS = [f"{k}-{c['mode']}" for k, c in enumerate(CASES)]


def _seed(s):
    torch.manual_seed(s)            # setup_seed, cvhelpers/torch_helpers.py:86-93
    np.random.seed(s)
    random.seed(s)


def test_fixture_covers_every_branch():
    seen = {(c['mode'], c['draws']['perturb_source'], c['draws']['swap'],
             c['max_pts'] < max(len(c['sample']['src_xyz']), len(c['sample']['tgt_xyz'])))
            for c in CASES}
    assert {m for m, *_ in seen} == {'none', 'small', 'large'}
    assert {(m, s) for m, s, *_ in seen} >= {('small', True), ('small', False), ('large', True),
                                             ('large', False)}
    assert {s for _, _, s, _ in seen} == {True, False}
    assert {t for *_, t in seen} == {True, False}
    assert any(not c['shuffle'] for c in CASES)


@pytest.mark.parametrize('k', range(len(CASES)), ids=IDS)
def test_draws_reproduce_the_reference(k):
    """Seeded as the reference is, draw_train_augment takes the reference's sample: the
    perturbation bit for bit in float32, both flags and both permutations exactly, and the
    noise exactly under the torch version that recorded it."""
    c = CASES[k]
    want = c['draws']
    _seed(c['seed'])
    got = augment.draw_train_augment(len(c['sample']['src_xyz']), len(c['sample']['tgt_xyz']),
                                     c['mode'], c['max_pts'], c['shuffle'])
    assert got['mode'] == c['mode']
    if c['mode'] == 'none':
        assert got['perturb'] is None and got['perturb_source'] is None
    else:
        assert got['perturb'].dtype == np.float32 and got['perturb'].shape == (3, 4)
        assert got['perturb'].tobytes() == want['perturb'].tobytes()
        assert got['perturb_source'] is want['perturb_source']
    assert got['swap'] is want['swap']
    for key in ('src_idx', 'tgt_idx'):
        assert np.array_equal(got[key], want[key]), key
    for key in ('noise_src', 'noise_tgt'):
        assert got[key].dtype == torch.float32 and got[key].shape == want[key].shape
    if torch.__version__ == TORCH_VERSION:
        for key in ('noise_src', 'noise_tgt'):
            assert torch.equal(got[key], want[key]), key


def test_draws_none_takes_nothing_for_the_perturbation():
    """'none' returns before RigidPerturb's draws: the first random.random() is the swap's."""
    _seed(7)
    d = augment.draw_train_augment(5, 6, 'none', shuffle=False)
    random.seed(7)
    assert d['swap'] is (random.random() > 0.5)
    assert np.array_equal(d['src_idx'], np.arange(5)) and np.array_equal(d['tgt_idx'], np.arange(6))
    with pytest.raises(ValueError):
        augment.draw_train_augment(5, 6, 'medium')


@pytest.mark.parametrize('k', range(len(CASES)), ids=IDS)
def test_host_pipeline_vs_reference(k):
    """train_augment_host on the recorded draws against the reference's outputs: integer fields
    exact, float fields within 16 * 2^-24 * S."""
    c = CASES[k]
    got = augment.train_augment_host(c['sample'], c['draws'], c['scale'])
    A.check_vs_reference(got, c['ref'], c['sample'], f'case {k}')
    assert got['idx'] == k and got['overlap_p'] == c['sample']['overlap_p']
    assert list(got) == ['src_xyz', 'tgt_xyz', 'src_overlap', 'tgt_overlap', 'correspondences',
                         'pose', 'idx', 'src_path', 'tgt_path', 'overlap_p']


def test_host_pipeline_end_to_end_from_the_seed():
    """Seed -> draws -> host pipeline, nothing recorded in between, against the reference."""
    for k, c in enumerate(CASES):
        if torch.__version__ != TORCH_VERSION and c['scale'] != 0:
            continue
        _seed(c['seed'])
        d = augment.draw_train_augment(len(c['sample']['src_xyz']), len(c['sample']['tgt_xyz']),
                                       c['mode'], c['max_pts'], c['shuffle'])
        got = augment.train_augment_host(c['sample'], d, c['scale'])
        A.check_vs_reference(got, c['ref'], c['sample'], f'case {k}')


def test_gpu_pipeline_has_no_cpu_fallback():
    c = CASES[0]
    with pytest.raises(ValueError, match='GPU'):
        augment.train_augment_gpu([c['sample']], draws=[c['draws']], device='cpu')


def test_samples_with_corr_xyz_are_refused():
    """RigidPerturb / RandomSwap also move 'corr_xyz' where a sample carries it; this chain
    does not, so such a sample is an error, not a silent omission."""
    s = dict(CASES[0]['sample'], corr_xyz=torch.zeros(4, 6))
    with pytest.raises(NotImplementedError, match='corr_xyz'):
        augment.train_augment_host(s, CASES[0]['draws'], 0.005)
