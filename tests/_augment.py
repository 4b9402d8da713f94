"""Shared by tests/test_augment.py and tests/test_gpu_augment*.py: the fixture's cases
(tests/golden/threedmatch_augment.npz, written by golden/make_golden_augment.py from the
reference's own transform objects) and the two float comparisons. Not a conftest: imported by
the tests that use it.

  S = max(1, largest |coordinate| or |pose entry| of the pair)
  GPU vs train_augment_host   |a - b| <= 2^-23 max(|b|, 2^-126) element by element: both round
                              one float64 result, whose summation order may flip that rounding
  anything vs the reference   |a - b| <= 16 * 2^-24 * S: the reference computes in float32
                              throughout; 16 counts the roundings along its chain (mean, three
                              3x3 compositions, transform, noise add)
Masks, correspondences, paths, dtypes and shapes are always exact.
"""
import functools

import numpy as np
import torch

from conftest import golden

FLOAT_KEYS = ('src_xyz', 'tgt_xyz', 'pose')
EXACT_KEYS = ('src_overlap', 'tgt_overlap', 'correspondences')
DTYPES = {'src_xyz': torch.float32, 'tgt_xyz': torch.float32, 'pose': torch.float32,
          'src_overlap': torch.bool, 'tgt_overlap': torch.bool, 'correspondences': torch.int64}


@functools.lru_cache(maxsize=None)
def cases():
    """-> list of dicts: sample (CPU tensors), draws (as draw_train_augment returns them), the
    reference's outputs (numpy), seed, mode, scale, max_pts, shuffle; and the torch version."""
    g = golden('threedmatch_augment')
    out = []
    for k in range(int(g['n_cases'])):
        p = f'c{k}.'
        sample = {key: torch.from_numpy(g[p + 'in.' + key]) for key in
                  ('src_xyz', 'tgt_xyz', 'src_overlap', 'tgt_overlap', 'correspondences', 'pose')}
        sample.update(idx=k, src_path=f'src_{k}', tgt_path=f'tgt_{k}',
                      overlap_p=float(g[p + 'in.overlap_p']))
        mode = str(g[p + 'mode'])
        draws = {'mode': mode, 'perturb': None, 'perturb_source': None,
                 'noise_src': torch.from_numpy(g[p + 'draw.noise_src']),
                 'noise_tgt': torch.from_numpy(g[p + 'draw.noise_tgt']),
                 'src_idx': g[p + 'draw.src_idx'].astype(np.int64),
                 'tgt_idx': g[p + 'draw.tgt_idx'].astype(np.int64),
                 'swap': bool(g[p + 'draw.swap'])}
        if mode != 'none':
            draws['perturb'] = g[p + 'draw.perturb']
            draws['perturb_source'] = bool(g[p + 'draw.perturb_source'])
        ref = {key: g[p + 'out.' + key] for key in FLOAT_KEYS + EXACT_KEYS}
        ref['src_path'], ref['tgt_path'] = ((f'tgt_{k}', f'src_{k}') if draws['swap']
                                            else (f'src_{k}', f'tgt_{k}'))
        out.append(dict(sample=sample, draws=draws, ref=ref, seed=int(g[p + 'seed']), mode=mode,
                        scale=float(g[p + 'scale']), max_pts=int(g[p + 'max_pts']),
                        shuffle=bool(g[p + 'shuffle'])))
    return out, str(g['torch_version'])


def _a(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def scale_of(sample):
    return max(1.0, *(float(np.abs(_a(sample[k])).max()) for k in FLOAT_KEYS))


def check_structure(got, want):
    """Keys' dtypes and shapes, the integer fields and the paths: exact."""
    for k in FLOAT_KEYS + EXACT_KEYS:
        assert torch.is_tensor(got[k]) and got[k].dtype == DTYPES[k], (k, got[k].dtype)
        assert tuple(got[k].shape) == tuple(_a(want[k]).shape), (k, got[k].shape)
    for k in EXACT_KEYS:
        assert np.array_equal(_a(got[k]), _a(want[k])), k
    for k in ('src_path', 'tgt_path'):
        if k in want:
            assert got[k] == want[k], k


def check_vs_reference(got, ref, sample, what=''):
    """Against the reference's float32 chain: <= 16 * 2^-24 * S."""
    check_structure(got, ref)
    bound = 16 * 2.0 ** -24 * scale_of(sample)
    for k in FLOAT_KEYS:
        err = float(np.abs(_a(got[k]).astype(np.float64) - _a(ref[k]).astype(np.float64)).max())
        print(f'{what} {k}: max err {err / (2.0 ** -24 * scale_of(sample)):.3f} x 2^-24 S')
        assert err <= bound, (what, k, err, bound)


def check_vs_host(got, host, what=''):
    """GPU against train_augment_host: one float32 ulp, element by element."""
    check_structure(got, host)
    for k in FLOAT_KEYS:
        a, b = _a(got[k]).astype(np.float64), _a(host[k]).astype(np.float64)
        tol = 2.0 ** -23 * np.maximum(np.abs(b), 2.0 ** -126)
        worst = float(((np.abs(a - b)) / tol).max()) if a.size else 0.0
        print(f'{what} {k}: max |a - b| / (2^-23 |b|) = {worst:.3f}, '
              f'{int((a != b).sum())} of {a.size} differ')
        assert worst <= 1.0, (what, k, worst)
    for k in ('idx', 'overlap_p'):
        if k in host:
            assert got[k] == host[k], k
