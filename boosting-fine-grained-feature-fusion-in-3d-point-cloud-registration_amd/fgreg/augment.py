"""The 3DMatch / MCD training augmentations as a GPU input pipeline.

The reference's `get_dataloader` (data_loaders/__init__.py:16-57) puts four transforms of
data_loaders/transforms.py in front of every 3DMatch and MCD training sample, controlled by
`perturb_pose` and `augment_noise` of conf/3dmatch.yaml / conf/mcd.yaml:

  RigidPerturb(perturb_pose)   :15-72    a small / large random rigid motion of one cloud
  -> Jitter(augment_noise)     :75-92    Gaussian noise on both clouds
  -> ShufflePoints()           :95-131   a permutation, truncated to max_pts = 30000 points
  -> RandomSwap()              :134-151  exchange source and target half of the time

The work splits where the reference's randomness allows, as in fgreg.transforms_gpu:

- host: `draw_train_augment` takes the sample's draws from the reference's three global
  generators (NumPy's, `random`'s and torch's CPU default generator) in the reference's
  order. None of them depends on the points, only on the two cloud sizes;
- GPU (csrc/augment.hip, `fgr_augment_pairs`): the centroid, the pose algebra, moving and
  gathering the points, the overlap flags and the correspondence remap, for a whole batch in
  three launches. `train_augment_gpu` returns the reference's sample dicts with every tensor
  on the GPU; one small readback per batch (the correspondence counts). No CPU fallback.

`train_augment_host` is the same chain in NumPy float64, rounded once to float32: the checker
of the kernels (tests/test_gpu_augment.py), itself pinned to the reference's own transform
objects by tests/golden/threedmatch_augment.npz (tests/test_augment.py).
"""
import random

import numpy as np
import torch

from . import _lib
from .transforms import _uniform_s2, collate_pair
from .transforms_gpu import _ptr, _upload

MODES = ('none', 'small', 'large')
AUG_PERTURB, AUG_SOURCE, AUG_CENTRE, AUG_SWAP = 1, 2, 4, 8      # FGR_AUG_* of include/fgreg.h


# ---- the draws -------------------------------------------------------------------------------
def _hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _sample_small(std=0.1):
    """SE3.sample_small(std=0.1) (cvhelpers/lie/numpy/se3.py:37-44, so3.py:30-38, :81-101) with
    its draws and its float64 evaluation order -> (3, 4) float64."""
    axis = _uniform_s2()                                   # uniform_2_sphere
    theta = np.random.randn()
    theta *= std * np.pi / np.sqrt(3)
    omega = axis * theta
    trans = np.random.randn(3, 1) * std / np.sqrt(3)
    ang = np.linalg.norm(omega, axis=-1, keepdims=True)    # (1,)
    if np.isclose(ang, 0.)[0]:
        rot = np.identity(3) + _hat(omega)
    else:
        w_hat = _hat(omega / ang)
        rot = np.identity(3) + np.sin(ang)[..., None] * w_hat \
            + (1 - np.cos(ang)[..., None]) * (w_hat @ w_hat)
    return np.concatenate([rot, trans], axis=-1)


def _sample_large():
    """RigidPerturb._sample_pose_large (transforms.py:27-32): rand(3) * 2 pi as extrinsic 'zyx'
    Euler angles (a turn about z, then y, then x: R = Rx Ry Rz), no translation."""
    az, ay, ax = np.random.rand(3) * np.pi * 2
    cz, sz, cy, sy, cx, sx = np.cos(az), np.sin(az), np.cos(ay), np.sin(ay), np.cos(ax), np.sin(ax)
    rot = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
           @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
           @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))
    return np.concatenate([rot, np.zeros((3, 1))], axis=1)


def draw_train_augment(n_src, n_tgt, perturb_pose, max_pts=30000, shuffle=True):
    """One sample's random draws, from np.random, random and torch's CPU default generator in
    the order the reference's chain takes them. -> dict:
      mode            perturb_pose
      perturb         (3, 4) float32 (rounded before anything is composed with it, as the
                      reference's .float()), None for 'none'
      perturb_source  bool: the source is perturbed (else the target); None for 'none'
      noise_src/_tgt  (n, 3) float32 torch.randn draws, unscaled
      src_idx/tgt_idx int64: ShufflePoints' kept rows in output order
      swap            bool"""
    if perturb_pose not in MODES:
        raise ValueError(f'perturb_pose must be one of {MODES}')
    d = {'mode': perturb_pose, 'perturb': None, 'perturb_source': None}
    if perturb_pose != 'none':
        p = _sample_small() if perturb_pose == 'small' else _sample_large()
        d['perturb'] = p.astype(np.float32)
        d['perturb_source'] = random.random() > 0.5
    d['noise_src'] = torch.randn((n_src, 3))
    d['noise_tgt'] = torch.randn((n_tgt, 3))
    if shuffle:
        d['src_idx'] = np.random.permutation(n_src)[:max_pts]
        d['tgt_idx'] = np.random.permutation(n_tgt)[:max_pts]
    else:
        d['src_idx'] = np.arange(min(n_src, max_pts))
        d['tgt_idx'] = np.arange(min(n_tgt, max_pts))
    d['swap'] = random.random() > 0.5
    return d


# ---- the float64 host pipeline ---------------------------------------------------------------
def _cat(a, b):
    return np.concatenate([a[:, :3] @ b[:, :3], a[:, :3] @ b[:, 3:] + a[:, 3:]], axis=1)


def _inv(a):
    return np.concatenate([a[:, :3].T, -(a[:, :3].T @ a[:, 3:])], axis=1)


def _np(t, dtype=None):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a if dtype is None else a.astype(dtype)


def _scaled_noise(draw, scale):
    """Jitter's `torch.randn(shape) * scale` (transforms.py:90): a float32 product."""
    return (draw * scale).numpy().astype(np.float64)


def _move(t, xyz, noise):
    x, y, z = xyz[:, 0:1], xyz[:, 1:2], xyz[:, 2:3]
    return (((t[:, 0] * x + t[:, 1] * y) + t[:, 2] * z) + t[:, 3]) + noise


def train_augment_host(sample, draws, scale):
    """The chain on one sample dict with the draws of draw_train_augment, evaluated in float64
    and rounded once to float32 -> the reference's sample dict (CPU tensors)."""
    _refuse_extra(sample)
    src, tgt = _np(sample['src_xyz'], np.float64), _np(sample['tgt_xyz'], np.float64)
    pose = _np(sample['pose'], np.float64)
    eye = np.concatenate([np.identity(3), np.zeros((3, 1))], axis=1)
    t_src, t_tgt = eye, eye
    if draws['perturb'] is not None:
        p = draws['perturb'].astype(np.float64)
        if draws['mode'] == 'small':
            # about the centroid of the perturbed cloud (all of its points): C^-1 P C
            c = np.mean(src if draws['perturb_source'] else tgt, axis=0)[:, None]
            ci, cm = eye.copy(), eye.copy()
            ci[:, 3:], cm[:, 3:] = c, -c
            p = _cat(_cat(ci, p), cm)
        if draws['perturb_source']:
            pose, t_src = _cat(pose, _inv(p)), p
        else:
            pose, t_tgt = _cat(p, pose), p
    s_idx, t_idx = np.asarray(draws['src_idx']), np.asarray(draws['tgt_idx'])
    s_rev, t_rev = np.full(src.shape[0], -1), np.full(tgt.shape[0], -1)
    src = _move(t_src, src, _scaled_noise(draws['noise_src'], scale))[s_idx]
    tgt = _move(t_tgt, tgt, _scaled_noise(draws['noise_tgt'], scale))[t_idx]
    s_ov, t_ov = _np(sample['src_overlap'])[s_idx], _np(sample['tgt_overlap'])[t_idx]
    s_rev[s_idx] = np.arange(len(s_idx))
    t_rev[t_idx] = np.arange(len(t_idx))
    corr = _np(sample['correspondences'], np.int64)
    corr = np.stack([s_rev[corr[0]], t_rev[corr[1]]])
    corr = corr[:, np.all(corr >= 0, axis=0)]
    paths = [sample.get('src_path'), sample.get('tgt_path')]
    if draws['swap']:
        src, tgt, s_ov, t_ov = tgt, src, t_ov, s_ov
        corr, pose, paths = corr[::-1], _inv(pose), paths[::-1]
    out = {'src_xyz': torch.from_numpy(src.astype(np.float32)),
           'tgt_xyz': torch.from_numpy(tgt.astype(np.float32)),
           'src_overlap': torch.from_numpy(np.ascontiguousarray(s_ov)),
           'tgt_overlap': torch.from_numpy(np.ascontiguousarray(t_ov)),
           'correspondences': torch.from_numpy(np.ascontiguousarray(corr, dtype=np.int64)),
           'pose': torch.from_numpy(pose.astype(np.float32))}
    return _finish(out, sample, paths)


def _finish(out, sample, paths):
    """idx, the (possibly swapped) paths and overlap_p, in the reference's key order."""
    if 'idx' in sample:
        out['idx'] = sample['idx']
    if paths[0] is not None:
        out['src_path'], out['tgt_path'] = paths
    if 'overlap_p' in sample:
        out['overlap_p'] = sample['overlap_p']
    return out


# ---- the GPU pipeline ------------------------------------------------------------------------
def _check_perm(idx, n, what):
    idx = np.asarray(idx)
    ok = idx.ndim == 1 and len(idx) <= n and idx.dtype.kind in 'iu'
    if ok and len(idx):
        ok = idx.min() >= 0 and idx.max() < n and np.bincount(idx, minlength=n).max() == 1
    if not ok:
        raise ValueError(f'train_augment_gpu: {what} is not a list of distinct rows of its cloud')
    return idx.astype(np.int32)


def _refuse_extra(sample):
    """RigidPerturb and RandomSwap also move 'corr_xyz' / 'corr_xyz_ds' where a sample has
    them (transforms.py:59-70, :146-149); no 3DMatch or MCD sample does, and this chain does
    not restate it."""
    for k in ('corr_xyz', 'corr_xyz_ds'):
        if k in sample:
            raise NotImplementedError(f"training augmentations: samples with '{k}'")


def train_augment_gpu(samples, perturb_pose='small', augment_noise=0.005, max_pts=30000,
                      shuffle=True, draws=None, device='cuda'):
    """The training augmentations on a list of sample dicts (the keys of ThreeDMatchDataset /
    fgreg.data.ThreeDMatchPairs; tensors on any device, or NumPy arrays) -> the augmented
    sample dicts with the reference's keys and dtypes, every tensor on the GPU.

    draws: one draw_train_augment dict per sample (None: drawn here, in sample order, from
    perturb_pose / max_pts / shuffle, which are otherwise unused)."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise ValueError('train_augment_gpu: a GPU device is required (no CPU fallback)')
    if len(samples) == 0:
        raise ValueError('train_augment_gpu: no samples')
    with torch.cuda.device(dev):                    # launches go to this device's stream
        return _augment_batch(samples, perturb_pose, augment_noise, max_pts, shuffle, draws, dev)


def _augment_batch(samples, perturb_pose, scale, max_pts, shuffle, draws, dev):
    L = _lib.load()
    B = len(samples)
    for s in samples:
        _refuse_extra(s)
    clouds = [torch.as_tensor(s[k]) for s in samples for k in ('src_xyz', 'tgt_xyz')]
    if any(c.dim() != 2 or c.shape[1] != 3 or c.shape[0] < 1 for c in clouds):
        raise ValueError('train_augment_gpu: clouds must be (N >= 1, 3)')
    ns = [int(c.shape[0]) for c in clouds]
    if draws is None:
        draws = [draw_train_augment(ns[2 * b], ns[2 * b + 1], perturb_pose, max_pts, shuffle)
                 for b in range(B)]
    if len(draws) != B:
        raise ValueError('train_augment_gpu: need one set of draws per sample')
    in_off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    n_tot = int(in_off[-1])
    if n_tot >= 2 ** 31:
        raise ValueError('train_augment_gpu: the batch holds 2^31 points or more')
    perms = [_check_perm(d[k], ns[2 * b + c], k)
             for b, d in enumerate(draws) for c, k in enumerate(('src_idx', 'tgt_idx'))]
    ms = [len(p) for p in perms]
    if min(ms) < 1:
        raise ValueError('train_augment_gpu: every cloud must keep at least one point')
    out_off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    m_tot = int(out_off[-1])
    corrs = [torch.as_tensor(s['correspondences']) for s in samples]
    if any(c.dim() != 2 or c.shape[0] != 2 for c in corrs):
        raise ValueError('train_augment_gpu: correspondences must be (2, C)')
    corr_off = np.concatenate([[0], np.cumsum([int(c.shape[1]) for c in corrs])]).astype(np.int64)
    c_tot = int(corr_off[-1])
    flags = np.zeros(B, dtype=np.int32)
    perturb = np.zeros((B, 3, 4), dtype=np.float32)
    for b, d in enumerate(draws):
        if d['perturb'] is not None:
            perturb[b] = d['perturb']
            flags[b] |= AUG_PERTURB | (AUG_SOURCE if d['perturb_source'] else 0) \
                | (AUG_CENTRE if d['mode'] == 'small' else 0)
        flags[b] |= AUG_SWAP if d['swap'] else 0

    xyz = torch.cat([c.to(dev, torch.float32) for c in clouds]).contiguous()
    ov = torch.cat([torch.as_tensor(s[k]).to(dev).to(torch.uint8)
                    for s in samples for k in ('src_overlap', 'tgt_overlap')]).contiguous()
    if ov.shape[0] != n_tot:
        raise ValueError('train_augment_gpu: one overlap flag per point')
    corr = torch.cat([c.to(dev, torch.int64) for c in corrs], dim=1).contiguous()
    poses = [torch.as_tensor(s['pose']) for s in samples]
    host = [in_off, out_off, corr_off, flags, perturb, np.concatenate(perms)]
    if not any(p.is_cuda for p in poses):
        host.append(np.stack([p.numpy().astype(np.float32) for p in poses]))
    if scale != 0:                                   # Jitter's float32 product, packed as xyz
        host.append(np.concatenate([(d[k] * scale).numpy() for d in draws
                                    for k in ('noise_src', 'noise_tgt')]).astype(np.float32))
        if host[-1].shape != (n_tot, 3):
            raise ValueError('train_augment_gpu: one noise row per point')
    up = _upload(dev, *host)
    in_off_d, out_off_d, corr_off_d, flags_d, perturb_d, perm_d = up[:6]
    pose_d = up[6] if not any(p.is_cuda for p in poses) else \
        torch.stack([p.to(dev, torch.float32) for p in poses]).contiguous()
    noise_d = up[-1] if scale != 0 else None

    xyz_out = torch.empty((m_tot, 3), dtype=torch.float32, device=dev)
    ov_out = torch.empty(m_tot, dtype=torch.uint8, device=dev)
    corr_out = torch.empty((2, c_tot), dtype=torch.int64, device=dev)
    n_corr = torch.empty(B, dtype=torch.int32, device=dev)
    pose_out = torch.empty((B, 3, 4), dtype=torch.float32, device=dev)
    ws_bytes = _lib.ws_size('fgr_augment_workspace_bytes', n_tot, B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(L.fgr_augment_pairs(
        _ptr(xyz), 3, _ptr(in_off_d), n_tot, _ptr(ov), _ptr(corr) if c_tot else None, c_tot,
        _ptr(corr_off_d), _ptr(pose_d), _ptr(perturb_d), _ptr(flags_d), _ptr(perm_d),
        _ptr(out_off_d), max(ms), None if noise_d is None else _ptr(noise_d), B,
        _ptr(xyz_out), _ptr(ov_out), _ptr(corr_out) if c_tot else None, _ptr(n_corr),
        _ptr(pose_out), _ptr(ws), ws_bytes, st), 'fgr_augment_pairs')
    nc = n_corr.cpu().numpy()                        # the one readback: correspondence counts
    if (nc < 0).any():
        raise _lib.FgrError('fgr_augment_pairs: a correspondence index lies outside its cloud '
                            f'(samples {np.nonzero(nc < 0)[0].tolist()})')
    ovb = ov_out.bool()
    out = []
    for b, (s, d) in enumerate(zip(samples, draws)):
        o, m_s, m_t = int(out_off[2 * b]), ms[2 * b], ms[2 * b + 1]
        paths = [s.get('src_path'), s.get('tgt_path')]
        if d['swap']:                                # post-swap order: the old target first
            m_s, m_t, paths = m_t, m_s, paths[::-1]
        co = int(corr_off[b])
        out.append(_finish({'src_xyz': xyz_out[o:o + m_s],
                            'tgt_xyz': xyz_out[o + m_s:o + m_s + m_t],
                            'src_overlap': ovb[o:o + m_s],
                            'tgt_overlap': ovb[o + m_s:o + m_s + m_t],
                            'correspondences': corr_out[:, co:co + int(nc[b])],
                            'pose': pose_out[b]}, s, paths))
    return out


def train_batch_gpu(samples, **kw):
    """train_augment_gpu + collate_pair (collate_functions.py:4-22): the batch dict the model's
    training forward and compute_loss take, GPU-resident."""
    return collate_pair(train_augment_gpu(samples, **kw))


class TrainAugment:
    """The chain as a callable on one sample, for `ThreeDMatchPairs(..., transforms=...)`:
    what get_dataloader composes for phase 'train' from cfg.perturb_pose / cfg.augment_noise."""

    def __init__(self, perturb_pose, augment_noise, max_pts=30000, shuffle=True, device=None):
        if perturb_pose not in MODES:
            raise ValueError(f'perturb_pose must be one of {MODES}')
        self.perturb_pose, self.augment_noise = perturb_pose, augment_noise
        self.max_pts, self.shuffle, self.device = max_pts, shuffle, device

    def __call__(self, sample):
        dev = self.device
        if dev is None:
            x = sample['src_xyz']
            dev = x.device if torch.is_tensor(x) and x.is_cuda else 'cuda'
        return train_augment_gpu([sample], self.perturb_pose, self.augment_noise, self.max_pts,
                                 self.shuffle, device=dev)[0]


__all__ = ['draw_train_augment', 'train_augment_host', 'train_augment_gpu', 'train_batch_gpu',
           'TrainAugment']
