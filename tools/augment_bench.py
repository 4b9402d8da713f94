"""Input-side timing of the 3DMatch / MCD training augmentations: one 20k + 20k-point pair with
about 10k correspondences (the 3DMatch training batch, B = 1) through
fgreg.augment.train_augment_gpu (host draws + upload + csrc/augment.hip, inputs already on the
GPU as ThreeDMatchPairs leaves them) and, beside it, through train_augment_host (the same chain
in NumPy float64, one core), with the same draws. Also the three kernels of
fgr_augment_pairs alone (HIP events) and the draws alone, which both paths share.

  python tools/augment_bench.py [n_points] [n_corr] [reps]
"""
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                'boosting-fine-grained-feature-fusion-in-3d-point-cloud-registration_amd'))
from fgreg import _lib, augment  # noqa: E402
from fgreg.synthetic import lowoverlap_pair  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    n_corr = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    src, tgt, pose, f = lowoverlap_pair(0, n_points=n)
    rng = np.random.default_rng(0)
    host_sample = {'src_xyz': torch.from_numpy(src), 'tgt_xyz': torch.from_numpy(tgt),
                   'src_overlap': torch.from_numpy(rng.random(n) < 0.3),
                   'tgt_overlap': torch.from_numpy(rng.random(n) < 0.3),
                   'correspondences': torch.from_numpy(np.stack([rng.integers(0, n, n_corr),
                                                                 rng.integers(0, n, n_corr)])),
                   'pose': torch.from_numpy(pose), 'idx': 0, 'src_path': 'a', 'tgt_path': 'b',
                   'overlap_p': f}
    dev_sample = {k: (v.cuda() if torch.is_tensor(v) and k != 'pose' else v)
                  for k, v in host_sample.items()}
    torch.manual_seed(0)
    np.random.seed(0)
    random.seed(0)
    t0 = time.perf_counter()
    for _ in range(reps):
        draws = augment.draw_train_augment(n, n, 'small')
    t_draw = (time.perf_counter() - t0) / reps

    augment.train_augment_gpu([dev_sample], draws=[draws])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        augment.train_augment_host(host_sample, draws, 0.005)
    t_host = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for _ in range(reps):
        augment.train_augment_gpu([dev_sample], draws=[draws])
    torch.cuda.synchronize()
    t_gpu = (time.perf_counter() - t0) / reps

    L = _lib.load()                       # the entry point's three launches, by HIP events
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    st = torch.cuda.current_stream()
    ms = []
    orig = L.fgr_augment_pairs

    def timed(*a):
        ev[0].record(st)
        rc = orig(*a)
        ev[1].record(st)
        ev[1].synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
        return rc
    L.fgr_augment_pairs = timed
    try:
        for _ in range(reps):
            augment.train_augment_gpu([dev_sample], draws=[draws])
    finally:
        L.fgr_augment_pairs = orig
    print(f'{n} + {n} points, {n_corr} correspondences, B = 1: draws {t_draw * 1e3:.2f} ms (shared); '
          f'host pipeline {t_host * 1e3:.2f} ms, GPU-resident {t_gpu * 1e3:.2f} ms '
          f'({t_host / t_gpu:.1f}x); fgr_augment_pairs (3 launches) {np.median(ms) * 1e3:.1f} us')


if __name__ == '__main__':
    main()
