"""Writes tests/golden/match_ref.npz: the reference's feature-matching utilities
(models/ransaclib/registration_utils.py: extract_corr_indices_from_feats in its one-way, mutual
and bilateral modes, compute_inlier_ratio) on one seeded case, arrays only. Run where the
reference is mounted:

    python tests/golden/make_match_golden.py /path/to/reference

Naming: the reference's `ref` cloud is this project's target, its `src` this project's source
(its transform takes src to ref, as ours takes source to target). Its one-way mode lists every
ref (target) row with its nearest source row; `oneway_swapped` calls it with the roles swapped,
which is this project's 'src' mode.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _match_ref as mr  # noqa: E402

NS, NT, D, SEED, RADIUS = 77, 130, 32, 20240, 0.1


def main(reference):
    sys.path.insert(0, os.path.join(reference, 'models', 'ransaclib'))
    from scipy.spatial import cKDTree
    import geotransformer.utils.pointcloud as pc

    class Tree(cKDTree):                    # newer scipy: query's n_jobs became `workers`
        def query(self, x, k=1, n_jobs=None, **kw):
            return super().query(x, k=k, **kw)
    pc.cKDTree = Tree
    import registration_utils as ru

    src_feat, tgt_feat, pick = mr.descriptors(SEED, NS, NT, D)
    rng = np.random.default_rng(SEED + 1)
    src_xyz = rng.uniform(-1, 1, (NS, 3)).astype(np.float32)
    ang = np.deg2rad(25.0)
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, [0.2, -0.1, 0.3]
    # target points: the copied source rows moved by T, a third of them displaced far beyond the
    # radius (outliers), the rest jittered well inside it
    tgt_xyz = src_xyz[pick].astype(np.float64) @ R.T + T[:3, 3] + rng.normal(0, 0.01, (NT, 3))
    tgt_xyz[rng.random(NT) < 0.33] += 0.5
    tgt_xyz = tgt_xyz.astype(np.float32)

    out = {'src_feat': src_feat, 'tgt_feat': tgt_feat, 'src_xyz': src_xyz, 'tgt_xyz': tgt_xyz,
           'transform': T, 'radius': np.float64(RADIUS)}
    calls = {'oneway': (tgt_feat, src_feat, {}), 'oneway_swapped': (src_feat, tgt_feat, {}),
             'mutual': (tgt_feat, src_feat, {'mutual': True}),
             'bilateral': (tgt_feat, src_feat, {'bilateral': True})}
    for name, (ref_f, src_f, kw) in calls.items():
        ref_i, src_i = ru.extract_corr_indices_from_feats(ref_f, src_f, **kw)
        out[name + '_ref'], out[name + '_src'] = ref_i.astype(np.int64), src_i.astype(np.int64)
        if name == 'oneway_swapped':       # ref = our source: the transform is the inverse
            ir = ru.compute_inlier_ratio(src_xyz[ref_i], tgt_xyz[src_i], np.linalg.inv(T), RADIUS)
        else:
            ir = ru.compute_inlier_ratio(tgt_xyz[ref_i], src_xyz[src_i], T, RADIUS)
        out[name + '_inlier_ratio'] = np.float64(ir)
    path = os.path.join(HERE, 'match_ref.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), {k: float(out[k]) for k in out if k.endswith('ratio')})


if __name__ == '__main__':
    main(sys.argv[1])
