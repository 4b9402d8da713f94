"""CPU: the large-extent input of the sparse grid-subsampling tests (fgreg.synthetic.
lidar_like_pair) is what those tests assume -- past the dense voxel histogram's ceiling at the
first pooling voxel of mcd.yaml / 3dmatch.yaml (dl = 0.05), below it one level down -- so the
GPU tests of tests/test_gpu_grid_sparse.py cannot pass silently through the dense path."""
import numpy as np

import geom as og


def _key_space(points, lengths, dl):
    """Summed nx * ny * nz of the clouds with the origin / dims formula of
    grid_subsampling.cpp:25-31 in fp32 (oracle/geom_oracle.c, csrc/grid.hip)."""
    dl = np.float32(dl)
    inv = np.float32(1.0) / dl
    total, o = 0, 0
    for n in lengths:
        p = points[o:o + n]
        o += n
        if n == 0:
            continue
        mn, mx = p.min(0), p.max(0)
        org = (np.floor(mn * inv) * dl).astype(np.float32)
        dims = np.floor(((mx - org).astype(np.float32) / dl).astype(np.float32)).astype(np.int64) + 1
        total += int(dims[0]) * int(dims[1]) * int(dims[2])
    return total


def test_lidar_like_pair_is_deterministic():
    from fgreg.synthetic import lidar_like_pair
    a, b = lidar_like_pair(0), lidar_like_pair(0)
    for x, y in zip(a, b):
        assert x.dtype == np.float32 and np.array_equal(x, y)
    src, tgt, pose = a
    assert src.shape == (6000, 3) and tgt.shape == (6000, 3) and pose.shape == (3, 4)
    assert np.allclose(pose[:, :3] @ pose[:, :3].T, np.eye(3), atol=1e-5)
    assert not np.array_equal(lidar_like_pair(1)[0], src)
    big = lidar_like_pair(0, n_points=60000)
    assert big[0].shape == (60000, 3)
    # the extent is the point: ~60 m x 60 m x 12 m
    ext = tgt.max(0) - tgt.min(0)
    assert 55 < ext[0] <= 63 and 55 < ext[1] <= 60 and 11 < ext[2] <= 12.2


def test_lidar_like_pair_leaves_the_dense_path_at_the_first_level_only():
    from fgreg import ops
    from fgreg.synthetic import lidar_like_pair
    src, tgt, _ = lidar_like_pair(0)
    pts, lens = np.concatenate([src, tgt]), [len(src), len(tgt)]
    assert _key_space(pts, lens, 0.05) > ops.GRID_MAX_CELLS
    p1, l1, k1 = og.grid_subsample(pts, lens, 0.05, return_keys=True)
    assert _key_space(p1, [int(v) for v in l1], 0.1) < ops.GRID_MAX_CELLS
    # the oracle runs on it; voxel keys ascend strictly per cloud
    assert l1.sum() == len(p1) and 0 < l1[0] <= 6000 and 0 < l1[1] <= 6000
    o = 0
    for n in l1:
        assert (np.diff(k1[o:o + n]) > 0).all()
        o += n
    assert k1.max() >= 1 << 28
