"""Pose refinement on the full clouds: point-to-point and point-to-plane ICP, surface normals,
fitness, inlier RMSE, information.

``RegTR.forward`` solves its pose from the coarsest pyramid level (keypoints on a 0.2 m lattice
for 3DMatch). What a consumer does next -- ModelNet RRE / RTE, a pose graph over fragments, a
mapping loop -- is to refine that pose on the dense points and ask how good it is. This module
does both on the GPU (csrc/icp.hip behind ``fgr_icp`` / ``fgr_registration_score``; the
semantics are stated in include/fgreg.h and restated in tests/_icp_ref.py):

    out = model(batch)
    ref = fgreg.refine_outputs(batch, out, max_corr_dist=0.05)
    ref['pose'], ref['fitness'], ref['inlier_rmse'], ref['n_iters']

It is opt-in (nothing in the forward calls it), GPU only like ``fgreg.transforms_gpu`` (host
tensors raise FgrError), runs on the current stream and never synchronises: the iteration loop
and its stopping rule live on the device, and every returned tensor is a device tensor.

``icp(..., method='point_to_plane', normal_radius=...)`` refines against the target's surface
instead of its samples (csrc/normals.hip behind ``fgr_estimate_normals``, ``fgr_icp_plane``;
restated in tests/_icp_plane_ref.py): the choice for planar scenes sampled at different places
in the two clouds. ``estimate_normals`` gives the normals on their own.

``information`` is the 6 x 6 matrix sum J^T J over the inlier correspondences,
J = [I3 | -[s]x] with s the matched target point, translation first: the matrix the Redwood
``gt.info`` files hold and ``fgreg.rr3dmatch.transformation_error`` consumes
(``information[b, 0, 0]`` is the inlier count).
"""
import torch

from . import _lib, ops


def _pack(clouds):
    """A list of (n_i, 3) float32 GPU tensors -> (packed (N, 3), device offsets, lengths)."""
    if torch.is_tensor(clouds):
        clouds = list(clouds) if clouds.dim() == 3 else [clouds]
    ops._dev(*clouds)
    for c in clouds:
        if c.dim() != 2 or c.shape[1] != 3 or c.dtype != torch.float32:
            raise _lib.FgrError(f'expected (n, 3) float32 clouds, got {tuple(c.shape)} {c.dtype}')
    lengths = [int(c.shape[0]) for c in clouds]
    packed = clouds[0].contiguous() if len(clouds) == 1 else torch.cat(clouds, 0)
    return packed, ops.offsets(lengths, packed.device), lengths


def _geometry(src_xyz, tgt_xyz, pose, max_corr_dist):
    src, src_off, src_len = _pack(src_xyz)
    tgt, tgt_off, tgt_len = _pack(tgt_xyz)
    ops._dev(pose)
    n_pairs = len(src_len)
    if len(tgt_len) != n_pairs or tuple(pose.shape) != (n_pairs, 3, 4):
        raise _lib.FgrError(f'{n_pairs} source clouds need {n_pairs} target clouds and a pose of '
                            f'shape ({n_pairs}, 3, 4); got {len(tgt_len)} and {tuple(pose.shape)}')
    if not float(max_corr_dist) > 0.0:
        raise _lib.FgrError(f'max_corr_dist must be positive, got {max_corr_dist}')
    pose = ops._c(pose, torch.float32)
    nb = _lib.ws_size('fgr_icp_workspace', src.shape[0], tgt.shape[0], n_pairs)
    ws = ops.scratch(src.device, nb)
    geo = (ops._ptr(src), ops._ptr(src_off), src.shape[0], ops._ptr(tgt), ops._ptr(tgt_off),
           tgt.shape[0], n_pairs, max(src_len))
    keep = (src, src_off, tgt, tgt_off, pose, ws)
    return geo, keep, pose, ws, nb, n_pairs, src_len


def score(src_xyz, tgt_xyz, pose, max_corr_dist, information=False, correspondences=False):
    """One association pass under ``pose`` (B, 3, 4), source -> target.

    src_xyz / tgt_xyz: lists of per-cloud (n, 3) float32 GPU tensors, as ``batch['src_xyz']``.
    Returns a dict: ``fitness`` (B,) = inliers / source points, ``inlier_rmse`` (B,);
    with ``information`` the (B, 6, 6) float64 matrix described above; with
    ``correspondences`` two lists of per-cloud tensors, ``idx`` (int32 row of the nearest
    target inside the pair's target cloud, -1 where none lies within ``max_corr_dist``) and
    ``d2`` (its squared distance, +inf where none)."""
    geo, keep, pose, ws, nb, n_pairs, src_len = _geometry(src_xyz, tgt_xyz, pose, max_corr_dist)
    dev = pose.device
    fitness = torch.empty(n_pairs, dtype=torch.float32, device=dev)
    rmse = torch.empty(n_pairs, dtype=torch.float32, device=dev)
    n_src = sum(src_len)
    idx = torch.empty(n_src, dtype=torch.int32, device=dev) if correspondences else None
    d2 = torch.empty(n_src, dtype=torch.float32, device=dev) if correspondences else None
    info = torch.empty(n_pairs, 6, 6, dtype=torch.float64, device=dev) if information else None
    _lib.check(_lib.load().fgr_registration_score(
        *geo, ops._ptr(pose), float(max_corr_dist), ops._ptr(ws), nb, ops._ptr(fitness),
        ops._ptr(rmse), ops._ptr(idx), ops._ptr(d2), ops._ptr(info), ops._stream()),
        'fgr_registration_score')
    out = {'fitness': fitness, 'inlier_rmse': rmse}
    if information:
        out['information'] = info
    if correspondences:
        out['idx'] = list(torch.split(idx, src_len))
        out['d2'] = list(torch.split(d2, src_len))
    return out


METHODS = ('point_to_point', 'point_to_plane')


def estimate_normals(xyz, radius, view=None):
    """Surface normals of every cloud of ``xyz`` (a list of (n, 3) float32 GPU tensors) from the
    neighbours within ``radius``: the eigenvector of the neighbourhood covariance's smallest
    eigenvalue, turned towards ``view`` ((B, 3), one viewpoint per cloud; default the origin).

    Returns a dict: ``normals`` a list of (n, 3) float32 tensors, (0, 0, 0) where a point has
    fewer than 3 neighbours (itself included), and ``n_valid`` (B,) int32, the non-zero normals
    of each cloud."""
    pts, off, lengths = _pack(xyz)
    if not float(radius) > 0.0:
        raise _lib.FgrError(f'radius must be positive, got {radius}')
    n_clouds, dev = len(lengths), pts.device
    if view is not None:
        ops._dev(view)
        if tuple(view.shape) != (n_clouds, 3):
            raise _lib.FgrError(f'view must be ({n_clouds}, 3), got {tuple(view.shape)}')
        view = ops._c(view, torch.float32)
    nb = _lib.ws_size('fgr_estimate_normals_workspace', pts.shape[0], n_clouds)
    ws = ops.scratch(dev, nb)
    normals = torch.empty(pts.shape[0], 3, dtype=torch.float32, device=dev)
    n_valid = torch.empty(n_clouds, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().fgr_estimate_normals(
        ops._ptr(pts), ops._ptr(off), pts.shape[0], n_clouds, float(radius), ops._ptr(view),
        ops._ptr(ws), nb, ops._ptr(normals), ops._ptr(n_valid), ops._stream()),
        'fgr_estimate_normals')
    return {'normals': list(torch.split(normals, lengths)), 'n_valid': n_valid}


def icp(src_xyz, tgt_xyz, pose, max_corr_dist, max_iters=30, rel_fitness=1e-6, rel_rmse=1e-6,
        information=False, method='point_to_point', tgt_normals=None, normal_radius=None):
    """ICP from ``pose`` (B, 3, 4), every pair iterated on the device until its fitness and
    inlier RMSE change by less than ``rel_fitness`` / ``rel_rmse`` between two passes, it has
    too few inliers (3, point-to-plane 6), or ``max_iters`` updates were made.

    Returns a dict: ``pose`` (B, 3, 4), ``fitness`` (B,), ``inlier_rmse`` (B,) (both of the
    returned pose), ``n_iters`` (B,) int32 = the updates made, and with ``information`` the
    (B, 6, 6) float64 information matrix under the returned pose.

    ``method='point_to_plane'`` minimises the distance to the target's tangent planes. It needs
    either ``tgt_normals`` (a list, one (n, 3) tensor per target cloud, as ``estimate_normals``
    returns) or ``normal_radius`` (the normals are estimated first, on the same stream, with the
    origin as viewpoint). The dict gains ``plane_rmse`` (B,), ``status`` (B,) int32 (0
    converged, 1 ``max_iters`` reached, 2 fewer than 6 inliers, 3 singular: the inliers lie on
    one plane or on parallel ones) and ``tgt_normals`` (the normals used, for reuse);
    ``information`` is then the point-to-plane matrix sum J^T J, J = [n | q x n], not the
    Redwood one."""
    if method not in METHODS:
        raise ValueError(f'method must be one of {METHODS}, got {method!r}')
    if method == 'point_to_plane':
        return _icp_plane(src_xyz, tgt_xyz, pose, max_corr_dist, max_iters, rel_fitness, rel_rmse,
                          information, tgt_normals, normal_radius)
    if tgt_normals is not None or normal_radius is not None:
        raise ValueError("tgt_normals / normal_radius belong to method='point_to_plane'")
    geo, keep, pose, ws, nb, n_pairs, _ = _geometry(src_xyz, tgt_xyz, pose, max_corr_dist)
    dev = pose.device
    pose_out = torch.empty(n_pairs, 3, 4, dtype=torch.float32, device=dev)
    fitness = torch.empty(n_pairs, dtype=torch.float32, device=dev)
    rmse = torch.empty(n_pairs, dtype=torch.float32, device=dev)
    n_iters = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    L = _lib.load()
    _lib.check(L.fgr_icp(*geo, ops._ptr(pose), float(max_corr_dist), int(max_iters),
                         float(rel_fitness), float(rel_rmse), ops._ptr(ws), nb, ops._ptr(pose_out),
                         ops._ptr(fitness), ops._ptr(rmse), ops._ptr(n_iters), ops._stream()),
               'fgr_icp')
    out = {'pose': pose_out, 'fitness': fitness, 'inlier_rmse': rmse, 'n_iters': n_iters}
    if information:
        info = torch.empty(n_pairs, 6, 6, dtype=torch.float64, device=dev)
        f2, e2 = torch.empty_like(fitness), torch.empty_like(rmse)
        _lib.check(L.fgr_registration_score(
            *geo, ops._ptr(pose_out), float(max_corr_dist), ops._ptr(ws), nb, ops._ptr(f2),
            ops._ptr(e2), None, None, ops._ptr(info), ops._stream()), 'fgr_registration_score')
        out['information'] = info
    return out


def _icp_plane(src_xyz, tgt_xyz, pose, max_corr_dist, max_iters, rel_fitness, rel_rmse,
               information, tgt_normals, normal_radius):
    if (tgt_normals is None) == (normal_radius is None):
        raise ValueError("method='point_to_plane' needs exactly one of tgt_normals, normal_radius")
    if tgt_normals is None:
        tgt_normals = estimate_normals(tgt_xyz, normal_radius)['normals']
    nrm, _, nrm_len = _pack(tgt_normals)
    src, src_off, src_len = _pack(src_xyz)
    tgt, tgt_off, tgt_len = _pack(tgt_xyz)
    ops._dev(pose)
    n_pairs = len(src_len)
    if len(tgt_len) != n_pairs or tuple(pose.shape) != (n_pairs, 3, 4):
        raise _lib.FgrError(f'{n_pairs} source clouds need {n_pairs} target clouds and a pose of '
                            f'shape ({n_pairs}, 3, 4); got {len(tgt_len)} and {tuple(pose.shape)}')
    if nrm_len != tgt_len:
        raise _lib.FgrError(f'tgt_normals of lengths {nrm_len} for targets of lengths {tgt_len}')
    if not float(max_corr_dist) > 0.0:
        raise _lib.FgrError(f'max_corr_dist must be positive, got {max_corr_dist}')
    pose = ops._c(pose, torch.float32)
    dev = pose.device
    nb = _lib.ws_size('fgr_icp_plane_workspace', src.shape[0], tgt.shape[0], n_pairs)
    ws = ops.scratch(dev, nb)
    pose_out = torch.empty(n_pairs, 3, 4, dtype=torch.float32, device=dev)
    fitness, rmse, plane_rmse = (torch.empty(n_pairs, dtype=torch.float32, device=dev)
                                 for _ in range(3))
    n_iters, status = (torch.empty(n_pairs, dtype=torch.int32, device=dev) for _ in range(2))
    info = torch.empty(n_pairs, 6, 6, dtype=torch.float64, device=dev) if information else None
    _lib.check(_lib.load().fgr_icp_plane(
        ops._ptr(src), ops._ptr(src_off), src.shape[0], ops._ptr(tgt), ops._ptr(tgt_off),
        tgt.shape[0], ops._ptr(nrm), n_pairs, max(src_len), ops._ptr(pose), float(max_corr_dist),
        int(max_iters), float(rel_fitness), float(rel_rmse), ops._ptr(ws), nb, ops._ptr(pose_out),
        ops._ptr(fitness), ops._ptr(rmse), ops._ptr(plane_rmse), ops._ptr(n_iters),
        ops._ptr(status), ops._ptr(info), ops._stream()), 'fgr_icp_plane')
    out = {'pose': pose_out, 'fitness': fitness, 'inlier_rmse': rmse, 'n_iters': n_iters,
           'plane_rmse': plane_rmse, 'status': status, 'tgt_normals': list(tgt_normals)}
    if information:
        out['information'] = info
    return out


def refine_outputs(batch, outputs, max_corr_dist, **kw):
    """``icp`` on the batch's full clouds from the forward's final pose ``outputs['pose'][-1]``
    (the last decoder layer's); keyword arguments as ``icp``."""
    return icp(batch['src_xyz'], batch['tgt_xyz'], outputs['pose'][-1], max_corr_dist, **kw)
