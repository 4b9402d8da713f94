"""Robust pose from putative correspondences: RANSAC on the GPU.

``RegTR.forward`` solves its pose with one weighted least-squares fit over every predicted
correspondence; a confidently wrong minority bends it, and ``fgreg.icp`` cannot recover from a
start outside its basin. This module is the estimator between the two (csrc/ransac.hip behind
``fgr_ransac_pose``; the semantics are stated in include/fgreg.h and restated in
tests/_ransac_ref.py): thousands of 3-point hypotheses, each scored against every
correspondence of its pair, the best one refitted on its inliers.

    out = model(batch)
    rob = fgreg.ransac_outputs(out, inlier_dist=0.1)
    ref = fgreg.icp(batch['src_xyz'], batch['tgt_xyz'], rob['pose'], max_corr_dist=0.05)

It is opt-in (nothing in the forward calls it), GPU only (host tensors raise FgrError), runs on
the current stream and never synchronises: sampling, selection and the refits live on the
device, and every returned tensor is a device tensor. The draws are a counter-based hash of
(seed, pair, hypothesis): the same seed gives the same result bit for bit.

A call can be captured into a graph after one eager call with the same lengths (the row
offsets of a list of lengths are uploaded once and kept).

``compat`` / ``compat_outputs`` are the estimator for few inliers (csrc/compat.hip behind
``fgr_compat_pose``, restated in tests/_compat_ref.py): at 3-5 % a uniform 3-point sample is
almost never all-inlier, so the seeds come from the spatial compatibility of the rows instead,
without a draw; scoring, selection and refits are RANSAC's, under the same terms as above.
"""
import torch

from . import _lib, ops

_OFFSETS = {}       # (device, lengths) -> device row offsets: no upload on a repeated call


def _offsets(lengths, device):
    key = (str(device), tuple(lengths))
    off = _OFFSETS.get(key)
    if off is None:
        if len(_OFFSETS) > 4096:
            _OFFSETS.clear()
        off = _OFFSETS[key] = ops.offsets(lengths, device)
    return off


def _rows(x, cols, what):
    """One tensor or a list of per-pair tensors -> the list, checked."""
    xs = [x] if torch.is_tensor(x) else list(x)
    ops._dev(*xs)
    for t in xs:
        ok = t.dtype == torch.float32 and (t.dim() == 2 and t.shape[1] == 3 if cols == 3 else t.dim() == 1)
        if not ok:
            raise _lib.FgrError(f'{what}: expected float32 of shape '
                                f'{"(n, 3)" if cols == 3 else "(n,)"}, got {tuple(t.shape)} {t.dtype}')
    return xs


def _packed(xs):
    return xs[0].contiguous() if len(xs) == 1 else torch.cat(xs, 0)


def _inputs(a, b, weights):
    """The checked, packed inputs of both estimators -> (a, b, w or None, lengths, offsets)."""
    A, Bs = _rows(a, 3, 'a'), _rows(b, 3, 'b')
    W = None if weights is None else _rows(weights, 1, 'weights')
    lengths = [int(t.shape[0]) for t in A]
    if [int(t.shape[0]) for t in Bs] != lengths or \
            (W is not None and [int(t.shape[0]) for t in W] != lengths) or not lengths:
        raise _lib.FgrError('a, b and weights need the same number of pairs and rows per pair')
    pa = _packed(A)
    return pa, _packed(Bs), None if W is None else _packed(W), lengths, _offsets(lengths, pa.device)


def _outputs(n_pairs, n_tot, dev, mask):
    """The outputs both estimators share -> (pose, rmse, n_inliers, n_eligible, best, n_updates,
    mask bytes or None)."""
    i32 = lambda: torch.empty(n_pairs, dtype=torch.int32, device=dev)
    return (torch.empty(n_pairs, 3, 4, dtype=torch.float32, device=dev),
            torch.empty(n_pairs, dtype=torch.float32, device=dev), i32(), i32(), i32(), i32(),
            torch.empty(n_tot, dtype=torch.uint8, device=dev) if mask else None)


def ransac(a, b, weights=None, *, inlier_dist, n_hyp=4096, w_min=0.0, seed=0, n_refits=4,
           mask=False, hypotheses=False):
    """RANSAC over the correspondences ``a[i] -> b[i]`` (b ~ R a + t) of every pair.

    a, b: lists of per-pair (n, 3) float32 GPU tensors, or one tensor for a single pair;
    weights: per-pair (n,) tensors or None. Only rows with ``weights > w_min`` take part.
    ``n_hyp`` 3-point hypotheses per pair are solved and scored by their number of rows within
    ``inlier_dist``; the best (the lowest index on a tie) is refitted on its inliers at most
    ``n_refits`` times, as long as the count does not drop.

    Returns a dict of device tensors: ``pose`` (B, 3, 4), ``n_inliers``, ``n_eligible``,
    ``best_hyp`` (-1: no valid hypothesis, the pose is the identity), ``n_updates`` (the refits
    adopted), all (B,) int32, and ``inlier_rmse`` (B,); with ``mask`` a list of per-pair bool
    tensors ``mask`` (the inliers of the returned pose, in the caller's row order); with
    ``hypotheses`` every hypothesis's ``hyp_pose`` (B, n_hyp, 3, 4) and ``hyp_count``
    (B, n_hyp) int32 (-1: a repeated sample)."""
    pa, pb, pw, lengths, off = _inputs(a, b, weights)
    dev = pa.device
    n_tot, n_pairs = int(pa.shape[0]), len(lengths)
    nb = _lib.ws_size('fgr_ransac_workspace', n_tot, n_pairs, int(n_hyp))
    ws = ops.scratch(dev, nb)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    pose, rmse, n_inl, n_el, best, upd, msk = _outputs(n_pairs, n_tot, dev, mask)
    hp = torch.empty(n_pairs, int(n_hyp), 3, 4, dtype=torch.float32, device=dev) if hypotheses else None
    hc = i32(n_pairs, int(n_hyp)) if hypotheses else None
    _lib.check(_lib.load().fgr_ransac_pose(
        ops._ptr(pa), ops._ptr(pb), ops._ptr(pw), n_tot, ops._ptr(off), n_pairs, float(w_min),
        float(inlier_dist), int(n_hyp), int(seed) & 0xFFFFFFFF, int(n_refits), ops._ptr(ws), nb,
        ops._ptr(pose), ops._ptr(n_inl), ops._ptr(rmse), ops._ptr(n_el), ops._ptr(best),
        ops._ptr(upd), ops._ptr(msk), ops._ptr(hp), ops._ptr(hc), ops._stream()), 'fgr_ransac_pose')
    out = {'pose': pose, 'n_inliers': n_inl, 'n_eligible': n_el, 'inlier_rmse': rmse,
           'best_hyp': best, 'n_updates': upd}
    if mask:
        out['mask'] = list(torch.split(msk.bool(), lengths))
    if hypotheses:
        out['hyp_pose'], out['hyp_count'] = hp, hc
    return out


def compat(a, b, weights=None, *, compat_dist, inlier_dist, n_seeds=64, k=16, w_min=0.0,
           n_refits=4, mask=False, seeds=False, scores=False):
    """Pose from spatial compatibility, for correspondences with few inliers (csrc/compat.hip
    behind ``fgr_compat_pose``; include/fgreg.h states the semantics, tests/_compat_ref.py
    restates them). Inputs, eligibility and refits as ``ransac``; no draws: rows i, j are
    compatible when the lengths |a_i - a_j| and |b_i - b_j| differ by less than
    ``compat_dist``, a row's score sums the common compatible rows over its compatible rows,
    the ``n_seeds`` best-scored rows each solve a pose from their ``k - 1`` most compatible
    neighbours, and the pose with the most rows within ``inlier_dist`` is refitted.

    Returns ``ransac``'s dict with ``best_seed`` (the winning seed's position, -1: no valid
    seed) in the place of ``best_hyp``; with ``seeds`` also ``seed_row`` (B, n_seeds) int32 (the
    seed's row within its pair, -1: unused), ``seed_pose`` (B, n_seeds, 3, 4) and ``seed_count``
    (B, n_seeds) int32 (-1: invalid); with ``scores`` a per-pair list ``row_score`` (int32, -1
    on rows that do not take part)."""
    pa, pb, pw, lengths, off = _inputs(a, b, weights)
    dev = pa.device
    n_tot, n_pairs, max_len, ns = int(pa.shape[0]), len(lengths), max(lengths), int(n_seeds)
    nb = _lib.ws_size('fgr_compat_workspace', n_tot, n_pairs, max_len, ns)
    ws = ops.scratch(dev, nb)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    pose, rmse, n_inl, n_el, best, upd, msk = _outputs(n_pairs, n_tot, dev, mask)
    rs = i32(n_tot) if scores else None
    sr = i32(n_pairs, ns) if seeds else None
    sp = torch.empty(n_pairs, ns, 3, 4, dtype=torch.float32, device=dev) if seeds else None
    sc = i32(n_pairs, ns) if seeds else None
    _lib.check(_lib.load().fgr_compat_pose(
        ops._ptr(pa), ops._ptr(pb), ops._ptr(pw), n_tot, ops._ptr(off), n_pairs, max_len,
        float(w_min), float(compat_dist), float(inlier_dist), ns, int(k), int(n_refits),
        ops._ptr(ws), nb, ops._ptr(pose), ops._ptr(n_inl), ops._ptr(rmse), ops._ptr(n_el),
        ops._ptr(best), ops._ptr(upd), ops._ptr(msk), ops._ptr(rs), ops._ptr(sr), ops._ptr(sp),
        ops._ptr(sc), ops._stream()), 'fgr_compat_pose')
    out = {'pose': pose, 'n_inliers': n_inl, 'n_eligible': n_el, 'inlier_rmse': rmse,
           'best_seed': best, 'n_updates': upd}
    if mask:
        out['mask'] = list(torch.split(msk.bool(), lengths))
    if seeds:
        out['seed_row'], out['seed_pose'], out['seed_count'] = sr, sp, sc
    if scores:
        out['row_score'] = list(torch.split(rs, lengths))
    return out


def correspondences(outputs, layer=-1):
    """The rows the forward's pose stage solves from, per pair:
    a = [src_kp ; tgt_kp_warped[layer]], b = [src_kp_warped[layer] ; tgt_kp],
    w = sigmoid([src_overlap[layer] ; tgt_overlap[layer]]) -> three lists."""
    a, b, w = [], [], []
    for p in range(len(outputs['src_kp'])):
        a.append(torch.cat([outputs['src_kp'][p], outputs['tgt_kp_warped'][p][layer]], 0))
        b.append(torch.cat([outputs['src_kp_warped'][p][layer], outputs['tgt_kp'][p]], 0))
        w.append(torch.sigmoid(torch.cat([outputs['src_overlap'][p][layer].reshape(-1),
                                          outputs['tgt_overlap'][p][layer].reshape(-1)], 0)))
    return a, b, w


def ransac_outputs(outputs, inlier_dist, layer=-1, **kw):
    """``ransac`` on the forward's correspondences of decoder layer ``layer``, weighted by the
    predicted overlap (``w_min`` thresholds it, as the forward's pose stage thresholds its
    weights); keyword arguments as ``ransac``. The returned ``pose`` starts ``fgreg.icp``."""
    a, b, w = correspondences(outputs, layer)
    return ransac(a, b, w, inlier_dist=inlier_dist, **kw)


def compat_outputs(outputs, compat_dist, inlier_dist, layer=-1, **kw):
    """``compat`` on the forward's correspondences of decoder layer ``layer``, as
    ``ransac_outputs``; keyword arguments as ``compat``."""
    a, b, w = correspondences(outputs, layer)
    return compat(a, b, w, compat_dist=compat_dist, inlier_dist=inlier_dist, **kw)
