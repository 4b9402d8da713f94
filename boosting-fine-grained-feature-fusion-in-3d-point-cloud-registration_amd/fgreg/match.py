"""Correspondences from the forward's descriptors: mutual nearest neighbours on the GPU.

The forward returns per-point descriptors (``src_feat`` / ``tgt_feat``, ``src_feat_un`` /
``tgt_feat_un``) that two of the three loss families train to match across the clouds; every
pose stage consumes only the regressed coordinates. This module matches the descriptors
(csrc/match.hip behind ``fgr_feature_nn`` and ``fgr_match_pairs``; the semantics are stated in
include/fgreg.h and restated in tests/_match_ref.py) and hands ``fgreg.ransac`` what it takes:

    out = model(batch)
    rob = fgreg.register_features(out, inlier_dist=0.1, model=model)
    ref = fgreg.icp(batch['src_xyz'], batch['tgt_xyz'], rob['pose'], max_corr_dist=0.05)

and, with a ground-truth pose, the descriptor metrics of the 3DMatch literature (Inlier Ratio
per pair, Feature-Matching Recall over pairs).

Opt-in (nothing in the forward calls it), GPU only (host tensors raise FgrError), on the
current stream, never synchronising: one launch finds every row's neighbour in both directions
of every pair, one more builds the correspondence rows, 0 / 1 weights and counts; rows that do
not take part keep weight 0 instead of being compacted, so no length is read back. The products
are always the fp32-accurate f16x3 ones, whatever ``fgreg.set_precision`` says. A call can be
captured into a graph after one eager call with the same lengths (the tables of a tuple of
lengths are uploaded once and kept).
"""
import torch

from . import _lib, ops
from .robust import _packed, _rows

METRICS = {'dot': 0, 'euclidean': 1, 'bilinear': 0}       # FGR_MATCH_DOT / FGR_MATCH_EUCLID
MODES = {'src': 0, 'mutual': 1, 'bilateral': 2}           # FGR_MATCH_SRC / MUTUAL / BILATERAL

_TABLES = {}        # (device, src lengths, tgt lengths) -> (off, kv_seg, out_off)


def _tables(ns, nt, device):
    key = (str(device), tuple(ns), tuple(nt))
    ent = _TABLES.get(key)
    if ent is None:
        if len(_TABLES) > 4096:
            _TABLES.clear()
        B = len(ns)
        ent = _TABLES[key] = (
            ops.offsets(list(ns) + list(nt), device),
            ops.to_device([(c + B) % (2 * B) for c in range(2 * B)], torch.int32, device),
            ops.offsets([a + b for a, b in zip(ns, nt)], device))
    return ent


def _feats(x, what):
    xs = [x] if torch.is_tensor(x) else list(x)
    ops._dev(*xs)
    for t in xs:
        if t.dtype != torch.float32 or t.dim() != 2:
            raise _lib.FgrError(f'{what}: expected float32 of shape (n, d), got {tuple(t.shape)} {t.dtype}')
    return xs


def feature_nn(q, k, off, kv_off, kv_seg, max_q_len, metric):
    """fgr_feature_nn on packed rows -> (nn_idx int32, best, second), one element per query row."""
    n_q, d = int(q.shape[0]), int(q.shape[1])
    L = _lib.load()
    if not L.fgr_feature_nn_supported(d) or int(k.shape[1]) != d:
        raise _lib.FgrError(f'feature matching needs a descriptor width d with d % 32 == 0 and '
                            f'32 <= d <= 512, got {d} and {int(k.shape[1])}')
    dev = q.device
    nn = torch.empty(n_q, dtype=torch.int32, device=dev)
    best = torch.empty(n_q, dtype=torch.float32, device=dev)
    second = torch.empty(n_q, dtype=torch.float32, device=dev)
    _lib.check(L.fgr_feature_nn(
        ops._ptr(q), ops._ptr(k), d, n_q, int(k.shape[0]), ops._ptr(off), ops._ptr(kv_off),
        ops._ptr(kv_seg), int(kv_seg.numel()), int(max_q_len), int(metric), ops._ptr(nn),
        ops._ptr(best), ops._ptr(second), ops._stream()), 'fgr_feature_nn')
    return nn, best, second


def _aligned(x):
    x = x.contiguous()
    return x if x.data_ptr() % 16 == 0 else x.clone()


def match_features(src_feat, tgt_feat, src_xyz, tgt_xyz, *, metric='euclidean', mode='mutual',
                   W=None, max_ratio=None, pose=None, inlier_dist=None):
    """Nearest neighbours in descriptor space, both ways, as weighted correspondences.

    src_feat, tgt_feat: lists of per-pair (n, d) float32 GPU tensors, or one tensor each for a
    single pair; src_xyz, tgt_xyz: the points they describe, (n, 3). ``metric``: 'euclidean',
    'dot', or 'bilinear' with the InfoNCE parameter ``W`` (queries X W_sym, W_sym = triu(W) +
    triu(W)^T, keys X, then 'dot'; one f16x3 product over all rows serves both directions).
    ``mode``: 'src' (every source row and its neighbour), 'mutual' (the source rows whose
    neighbour points back) or 'bilateral' (every row of both clouds). ``max_ratio``: Lowe's
    ratio test, best distance < max_ratio * second-best ('euclidean' only).

    Returns a dict of device tensors: per-pair lists ``a``, ``b`` (ns + nt, 3) and ``w``
    (ns + nt,) in the row layout of ``fgreg.robust.correspondences`` (source rows, then target
    rows; b ~ R a + t; w is 0 / 1 and nothing is compacted), ``nn_src``, ``nn_tgt`` (int32, -1
    without a neighbour), ``score_src``, ``score_tgt`` (the best score, or squared distance for
    'euclidean') and ``n_matches`` (B,) int32; with ``pose`` ((B, 3, 4) or (3, 4), source to
    target) and ``inlier_dist`` also ``n_inliers`` and ``inlier_ratio`` = n_inliers /
    max(1, n_matches)."""
    if metric not in METRICS or mode not in MODES:
        raise _lib.FgrError(f'metric {metric!r} / mode {mode!r}: expected one of {sorted(METRICS)} '
                            f'/ {sorted(MODES)}')
    if (metric == 'bilinear') != (W is not None):
        raise _lib.FgrError("metric='bilinear' and W go together")
    if max_ratio is not None and metric != 'euclidean':
        raise _lib.FgrError("max_ratio is the ratio of two distances: metric='euclidean' only")
    if (pose is None) != (inlier_dist is None):
        raise _lib.FgrError('pose and inlier_dist go together')
    fs, ft = _feats(src_feat, 'src_feat'), _feats(tgt_feat, 'tgt_feat')
    xs, xt = _rows(src_xyz, 3, 'src_xyz'), _rows(tgt_xyz, 3, 'tgt_xyz')
    ns, nt = [int(t.shape[0]) for t in fs], [int(t.shape[0]) for t in ft]
    B = len(ns)
    if not B or len(nt) != B or [int(t.shape[0]) for t in xs] != ns or [int(t.shape[0]) for t in xt] != nt:
        raise _lib.FgrError('features and points need the same number of pairs and rows per cloud')
    widths = {int(t.shape[1]) for t in fs + ft}
    if len(widths) != 1:
        raise _lib.FgrError(f'descriptor widths differ: {sorted(widths)}')
    dev = fs[0].device
    off, kv_seg, out_off = _tables(ns, nt, dev)
    keys = _aligned(torch.cat(fs + ft, 0))
    xyz = torch.cat(xs + xt, 0)
    if W is not None:
        from . import linear, loss
        ops._dev(W)
        with linear.mode_scope('f16x3'):                    # also in bf16 mode
            queries = linear.linear(keys, loss._w_sym(W))
    else:
        queries = keys
    nn, best, second = feature_nn(queries, keys, off, off, kv_seg, max(ns + nt), METRICS[metric])

    n_rows, n_s = sum(ns) + sum(nt), sum(ns)
    a = torch.empty(n_rows, 3, dtype=torch.float32, device=dev)
    b = torch.empty(n_rows, 3, dtype=torch.float32, device=dev)
    w = torch.empty(n_rows, dtype=torch.float32, device=dev)
    n_match = torch.empty(B, dtype=torch.int32, device=dev)
    gt = n_inl = None
    if pose is not None:
        ops._dev(pose)
        gt = pose.detach().to(torch.float32).reshape(-1, 3, 4).contiguous()
        if gt.shape[0] != B:
            raise _lib.FgrError(f'pose: expected ({B}, 3, 4), got {tuple(pose.shape)}')
        n_inl = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().fgr_match_pairs(
        ops._ptr(nn), ops._ptr(best), ops._ptr(second), ops._ptr(xyz), n_rows, ops._ptr(off),
        ops._ptr(out_off), B, MODES[mode], float(max_ratio) if max_ratio is not None else 0.0,
        ops._ptr(gt), float(inlier_dist) if inlier_dist is not None else 0.0, ops._ptr(a),
        ops._ptr(b), ops._ptr(w), ops._ptr(n_match), ops._ptr(n_inl), ops._stream()),
        'fgr_match_pairs')
    both = [s + t for s, t in zip(ns, nt)]
    out = {'a': list(torch.split(a, both)), 'b': list(torch.split(b, both)),
           'w': list(torch.split(w, both)),
           'nn_src': list(torch.split(nn[:n_s], ns)), 'nn_tgt': list(torch.split(nn[n_s:], nt)),
           'score_src': list(torch.split(best[:n_s], ns)),
           'score_tgt': list(torch.split(best[n_s:], nt)), 'n_matches': n_match}
    if pose is not None:
        out['n_inliers'] = n_inl
        out['inlier_ratio'] = n_inl.float() / n_match.clamp(min=1).float()
    return out


def match_outputs(outputs, model=None, layer=-1, features='cond', **kw):
    """``match_features`` on a forward's descriptors: ``features='cond'`` takes layer ``layer``
    of ``src_feat`` / ``tgt_feat``, ``'un'`` takes ``src_feat_un`` / ``tgt_feat_un``; the points
    are ``src_kp`` / ``tgt_kp``. With ``model`` and no ``metric`` the metric is the one the
    descriptors were trained under: 'bilinear' with the model's InfoNCE parameter for
    ``feature_loss_type == 'infonce'``, 'euclidean' for 'circle'."""
    if features not in ('cond', 'un'):
        raise _lib.FgrError(f"features {features!r}: expected 'cond' or 'un'")
    if features == 'cond':
        fs = [f[layer] for f in outputs['src_feat']]
        ft = [f[layer] for f in outputs['tgt_feat']]
    else:
        fs, ft = list(outputs['src_feat_un']), list(outputs['tgt_feat_un'])
    if model is not None and 'metric' not in kw:
        kind = model.cfg.get('feature_loss_type', 'infonce')
        if kind == 'infonce':
            crit = model.feature_criterion if features == 'cond' else model.feature_criterion_un
            kw['metric'], kw['W'] = 'bilinear', crit.W
        elif kind == 'circle':
            kw['metric'] = 'euclidean'
        else:
            raise _lib.FgrError(f'no matching metric for feature_loss_type {kind!r}')
    return match_features(fs, ft, list(outputs['src_kp']), list(outputs['tgt_kp']), **kw)


def register_features(outputs, inlier_dist, model=None, layer=-1, features='cond', n_hyp=4096,
                      seed=0, n_refits=4, mask=False, estimator='ransac', compat_dist=None,
                      n_seeds=64, k=16, **kw):
    """``match_outputs``, then ``fgreg.ransac`` on its rows and weights -> RANSAC's dict plus
    the match dict under ``'matches'``. ``n_hyp``, ``seed``, ``n_refits`` and ``mask`` go to
    ``ransac``, every other keyword to ``match_outputs`` (a ground-truth ``pose`` is scored at
    ``inlier_dist`` unless another is given). The returned ``pose`` starts ``fgreg.icp``.
    ``estimator='compat'`` estimates with ``fgreg.compat`` instead, for matches with few
    inliers: ``compat_dist`` (default ``inlier_dist``), ``n_seeds`` and ``k`` go to it, ``n_hyp``
    and ``seed`` are ignored, and the dict carries ``best_seed`` in the place of ``best_hyp``."""
    from .robust import compat, ransac
    if estimator not in ('ransac', 'compat'):
        raise _lib.FgrError(f"estimator {estimator!r}: expected 'ransac' or 'compat'")
    if kw.get('pose') is not None:
        kw.setdefault('inlier_dist', inlier_dist)
    m = match_outputs(outputs, model=model, layer=layer, features=features, **kw)
    if estimator == 'compat':
        out = compat(m['a'], m['b'], m['w'], inlier_dist=inlier_dist, n_seeds=n_seeds, k=k,
                     compat_dist=inlier_dist if compat_dist is None else compat_dist,
                     n_refits=n_refits, mask=mask)
    else:
        out = ransac(m['a'], m['b'], m['w'], inlier_dist=inlier_dist, n_hyp=n_hyp, seed=seed,
                     n_refits=n_refits, mask=mask)
    out['matches'] = m
    return out


def feature_match_recall(inlier_ratio, tau=0.05):
    """Feature-Matching Recall: the share of pairs whose inlier ratio exceeds ``tau``."""
    return (inlier_ratio > tau).float().mean()
