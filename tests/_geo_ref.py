"""Host restatement of the geometric structure embedding (fgreg.transformer.
GeometricStructureEmbedding; position_embedding.py:129-196), for the tests and for the fixture
generator (tests/golden/make_golden_geo_pe.py). Torch on the CPU, in the dtype it is asked for:
float64 is the checker, float32 the "what plain fp32 gives" baseline of the acceptance rule.

For point i of a cloud, nn(i) = its k nearest OTHER points of the same cloud (i excluded by index,
ties in squared distance to the lower index),

    d_ij  = |p_j - p_i| / sigma_d                                               j in nn(i)
    a_ijr = atan2(|(p_r - p_i) x (p_j - p_i)|, (p_r - p_i) . (p_j - p_i)) * 180 / (sigma_a pi)
    E(t)  = [sin(t w_0), cos(t w_0), sin(t w_1), cos(t w_1), ...],  w_m = exp(-2 m ln(1e4) / D)
    out_i = max_j [ proj_d(E(d_ij)) + red_r proj_a(E(a_ijr)) ],   red = max | mean, per channel
"""
import math

import numpy as np
import torch


def div_term(D, dtype=torch.float64):
    """w_m as the module's buffer holds it: computed in fp32 (position_embedding.py:108-110)."""
    w = torch.exp(torch.arange(0, D, 2).float() * (-math.log(10000.0) / D))
    return w.to(dtype)


def knn(xyz, lengths, k, dtype=np.float64):
    """(N, k) int64 packed row indices: per cloud, the k nearest other points by squared
    distance from coordinate differences evaluated in ``dtype`` ((dx dx + dy dy) + dz dz), the
    point itself excluded by index, ties to the lower index (stable sort)."""
    x = np.asarray(xyz, dtype)
    out, o = [], 0
    for n in lengths:
        p = x[o:o + n]
        df = p[None, :, :] - p[:, None, :]
        d2 = (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]
        d2[np.arange(n), np.arange(n)] = np.inf
        out.append(np.argsort(d2, axis=1, kind='stable')[:, :k] + o)
        o += n
    return np.concatenate(out).astype(np.int64)


def knn_margin(xyz, lengths, k):
    """Per point, the relative gap in fp64 squared distance between its k-th and (k+1)-th nearest
    other point of its cloud, (d2_{k+1} - d2_k) / d2_{k+1} (inf in a cloud of exactly k + 1
    points): below ~1e-4 an fp32 evaluation may rank the two the other way."""
    x = np.asarray(xyz, np.float64)
    out, o = [], 0
    for n in lengths:
        p = x[o:o + n]
        d2 = ((p[None] - p[:, None]) ** 2).sum(-1)
        d2[np.arange(n), np.arange(n)] = np.inf
        s = np.sort(d2, axis=1)
        if n > k + 1:
            out.append((s[:, k] - s[:, k - 1]) / np.maximum(s[:, k], 1e-300))
        else:
            out.append(np.full(n, np.inf))
        o += n
    return np.concatenate(out)


def indices(xyz, nn, sigma_d, sigma_a, dtype=torch.float64):
    """d (N, k), a (N, k, k) [i][j][r] for given neighbours nn (N, k)."""
    x = torch.as_tensor(np.asarray(xyz)).to(dtype)
    nn = torch.as_tensor(np.asarray(nn)).long()
    v = x[nn] - x[:, None, :]                                   # (N, k, 3): p_nn - p_i
    d = v.norm(dim=-1) / sigma_d
    ref, anc = v[:, None, :, :], v[:, :, None, :]               # [i][j][r]: ref = v_r, anc = v_j
    sin = torch.linalg.norm(torch.cross(ref.expand(-1, v.shape[1], -1, -1),
                                        anc.expand(-1, -1, v.shape[1], -1), dim=-1), dim=-1)
    cos = (ref * anc).sum(-1)
    a = torch.atan2(sin, cos) * (180.0 / (sigma_a * math.pi))
    return d, a


def sin_embed(t, w):
    """E(t): (*) -> (*, 2 len(w)), interleaved sin / cos."""
    om = t.unsqueeze(-1) * w
    return torch.stack([torch.sin(om), torch.cos(om)], dim=-1).reshape(*t.shape, 2 * w.numel())


def embed(d, a, w, Wd, bd, Wa, ba, reduction):
    """out (N, D) from d (N, k), a (N, k, k); every operand in d's dtype."""
    dt = d.dtype
    pd = sin_embed(d, w.to(dt)) @ Wd.to(dt).t() + bd.to(dt)             # (N, k, D)
    pa = sin_embed(a, w.to(dt)) @ Wa.to(dt).t() + ba.to(dt)             # (N, k, k, D)
    pa = pa.max(dim=2)[0] if reduction == 'max' else pa.mean(dim=2)
    return (pd + pa).max(dim=1)[0]


def forward(xyz, lengths, k, sigma_d, sigma_a, w, Wd, bd, Wa, ba, reduction, nn=None,
            dtype=torch.float64):
    """The whole definition; ``nn`` given: those neighbours instead of knn()'s."""
    if nn is None:
        nn = knn(xyz, lengths, k)
    d, a = indices(xyz, nn, sigma_d, sigma_a, dtype)
    return embed(d, a, w, Wd, bd, Wa, ba, reduction)


def max_gaps(d, a, w, Wd, bd, Wa, ba, reduction):
    """(N, D): per output, the smallest gap between the largest and the second largest candidate
    over the maxima that output takes (over r for every j with reduction 'max', then over j), in
    d's dtype. Where an evaluation's error stays below the gap it picks the same arg-max, so its
    gradient routes through the same embedding rows; at a tie the derivative is not defined."""
    dt = d.dtype
    pd = sin_embed(d, w.to(dt)) @ Wd.to(dt).t() + bd.to(dt)
    pa = sin_embed(a, w.to(dt)) @ Wa.to(dt).t() + ba.to(dt)
    gap = torch.full_like(pd[:, 0], float('inf'))
    if d.shape[1] < 2:
        return gap
    if reduction == 'max':
        t = pa.topk(2, dim=2)[0]
        gap = (t[:, :, 0] - t[:, :, 1]).min(dim=1)[0]
        pa = pa.max(dim=2)[0]
    else:
        pa = pa.mean(dim=2)
    t = (pd + pa).topk(2, dim=1)[0]
    return torch.minimum(gap, t[:, 0] - t[:, 1])
