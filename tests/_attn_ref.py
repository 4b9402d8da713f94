"""The attention reference of the GPU tests, in one place: packed-segment multi-head softmax
attention on the CPU in the dtype of its inputs (fp64: the reference; fp32: the "fp32
restatement" whose error sets the bounds), with the training forward's attention-weight dropout
and log2-sum-exp, the sum|terms| denominators of every output, and the seeded cases of
test_attn_ref.py (CPU) and test_gpu_attention_train.py (GPU). Not a conftest: imported.

Semantics (include/fgreg.h): query segment i (rows q_off[i]..q_off[i+1]) attends key segment
kv_seg[i]; head h owns columns [h dh, (h + 1) dh). S = scale Q K^T, P = softmax(S). With dropout
(seed, p) the mask M of an entry is 0 where attn_drop_hash(seed, head, packed query row, packed
key row) < p 2^32 and 1 / (1 - p) elsewhere (fgreg.autograd.attn_drop_mask restates the hash);
the softmax sum runs over every weight and only the PV product sees M:
  O = (P o M) V            lse2 = log2 sum_k exp2(scale log2(e) q.k)   (of the undropped softmax)
  dV = (P o M)^T dO        dP = M o (dO V^T)        D = rowsum(dO o O) = rowsum(P o dP)
  dS = P o (dP - D)        dQ = scale dS K          dK = scale dS^T Q

sum|terms| per element (the denominators of _cond_err; M = 1 without dropout)
  o   (P o M) |V|
  a = M o (|dO| |V|^T), G = P o (a + rowsum(P o a)) bounds |dS| term by term, so
  dq  scale G |K|          dk  scale G^T |Q|          dv  (P o M)^T |dO|
An element whose terms all vanish (a (row, head) whose every weight is dropped, a key row that
no query segment attends) has denominator 0 and reference 0: the kernels must give an exact 0.

A non-empty query segment on an empty key segment is a softmax over nothing, outside the
contract; no case contains one.
"""
import functools
import math
import types

import numpy as np
import torch

LN2 = math.log(2.0)

# name -> (query segment lengths, key segment lengths, kv_seg)
_LENS = [130, 0, 1, 64, 65, 300, 128]
SEGS = {
    # every segment attends itself: an empty segment, a one-row segment (one key), a full tile,
    # one row past a tile, five tiles with a partial last one, two full tiles
    'self': (_LENS, _LENS, [0, 1, 2, 3, 4, 5, 6]),
    # key segment 5 is shared by query segments 0 (3 tiles) and 2 (1 tile), key segment 0 by 5
    # (5 tiles) and 6 (2 tiles); key segments 2 and 6 (129 rows) are attended by nobody; the
    # empty segment attends itself
    'mixed': (_LENS, _LENS, [5, 1, 5, 4, 3, 0, 0]),
    # keys of their own row space: 330 key rows, 260 query rows
    'separate': ([130, 1, 64, 65], [65, 200, 1, 64], [1, 0, 3, 2]),
}
REGIMES = ('unit', 'peaked', 'blocks')
# (seed, p): at nhead 2 on 'self' the first drops the only key of row 130 in exactly one head,
# the second and third in both (test_attn_ref.py asserts it)
DROPS = ((987654321, 0.3), (0, 0.9), (0xFFFFFFFF, 0.9), (12345, 0.01))
NAMES = ('o', 'dq', 'dk', 'dv')
# added to every case's seed; test_attn_ref.py asserts the conditions the cases rely on, so
# another value that voids one fails there
SALT = 2


def p32(p):
    """The dropout probability as the C ABI receives it (a float)."""
    return float(np.float32(p))


def drop_scale(seed, p, head, q_rows, k_rows, dtype):
    """M: 0 (dropped) or 1 / (1 - p) (kept) over packed query x key rows."""
    from fgreg.autograd import attn_drop_mask
    dropped = attn_drop_mask(seed, p32(p), head, q_rows, k_rows)
    keep = torch.from_numpy(~np.asarray(dropped, dtype=bool)).to(dtype)
    return keep * torch.tensor(1.0 / (1.0 - p32(p)), dtype=torch.float64).to(dtype)


def mha(q, k, v, qlens, klens, kv_seg, nhead, scale, R=None, dens=None, drop=None,
        with_lse=False):
    """Packed-segment multi-head softmax attention in the dtype of q on the CPU. ``dens`` (a
    dict): filled with sum|terms| of the output ('o') and, given the cotangent R, of the three
    gradients ('dq', 'dk', 'dv'); see the module docstring. ``drop`` = (seed, p): attention-weight
    dropout. ``with_lse``: returns (out, lse2 of shape (rows, nhead)) instead of out."""
    d = q.shape[1]
    dh = d // nhead
    qo, ko = np.cumsum([0] + list(qlens)), np.cumsum([0] + list(klens))
    out = torch.zeros(q.shape[0], v.shape[1], dtype=q.dtype)
    dv_w = v.shape[1] // nhead
    if dens is not None:
        dens['o'] = torch.zeros_like(out)
        for name, t in (('dq', q), ('dk', k), ('dv', v)):
            dens[name] = torch.zeros(t.shape, dtype=q.dtype)
    outs, lses = [], []
    for i in range(len(qlens)):
        j = kv_seg[i]
        heads, lse_h = [], []
        for h in range(nhead):
            qs = q[qo[i]:qo[i + 1], h * dh:(h + 1) * dh]
            ks = k[ko[j]:ko[j + 1], h * dh:(h + 1) * dh]
            vs = v[ko[j]:ko[j + 1], h * dv_w:(h + 1) * dv_w]
            s = (qs * scale) @ ks.t()
            p = torch.softmax(s, -1)
            m = None
            if drop is not None:
                m = drop_scale(drop[0], drop[1], h, np.arange(qo[i], qo[i + 1]),
                               np.arange(ko[j], ko[j + 1]), q.dtype)
            pm = p if m is None else p * m
            heads.append(pm @ vs)
            if with_lse:
                lse_h.append(torch.logsumexp(s, -1) / LN2)
            if dens is not None:
                with torch.no_grad():
                    dens['o'][qo[i]:qo[i + 1], h * dv_w:(h + 1) * dv_w] = pm @ vs.abs()
                    if R is not None:
                        do = R[qo[i]:qo[i + 1], h * dv_w:(h + 1) * dv_w].abs()
                        a = do @ vs.abs().t()
                        if m is not None:
                            a = a * m
                        g = p * (a + (p * a).sum(-1, keepdim=True))
                        dens['dq'][qo[i]:qo[i + 1], h * dh:(h + 1) * dh] += scale * (g @ ks.abs())
                        dens['dk'][ko[j]:ko[j + 1], h * dh:(h + 1) * dh] += scale * (g.t() @ qs.abs())
                        dens['dv'][ko[j]:ko[j + 1], h * dv_w:(h + 1) * dv_w] += pm.t() @ do
        outs.append(torch.cat(heads, 1))
        if with_lse:
            lses.append(torch.stack(lse_h, 1))
    o = torch.cat(outs, 0)
    return (o, torch.cat(lses, 0)) if with_lse else o


def cond_err(got, ref, den):
    """max_i |got_i - ref_i| / den_i, den_i = sum|terms| of element i (fp64). An element whose
    terms are all zero has den 0 and ref 0: anything but an exact 0 there is an error."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == den.shape, (got.shape, ref.shape, den.shape)
    assert bool(torch.isfinite(got).all())
    if got.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / den.clamp_min(1e-300)).max())


def tile_ids(lens):
    """The 64-row tile of every packed row, numbered through the segments (a segment's tiles
    start at its first row, as the kernels' images do)."""
    ids, nxt = [], 0
    for n in lens:
        ids.append(nxt + np.arange(n) // 64)
        nxt += (n + 63) // 64
    return np.concatenate(ids).astype(np.int64) if ids else np.zeros(0, np.int64), nxt


def inputs(regime, seg, nhead, dh):
    """(q, k, v, dO) fp32 of one seeded case.
      unit    randn.
      peaked  q * 3: scores reach about +-12, P spans about 1e-10 .. 1.
      blocks  per head h, q *= 2^-a_h and k *= 2^a_h (a_h in -8 .. 8); k per (64-row tile, head)
              *= 2^(-1 .. 1); v and dO per (64-row tile, head) *= 2^(-8 .. 8). Scores stay O(1),
              every tile and head carries another scale exponent. All factors are exact powers
              of two."""
    qlens, klens, _ = SEGS[seg]
    d = nhead * dh
    seed = SALT + 100003 * REGIMES.index(regime) + 1009 * list(SEGS).index(seg) + 17 * nhead + dh
    g = torch.Generator().manual_seed(seed)
    nq, nk = sum(qlens), sum(klens)
    q, k = torch.randn(nq, d, generator=g), torch.randn(nk, d, generator=g)
    v, R = torch.randn(nk, d, generator=g), torch.randn(nq, d, generator=g)
    if regime == 'peaked':
        q = q * 3
    elif regime == 'blocks':
        def pw(lo, hi, shape):
            return torch.randint(lo, hi + 1, shape, generator=g).double()
        tq, ntq = tile_ids(qlens)
        tk, ntk = tile_ids(klens)
        a = pw(-8, 8, (nhead,))
        ek, ev, eo = pw(-1, 1, (ntk, nhead)), pw(-8, 8, (ntk, nhead)), pw(-8, 8, (ntq, nhead))
        col = lambda e: torch.exp2(e).float().repeat_interleave(dh, dim=-1)
        q = q * col(-a)
        k = k * col(a) * col(ek[tk])
        v = v * col(ev[tk])
        R = R * col(eo[tq])
    return q, k, v, R


def closed_form(q, k, v, R, qlens, klens, kv_seg, nhead, scale, drop=None):
    """(dq, dk, dv) evaluated directly from the formulas of the module docstring."""
    dh = q.shape[1] // nhead
    qo, ko = np.cumsum([0] + list(qlens)), np.cumsum([0] + list(klens))
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    for i in range(len(qlens)):
        j = kv_seg[i]
        for h in range(nhead):
            c = slice(h * dh, (h + 1) * dh)
            qs, ks, vs = q[qo[i]:qo[i + 1], c], k[ko[j]:ko[j + 1], c], v[ko[j]:ko[j + 1], c]
            do = R[qo[i]:qo[i + 1], c]
            p = torch.softmax((qs * scale) @ ks.t(), -1)
            m = torch.ones_like(p)
            if drop is not None:
                m = drop_scale(drop[0], drop[1], h, np.arange(qo[i], qo[i + 1]),
                               np.arange(ko[j], ko[j + 1]), q.dtype)
            dp = m * (do @ vs.t())
            ds = p * (dp - (p * dp).sum(-1, keepdim=True))
            dq[qo[i]:qo[i + 1], c] += scale * (ds @ ks)
            dk[ko[j]:ko[j + 1], c] += scale * (ds.t() @ qs)
            dv[ko[j]:ko[j + 1], c] += (p * m).t() @ do
    return dq, dk, dv


def run(q, k, v, R, seg, nhead, dtype, drop=None, dens=None):
    """Forward and autograd backward of sum(o * R) in ``dtype`` -> dict o, lse, dq, dk, dv."""
    qlens, klens, kv_seg = SEGS[seg]
    scale = math.sqrt(1.0 / (q.shape[1] // nhead))
    ql, kl, vl = (t.to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    o, lse = mha(ql, kl, vl, qlens, klens, kv_seg, nhead, scale, R=R.to(dtype), dens=dens,
                 drop=drop, with_lse=True)
    (o * R.to(dtype)).sum().backward()
    return {'o': o.detach(), 'lse': lse.detach(), 'dq': ql.grad, 'dk': kl.grad, 'dv': vl.grad}


@functools.lru_cache(maxsize=None)
def case(regime, seg, nhead, dh, drop=None):
    """One seeded case, computed once and shared (read-only) by every test that needs it:
    .q .k .v .R (fp32), .ref (fp64 o, lse, dq, dk, dv), .dens (sum|terms| of o, dq, dk, dv),
    .e32 (the fp32 restatement's error: per element over sum|terms| for o / dq / dk / dv,
    absolute for lse), .qlens .klens .kv_seg .scale."""
    q, k, v, R = inputs(regime, seg, nhead, dh)
    dens = {}
    ref = run(q, k, v, R, seg, nhead, torch.float64, drop, dens)
    r32 = run(q, k, v, R, seg, nhead, torch.float32, drop)
    e32 = {n: cond_err(r32[n], ref[n], dens[n]) for n in NAMES}
    e32['lse'] = float((r32['lse'].double() - ref['lse']).abs().max())
    qlens, klens, kv_seg = SEGS[seg]
    return types.SimpleNamespace(q=q, k=k, v=v, R=R, ref=ref, dens=dens, e32=e32, qlens=qlens,
                                 klens=klens, kv_seg=kv_seg, nhead=nhead, dh=dh, drop=drop,
                                 scale=math.sqrt(1.0 / dh), regime=regime, seg=seg)


# ---- the cases of test_gpu_attention_train.py (test_attn_ref.py pins their conditions) ----------
BASE = [(r, s) for r in REGIMES for s in ('self', 'mixed')] + [('unit', 'separate')]
# forward, p = 0 and p > 0: unit at every (seed, p), peaked and blocks at the first only
FWD_P0 = [(r, s, None) for r, s in BASE]
FWD_DROP = ([('unit', s, dr) for s in SEGS for dr in DROPS] +
            [(r, s, DROPS[0]) for r, s in BASE if r != 'unit'])
# f16x3 backward: R1 (p = 0), R2 (p > 0; the all-dropped (row, head) pairs on unit / self)
BWD_P0 = FWD_P0
BWD_DROP = [(r, s, DROPS[0]) for r, s in BASE] + [('unit', 'self', dr) for dr in DROPS[1:]]
# fp32-MFMA backward (R3 - R5)
MFMA = [('unit', 'mixed'), ('blocks', 'mixed'), ('unit', 'separate')]
MFMA_P0 = [(r, s, None) for r, s in MFMA]
# (the all-dropped (row, head) pairs of unit / self too)
MFMA_DROP = [(r, s, DROPS[0]) for r, s in MFMA] + [('unit', 'self', DROPS[1])]
# head-index stride: (nhead, dh) besides the default nhead 2
HEADS = [(3, 32), (8, 32)]


def all_cases():
    """Every (regime, seg, nhead, dh, drop) the GPU module runs."""
    out = []
    for dh in (32, 64):
        out += [(r, s, 2, dh, dr) for r, s, dr in FWD_P0 + FWD_DROP + BWD_DROP]
    for dh in (16, 32, 64):
        out += [(r, s, 2, dh, dr) for r, s, dr in MFMA_P0 + MFMA_DROP]
    out += [('unit', 'mixed', 2, 8, None), ('unit', 'mixed', 2, 8, DROPS[0])]
    for nhead, dh in HEADS:
        out += [('unit', 'mixed', nhead, dh, None), ('unit', 'mixed', nhead, dh, DROPS[0])]
    return sorted(set(out), key=repr)
