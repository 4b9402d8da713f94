"""The deformable / modulated KPConv gather (finegrained_kpconv_blocks.py:270-345, :384-399)
restated in torch in any dtype (fp64: the checker; fp32: the yardstick of the project's error
bound), differentiable in x, W, kp_q and mod, and the test tables of test_kpconv_deform.py and
test_gpu_kpconv_deform.py. Not a conftest: imported by the tests that use it, as _kpconv_modes.py.

Semantics. With per-query kernel points kp_q (nq, K, 3), modulations mod (nq, K) or None and
d2[q, h, k] = |(s[idx[q, h]] - q) - kp_q[q, k]|^2, a valid neighbour is IN RANGE iff d2 < e^2
for some k; one that is not is treated exactly like a shadow (zero feature row: what the
reference's topk re-indexing at :319-343 amounts to). Then
  wf[q, k, :] = mod[q, k] * sum_{in-range h} w(d2[q, h, k]) x[idx[q, h], :]
  nnorm[q]    = max(1, #{in-range h : sum_c x[idx[q, h], c] > 0})
and the in-range mask and the closest one-hot are constants of the gradient.

Edit rule. The function is discontinuous where a neighbour enters or leaves the range and where
the closest kernel point changes, the linear influence has a kink at the extent and its
derivative does not exist at distance 0 (the reference's is NaN there, the kernel returns 0). So a
valid entry of a test table becomes a shadow when, in fp64 and under its query's kp_q,
  (a) some |sqrt(d2) / e - 1| < 0.02         (the linear kink and the in-range flip),
  (b) the two smallest d2 are closer than 1e-3 e^2 (TIE of _kpconv_modes.py), or
  (c) min_k sqrt(d2) < 1e-3 e.
The builder asserts that (b) alone removes at most 2 % of the valid entries and all three at
most 20 % (measured over every shape of the GPU tests: 1.04 % and 15.7 % at worst), that on the
edited table the fp32 argmin and the fp32 in-range mask equal the fp64 ones for every live entry,
and that at least 20 live entries are in range and at least 20 are live but out of range.
"""
import functools

import numpy as np
import torch

import _kpconv_modes as km

EXT = km.EXT
COMBOS = [(i, a) for i in km.INFLUENCES for a in km.AGGREGATIONS]


def sq_distances(q, s, idx, kp_q):
    """(nq, H, K) squared distances of the centred neighbours to each query's own kernel points
    (:296-316 with deformed_K_points = kp_q.unsqueeze(1)); shadows name the appended far point."""
    sp = torch.cat([s, torch.full((1, 3), 1e6, dtype=s.dtype)])
    nb = sp[idx] - q.unsqueeze(1)
    return ((nb.unsqueeze(2) - kp_q.unsqueeze(1)) ** 2).sum(3)


def in_range(d2, extent):
    """(nq, H) bool, :325 (shadow entries are never in range: their point is 1e6 away)."""
    return (d2 < extent ** 2).any(2)


def gather_ref(q, s, idx, x, kp_q, mod, extent, influence, aggregation, dtype):
    """-> (wf (nq, K, cin), den = |mod| sum_h w_h |x_h|, nnorm (nq,)) in ``dtype`` on the CPU;
    differentiable in x, kp_q and mod."""
    q, s, kp_q, x = q.to(dtype), s.to(dtype), kp_q.to(dtype), x.to(dtype)
    d2 = sq_distances(q, s, idx, kp_q)
    keep = in_range(d2.detach(), extent)
    w = km.influences(d2, extent, influence, aggregation)                       # (nq, K, H)
    nx = torch.cat([x, torch.zeros(1, x.shape[1], dtype=dtype)])[idx]           # (nq, H, cin)
    nx = nx * keep.unsqueeze(2).to(dtype)
    wf, den = torch.matmul(w, nx), torch.matmul(w, nx.abs())
    if mod is not None:
        mod = mod.to(dtype)
        wf, den = wf * mod.unsqueeze(2), den * mod.abs().unsqueeze(2)
    cnt = torch.clamp((nx.detach().sum(-1) > 0).sum(-1), min=1)
    return wf, den, cnt.to(dtype)


def deform_points_ref(offset_features, kp, extent, modulated):
    """(kp_q, mod) of :272-306 from offset_features (nq, 3K or 4K)."""
    K = kp.shape[0]
    kp_q = kp + (offset_features[:, :3 * K] * extent).reshape(-1, K, 3)
    mod = 2 * torch.sigmoid(offset_features[:, 3 * K:]) if modulated else None
    return kp_q, mod


def deform_kpconv_ref(q, s, idx, x, W, kp, offset_W, offset_kp, offset_bias, extent, influence,
                      aggregation, modulated):
    """KPConv(deformable=True).forward in x's dtype -> (output, kp_q)."""
    off = km.kpconv_ref(q, s, idx, x, offset_W, offset_kp, extent, influence, aggregation) + offset_bias
    kp_q, mod = deform_points_ref(off, kp, extent, modulated)
    wf, _, cnt = gather_ref(q, s, idx, x, kp_q, mod, extent, influence, aggregation, x.dtype)
    return torch.einsum('qkc,kco->qo', wf, W) / cnt.unsqueeze(1), kp_q


def unsafe_entries(d2, extent, valid):
    """-> (rule (b) alone, rules (a) | (b) | (c)) of the module docstring, (nq, H) bool."""
    r = torch.sqrt(d2) / extent
    a = ((r - 1).abs() < 0.02).any(2)
    b = km.tie_gap(d2) < km.TIE * extent ** 2
    c = r.min(2).values < 1e-3
    return b & valid, (a | b | c) & valid


@functools.lru_cache(maxsize=None)
def table(cin, H, n_kp, nq=70, ns=90):
    """_kpconv_modes.table's recipe (70 queries over 90 supports, 60 % shadows, query 3 all shadow,
    extent 0.5, every feature row sum >= 1e-3 in magnitude) plus kp_q = kp + N(0, 0.2 extent) per
    query and mod uniform in (0.2, 1.8), edited by the rule of the module docstring.
    -> (q, s, idx, x, kp, kp_q, mod, cnt, stats): CPU tensors, cnt the exact normaliser."""
    rng = np.random.default_rng(1000 * cin + 10 * H + n_kp)
    s = rng.uniform(-1, 1, (ns, 3)).astype(np.float32)
    q = (s[rng.choice(ns, nq, replace=False)] + rng.normal(0, 0.01, (nq, 3))).astype(np.float32)
    idx = rng.integers(0, ns, (nq, H))
    idx[rng.uniform(size=(nq, H)) < 0.6] = ns
    idx[3] = ns
    x = rng.normal(size=(ns, cin)).astype(np.float32)
    rs = x.astype(np.float64).sum(1)
    x[np.abs(rs) < 1e-3, 0] += np.float32(0.5)
    kp = (rng.normal(size=(n_kp, 3)) * 0.3).astype(np.float32)
    kp_q = (kp[None] + rng.normal(0, 0.2 * EXT, (nq, n_kp, 3))).astype(np.float32)
    mod = rng.uniform(0.2, 1.8, (nq, n_kp)).astype(np.float32)
    q, s, x, kp, kp_q, mod, idx = (torch.from_numpy(a) for a in (q, s, x, kp, kp_q, mod, idx))
    valid = idx < ns
    n_valid = int(valid.sum())
    tie, bad = unsafe_entries(sq_distances(q.double(), s.double(), idx, kp_q.double()), EXT, valid)
    share_tie, share_all = int(tie.sum()) / n_valid, int(bad.sum()) / n_valid
    assert share_tie <= 0.02 and share_all <= 0.20, (cin, H, n_kp, share_tie, share_all)
    idx[bad] = ns
    assert bool((idx[3] == ns).all())
    live = idx < ns
    d64 = sq_distances(q.double(), s.double(), idx, kp_q.double())
    d32 = sq_distances(q, s, idx, kp_q)
    assert bool((torch.argmin(d64, 2) == torch.argmin(d32, 2))[live].all()), (cin, H, n_kp)
    keep = in_range(d64, EXT)
    assert bool((keep == in_range(d32, EXT))[live].all()), (cin, H, n_kp)
    n_in, n_out = int((keep & live).sum()), int((~keep & live).sum())
    assert n_in >= 20 and n_out >= 20, (cin, H, n_kp, n_in, n_out)
    nx = torch.cat([x.double(), torch.zeros(1, cin, dtype=torch.float64)])[idx]
    pos = nx.sum(-1) > 0
    cnt = torch.clamp((pos & keep).sum(-1), min=1).float()
    cnt_all = torch.clamp(pos.sum(-1), min=1).float()
    # the mask matters: a kernel that counts every valid neighbour gets another nnorm
    assert int((cnt != cnt_all).sum()) >= 1, (cin, H, n_kp)
    stats = dict(share_tie=share_tie, share_all=share_all, n_in=n_in, n_out=n_out,
                 n_live=int(live.sum()), nnorm_changed=int((cnt != cnt_all).sum()))
    return q, s, idx, x, kp, kp_q, mod, cnt, stats


@functools.lru_cache(maxsize=None)
def reference(cin, H, n_kp, influence, aggregation, modulated=True):
    """-> (wf fp64, den, e32): the fp64 gather of table(cin, H, n_kp), the condition-number
    denominator (for gaussian plus the subnormal term of _kpconv_modes.reference) and the torch
    fp32 restatement's own conditioned error against it."""
    q, s, idx, x, kp, kp_q, mod, _, _ = table(cin, H, n_kp)
    m = mod if modulated else None
    ref, den, _ = gather_ref(q, s, idx, x, kp_q, m, EXT, influence, aggregation, torch.float64)
    if influence == 'gaussian':
        den = den + H * 2.0 ** -126 * float(x.abs().max())
    assert int((ref != 0).sum()) > 10                      # the case has live elements
    got32 = gather_ref(q, s, idx, x, kp_q, m, EXT, influence, aggregation, torch.float32)[0]
    return ref, den, km.cond_err(got32, ref, den)
