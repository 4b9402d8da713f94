"""The KPConv gather with every influence function and aggregation mode, restated from
finegrained_kpconv_blocks.py:296-381 in any dtype (fp64: the checker; fp32: the yardstick of
the project's error bound), and the test tables of test_gpu_kpconv_modes.py. Not a conftest:
imported by the tests that use it (oracle/model_oracle.py knows linear / sum only).

Tie rule. ``closest`` is a discontinuous function of its inputs: an argmin that flips between
two nearly equidistant kernel points sends a neighbour to another weight matrix. So an entry
of a test table becomes a shadow when, in fp64, the gap between its two smallest d2 is below
TIE * extent^2 -- about a thousand times the fp32 evaluation error of d2 at these magnitudes
(|d| <= 4, 2^-24 * 16 ~ 1e-6 against 2.5e-4). The builder asserts that the rule removes at most
1 % of the valid entries, that together with the linear influence's 2 % boundary rule at most
15 % go, and that on the edited table the fp32 argmin equals the fp64 argmin everywhere.
"""
import functools

import numpy as np
import torch

EXT = 0.5
TIE = 1e-3
INFLUENCES = ('linear', 'gaussian', 'constant')
AGGREGATIONS = ('sum', 'closest')
NEW_COMBOS = [(i, a) for i in INFLUENCES for a in AGGREGATIONS if (i, a) != ('linear', 'sum')]


def sq_distances(q, s, idx, kp):
    """(nq, H, K) squared distances of the centred neighbours to the kernel points; shadow
    entries name the appended far point (:296-316)."""
    sp = torch.cat([s, torch.full((1, 3), 1e6, dtype=s.dtype)])
    nb = sp[idx] - q.unsqueeze(1)
    return ((nb.unsqueeze(2) - kp) ** 2).sum(3)


def influences(d2, extent, influence, aggregation):
    """all_weights (nq, K, H) of :347-372."""
    if influence == 'constant':
        w = torch.ones_like(d2)
    elif influence == 'linear':
        w = torch.clamp(1 - torch.sqrt(d2) / extent, min=0.0)
    elif influence == 'gaussian':
        w = torch.exp(-d2 / (2 * (extent * 0.3) ** 2 + 1e-9))
    else:
        raise ValueError(influence)
    if aggregation == 'closest':
        w = w * torch.nn.functional.one_hot(torch.argmin(d2, dim=2), d2.shape[2]).to(w.dtype)
    elif aggregation != 'sum':
        raise ValueError(aggregation)
    return w.transpose(1, 2)


def gather_ref(q, s, idx, x, kp, extent, influence, aggregation, dtype):
    """(wf (nq, K, cin), sum_h w_h |x_h|) in ``dtype`` on the CPU; differentiable in x."""
    q, s, kp = q.to(dtype), s.to(dtype), kp.to(dtype)
    x = x.to(dtype)
    w = influences(sq_distances(q, s, idx, kp), extent, influence, aggregation)
    nx = torch.cat([x, torch.zeros(1, x.shape[1], dtype=dtype)])[idx]           # (nq, H, cin)
    return torch.matmul(w, nx), torch.matmul(w, nx.abs())


def kpconv_ref(q, s, idx, x, W, kp, extent, influence, aggregation):
    """KPConv.forward (:296-401) in x's dtype: the gather, the weight product, the normaliser."""
    wf, _ = gather_ref(q, s, idx, x, kp, extent, influence, aggregation, x.dtype)
    out = torch.einsum('qkc,kco->qo', wf, W)
    nx = torch.cat([x, torch.zeros(1, x.shape[1], dtype=x.dtype)])[idx]
    cnt = torch.clamp((nx.sum(-1) > 0).sum(-1), min=1)
    return out / cnt.unsqueeze(1).to(x.dtype)


def tie_gap(d2):
    """Gap between the two smallest d2 of every entry, (nq, H)."""
    two = torch.topk(d2, 2, dim=2, largest=False).values
    return two[..., 1] - two[..., 0]


def cond_err(got, ref, den):
    """max_i |got_i - ref_i| / den_i (test_gpu_dispatch._cond_err)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == den.shape, (got.shape, ref.shape, den.shape)
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / den.clamp_min(1e-300)).max())


@functools.lru_cache(maxsize=None)
def table(cin, H, n_kp, nq=70, ns=90):
    """The recipe of test_gpu_dispatch._gather_data restated (70 queries over 90 supports, 60 %
    shadows, query 3 all shadow, every feature row sums to |.| >= 1e-3, entries within 2 % of a
    linear influence boundary become shadows) plus the tie rule of the module docstring.
    -> (q, s, idx, x, kp, cnt): CPU tensors, cnt the exact normaliser."""
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
    q, s, x, kp, idx = (torch.from_numpy(a) for a in (q, s, x, kp, idx))
    d2 = sq_distances(q.double(), s.double(), idx, kp.double())
    valid = idx < ns
    n_valid = int(valid.sum())
    boundary = ((1 - torch.sqrt(d2) / EXT).abs() < 0.02).any(2) & valid
    tie = (tie_gap(d2) < TIE * EXT ** 2) & valid
    share_tie, share_both = int(tie.sum()) / n_valid, int((tie | boundary).sum()) / n_valid
    assert share_tie <= 0.01 and share_both <= 0.15, (cin, H, n_kp, share_tie, share_both)
    idx[boundary | tie] = ns
    assert int((idx < ns).sum()) > nq and bool((idx[3] == ns).all())
    valid = idx < ns
    a64 = torch.argmin(sq_distances(q.double(), s.double(), idx, kp.double()), dim=2)
    a32 = torch.argmin(sq_distances(q, s, idx, kp), dim=2)
    assert bool((a64 == a32)[valid].all()), (cin, H, n_kp)
    nx = torch.cat([x.double(), torch.zeros(1, cin, dtype=torch.float64)])[idx]
    cnt = torch.clamp((nx.sum(-1) > 0).sum(-1), min=1).float()
    return q, s, idx, x, kp, cnt


@functools.lru_cache(maxsize=None)
def reference(cin, H, n_kp, influence, aggregation):
    """-> (wf fp64, den, e32): the fp64 gather of table(cin, H, n_kp), the condition-number
    denominator sum_h w_h |x_h| (for gaussian plus H * 2^-126 * max|x|: a kernel may flush
    subnormal weights to zero, and an element all of whose terms underflow has den ~ 0) and
    the torch fp32 restatement's own error against it."""
    q, s, idx, x, kp, _ = table(cin, H, n_kp)
    ref, den = gather_ref(q, s, idx, x, kp, EXT, influence, aggregation, torch.float64)
    if influence == 'gaussian':
        den = den + H * 2.0 ** -126 * float(x.abs().max())
    assert int((ref != 0).sum()) > 10                      # the case has live elements
    got32 = gather_ref(q, s, idx, x, kp, EXT, influence, aggregation, torch.float32)[0]
    return ref, den, cond_err(got32, ref, den)
