"""The attention-map reference of the tests, in one place: the head-averaged softmax weights of
packed-segment multi-head attention on the CPU, in the dtype of its inputs (fp64: the reference;
fp32: the "fp32 restatement" whose error sets the kernel's bound). Not a conftest: imported.

Semantics (include/fgreg.h, fgr_attention_weights; segments as tests/_attn_ref.py): query segment
i (rows q_off[i]..q_off[i+1]) attends key segment kv_seg[i] of n keys; head h owns columns
[h dh, (h + 1) dh):
  w[r, j] = (1 / H) sum_h softmax_j(scale q_h[r] . k_h[j])      j < n
  w[r, j] = 0                                                   n <= j < max_kv_len
which is what nn.MultiheadAttention returns beside its output with need_weights = True
(test_attention_weights_ref.py pins that). A non-empty query segment on an empty key segment is
outside the contract.
"""
import functools
import math
import types

import numpy as np
import torch

from _attn_ref import SEGS, inputs


def head_mean_weights(q, k, qlens, klens, kv_seg, nhead, scale, max_kv_len=None):
    """(sum(qlens), max_kv_len) head-mean softmax weights in the dtype of q; heads are summed in
    ascending order and divided by their number once."""
    dh = q.shape[1] // nhead
    qo, ko = np.cumsum([0] + list(qlens)), np.cumsum([0] + list(klens))
    used = [klens[kv_seg[i]] for i in range(len(qlens)) if qlens[i] > 0]
    max_kv_len = max(used, default=0) if max_kv_len is None else max_kv_len
    w = torch.zeros(q.shape[0], max_kv_len, dtype=q.dtype)
    for i in range(len(qlens)):
        j = kv_seg[i]
        n = klens[j]
        if qlens[i] == 0:
            continue
        acc = torch.zeros(qlens[i], n, dtype=q.dtype)
        for h in range(nhead):
            qs = q[qo[i]:qo[i + 1], h * dh:(h + 1) * dh]
            ks = k[ko[j]:ko[j + 1], h * dh:(h + 1) * dh]
            acc = acc + torch.softmax((qs * scale) @ ks.t(), -1)
        w[qo[i]:qo[i + 1], :n] = acc / nhead
    return w


def valid_mask(qlens, klens, kv_seg, max_kv_len):
    """(rows, max_kv_len) bool: True on the columns j < n of every row."""
    m = torch.zeros(sum(qlens), max_kv_len, dtype=torch.bool)
    qo = np.cumsum([0] + list(qlens))
    for i in range(len(qlens)):
        m[qo[i]:qo[i + 1], :klens[kv_seg[i]]] = True
    return m


@functools.lru_cache(maxsize=None)
def case(regime, seg, nhead, dh):
    """One seeded case of tests/_attn_ref.py (its q and k), computed once and shared read-only:
    .q .k (fp32), .w64 (the fp64 reference), .w32 (the fp32 restatement), .mask (valid columns),
    .qlens .klens .kv_seg .max_q .max_kv .scale."""
    q, k, _, _ = inputs(regime, seg, nhead, dh)
    qlens, klens, kv_seg = SEGS[seg]
    scale = float(np.float32(math.sqrt(1.0 / dh)))       # as the C ABI receives it (a float)
    max_kv = max(klens[kv_seg[i]] for i in range(len(qlens)) if qlens[i] > 0)
    w64 = head_mean_weights(q.double(), k.double(), qlens, klens, kv_seg, nhead, scale, max_kv)
    w32 = head_mean_weights(q, k, qlens, klens, kv_seg, nhead, scale, max_kv)
    return types.SimpleNamespace(q=q, k=k, w64=w64, w32=w32,
                                 mask=valid_mask(qlens, klens, kv_seg, max_kv), qlens=qlens,
                                 klens=klens, kv_seg=kv_seg, max_q=max(qlens), max_kv=max_kv,
                                 scale=scale, nhead=nhead, dh=dh)
