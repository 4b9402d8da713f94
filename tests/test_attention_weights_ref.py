"""CPU: tests/_attn_weights_ref.py (the reference of the attention-map tests) pinned against
torch.nn.MultiheadAttention itself, and fgr_attention_weights' argument errors, which need no
GPU (a refused call launches nothing)."""
import ctypes
import math

import pytest
import torch

from _attn_weights_ref import head_mean_weights, valid_mask


@pytest.mark.parametrize('nhead,dh', [(8, 4), (2, 32)])
def test_reference_equals_multihead_attention(nhead, dh):
    """A padded B = 2 batch through nn.MultiheadAttention (key_padding_mask, need_weights = True,
    the reference's call) in fp64: the packed reference equals the returned weights on every
    pair's valid block within 1e-12, and MHA's padded key columns are exactly 0."""
    d = nhead * dh
    g = torch.Generator().manual_seed(1234 + dh)
    qlens, klens = [37, 50], [41, 29]                 # pair b: qlens[b] queries on klens[b] keys
    Lq, Lk = max(qlens), max(klens)
    mha = torch.nn.MultiheadAttention(d, nhead).double()
    with torch.no_grad():
        for p in mha.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.3)
    xq = torch.randn(Lq, 2, d, generator=g, dtype=torch.float64)
    xk = torch.randn(Lk, 2, d, generator=g, dtype=torch.float64)
    pad = torch.ones(2, Lk, dtype=torch.bool)
    for b in range(2):
        pad[b, :klens[b]] = False
    with torch.no_grad():
        _, w = mha(xq, xk, xk, key_padding_mask=pad)                    # (B, Lq, Lk)
        W, bias = mha.in_proj_weight, mha.in_proj_bias
        q = torch.cat([xq[:qlens[b], b] @ W[:d].t() + bias[:d] for b in range(2)])
        k = torch.cat([xk[:klens[b], b] @ W[d:2 * d].t() + bias[d:2 * d] for b in range(2)])
    assert w.shape == (2, Lq, Lk)
    ref = head_mean_weights(q, k, qlens, klens, [0, 1], nhead, math.sqrt(1.0 / dh), Lk)
    assert ref.dtype == torch.float64 and ref.shape == (sum(qlens), Lk)
    row = 0
    for b in range(2):
        blk = ref[row:row + qlens[b]]
        assert float((blk[:, :klens[b]] - w[b, :qlens[b], :klens[b]]).abs().max()) <= 1e-12
        assert bool((w[b, :, klens[b]:] == 0).all())        # MHA's padded key columns
        assert bool((blk[:, klens[b]:] == 0).all())
        assert float((blk.sum(-1) - 1).abs().max()) <= 1e-12
        row += qlens[b]
    mask = valid_mask(qlens, klens, [0, 1], Lk)
    assert bool((ref[~mask] == 0).all()) and int(mask.sum()) == 37 * 41 + 50 * 29


def test_reference_shared_and_empty_segments():
    """kv_seg may share a key segment between query segments; an empty query segment
    contributes no rows; max_kv_len pads with zeros."""
    g = torch.Generator().manual_seed(7)
    qlens, klens, kv_seg = [3, 0, 2], [4, 0, 1], [0, 1, 0]
    q = torch.randn(5, 8, generator=g, dtype=torch.float64)
    k = torch.randn(5, 8, generator=g, dtype=torch.float64)
    w = head_mean_weights(q, k, qlens, klens, kv_seg, 2, 0.5, 6)
    assert w.shape == (5, 6) and bool((w[:, 4:] == 0).all())
    assert float((w.sum(-1) - 1).abs().max()) < 1e-14
    one = head_mean_weights(q[:2], k[:1], [2], [1], [0], 2, 0.5)
    assert bool((one == 1).all())                            # a one-key row


def _call(L, head_dim, ld_w, max_kv=8, n_head=2):
    fake = ctypes.c_void_p(64)          # never dereferenced: the call is refused before a launch
    return L.fgr_attention_weights(fake, n_head * max(head_dim, 1), fake, n_head * max(head_dim, 1),
                                   fake, ld_w, fake, fake, fake, 1, 8, max_kv, n_head, head_dim,
                                   ctypes.c_float(0.5), None)


def test_argument_errors_need_no_gpu():
    """Unsupported head_dim and ld_w < max_kv_len are FGR_E_ARG with a message."""
    import fgreg
    L = fgreg.load()
    for hd in (0, 6, 30, 260, 512):
        assert _call(L, hd, 8) == -1
        assert f'head_dim {hd} unsupported'.encode() in L.fgr_last_error()
    assert _call(L, 32, 7) == -1
    assert b'ld_w 7 < max_kv_len 8' in L.fgr_last_error()
    assert _call(L, 64, 8, n_head=200) == -1 and b'LDS' in L.fgr_last_error()
    rc = L.fgr_attention_weights(None, 0, None, 0, None, 0, None, None, None, 1, 1, 1, 1, 32,
                                 ctypes.c_float(1.0), None)
    assert rc == -1 and b'fgr_attention_weights' in L.fgr_last_error()
    assert _call(L, 32, 8, max_kv=0) == 0                    # nothing to write: no launch
