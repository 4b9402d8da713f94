"""The conv1 weight image of fgr_res2net_block_h3 (fgreg.ops.res2net_conv1_fragments) against
its written definition: [jt = j * KT + tile][ks][term][g][c][e] holds the two fp16 terms of
W1[j * w + 16 tile + c][32 ks + 8 g + e] * 2^e_row, chunks zero-padded to whole tiles."""
import math

import torch


def test_conv1_fragments_definition():
    from fgreg import ops
    scale, w, cin = 3, 28, 64                     # KT = 2: 4 padded rows per chunk
    g = torch.Generator().manual_seed(11)
    W1 = torch.randn(scale * w, cin, generator=g) * torch.logspace(-3, 3, scale * w)[:, None]
    W1[37] = 0                                    # an all-zero output row
    img, inv = ops.res2net_conv1_fragments(W1, scale)
    kt, ks = 2, cin // 32
    assert img.shape == (scale * kt, ks, 2, 4, 16, 8) and img.dtype == torch.float16
    assert inv.shape == (scale * w,) and inv.dtype == torch.float32
    # scales: powers of two putting the row max into [2^14, 2^15); 1 for the zero row
    mx = W1.abs().amax(1)
    sc = 1.0 / inv
    assert float(inv[37]) == 1.0 and bool((img[37 // w * kt + (37 % w) // 16, :, :, :, 37 % w % 16] == 0).all())
    live = mx > 0
    assert bool((torch.frexp(sc)[0] == 0.5).all())
    top = mx[live] * sc[live]
    assert bool((top >= 2.0 ** 14).all()) and bool((top < 2.0 ** 15).all())
    # the value at a given [jt][ks][term][g][c][e]
    for (j, tile, s, gg, c, e) in [(0, 0, 0, 0, 0, 0), (1, 1, 1, 3, 11, 7), (2, 0, 1, 2, 15, 4),
                                   (2, 1, 0, 1, 5, 3)]:
        row, k = j * w + 16 * tile + c, 32 * s + 8 * gg + e
        v = float(W1[row, k]) * float(sc[row])
        hi = torch.tensor(v).to(torch.float16)
        lo = torch.tensor(v - float(hi)).to(torch.float16)
        assert float(img[j * kt + tile, s, 0, gg, c, e]) == float(hi)
        assert float(img[j * kt + tile, s, 1, gg, c, e]) == float(lo)
    # padding rows (16 tile + c >= w) are zero
    assert bool((img.reshape(scale, kt, ks, 2, 4, 16, 8)[:, 1, :, :, :, w - 16:] == 0).all())
    # the terms sum to the scaled weight within fp16's residual: |x - hi - lo| <= 2^-22 |x|
    # (two 11-bit significands), or half the fp16 subnormal spacing 2^-25 where lo is subnormal
    t = img.reshape(scale, kt, ks, 2, 4, 16, 8).permute(3, 0, 1, 5, 2, 4, 6).reshape(
        2, scale, kt * 16, cin)[:, :, :w].reshape(2, scale * w, cin).double()
    want = W1.double() * sc.double()[:, None]
    res = (want - t[0] - t[1]).abs()
    assert bool((res <= want.abs() * 2.0 ** -22 + 2.0 ** -25).all())
    # scale = 1 gives the same image when w is a multiple of 16
    W2 = torch.randn(2 * 32, 32, generator=g) / math.sqrt(32)
    a, b = ops.res2net_conv1_fragments(W2, 2), ops.res2net_conv1_fragments(W2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
