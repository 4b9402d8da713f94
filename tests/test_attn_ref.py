"""Pins tests/_attn_ref.py, the reference of test_gpu_attention_train.py, on the CPU: the
forward against torch's scaled_dot_product_attention, autograd against the closed-form
gradients, lse2 against a direct evaluation, the dropout mask restatement against a scalar
transcription of attn_drop_hash (csrc/common.h), and the conditions each seeded case relies on
(so a change of seed cannot silently void a case)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _attn_ref as ar

F64 = torch.float64


@pytest.mark.parametrize('seg', list(ar.SEGS))
@pytest.mark.parametrize('regime', ar.REGIMES)
def test_forward_matches_sdpa(regime, seg):
    """fp64 mha without dropout = scaled_dot_product_attention per (segment, head); lse2 =
    logsumexp / ln 2 = log2 sum exp2(scale log2(e) q.k) evaluated directly."""
    nhead, dh = 2, 32
    q, k, v, _ = (t.double() for t in ar.inputs(regime, seg, nhead, dh))
    qlens, klens, kv_seg = ar.SEGS[seg]
    scale = math.sqrt(1.0 / dh)
    dens = {}
    o, lse = ar.mha(q, k, v, qlens, klens, kv_seg, nhead, scale, dens=dens, with_lse=True)
    assert torch.equal(o, ar.mha(q, k, v, qlens, klens, kv_seg, nhead, scale))
    qo, ko = np.cumsum([0] + qlens), np.cumsum([0] + klens)
    ref, lref, ldir = torch.zeros_like(o), torch.zeros_like(lse), torch.zeros_like(lse)
    for i, j in enumerate(kv_seg):
        for h in range(nhead):
            c = slice(h * dh, (h + 1) * dh)
            qs, ks, vs = q[qo[i]:qo[i + 1], c], k[ko[j]:ko[j + 1], c], v[ko[j]:ko[j + 1], c]
            if qs.shape[0] == 0:
                continue
            ref[qo[i]:qo[i + 1], c] = F.scaled_dot_product_attention(qs[None], ks[None], vs[None],
                                                                     scale=scale)[0]
            s = scale * (qs @ ks.t())
            lref[qo[i]:qo[i + 1], h] = torch.logsumexp(s, -1) / math.log(2.0)
            s2 = s * math.log2(math.e)
            mx = s2.max(-1, keepdim=True).values
            ldir[qo[i]:qo[i + 1], h] = (mx + torch.log2(torch.exp2(s2 - mx).sum(-1, keepdim=True)))[:, 0]
    assert ar.cond_err(o, ref, dens['o']) <= 1e-13
    assert float((lse - lref).abs().max()) <= 1e-13
    assert float((lse - ldir).abs().max()) <= 1e-12


@pytest.mark.parametrize('drop', [None, ar.DROPS[0], ar.DROPS[1]])
@pytest.mark.parametrize('seg', list(ar.SEGS))
def test_autograd_matches_closed_forms(seg, drop):
    """The reference's autograd gradients = dV = (P o M)^T dO, dS = P o (M o dP - D), dQ = scale
    dS K, dK = scale dS^T Q evaluated directly, with and without the mask."""
    c = ar.case('blocks' if seg != 'separate' else 'unit', seg, 2, 32, drop)
    direct = ar.closed_form(c.q.double(), c.k.double(), c.v.double(), c.R.double(), c.qlens,
                            c.klens, c.kv_seg, 2, c.scale, drop)
    for name, got in zip(('dq', 'dk', 'dv'), direct):
        assert ar.cond_err(got, c.ref[name], c.dens[name]) <= 1e-13, name


def _hash_scalar(seed, head, q, k):
    """attn_drop_hash of csrc/common.h, one tuple at a time in Python integers."""
    m = 0xFFFFFFFF
    x = (seed & m) ^ ((head * 0x9E3779B9) & m)
    x ^= ((q & m) * 0x85EBCA6B) & m
    x = ((x ^ (x >> 16)) * 0x7FEB352D) & m
    x ^= ((k & m) * 0xC2B2AE35) & m
    x = ((x ^ (x >> 15)) * 0x846CA68B) & m
    return x ^ (x >> 16)


def test_mask_restates_the_hash():
    """attn_drop_mask = (attn_drop_hash < p 2^32) on 5 seeds x 3 heads x 6 x 6 rows (seeds 0 and
    0xFFFFFFFF, rows past 2^16) at four p, and the hash is no constant."""
    from fgreg.autograd import attn_drop_mask
    rows = [0, 1, 63, 64, 70000, (1 << 20) + 5]
    keys = [0, 2, 129, 687, 65536 + 3, (1 << 21) + 77]
    seen = set()
    for seed in (0, 0xFFFFFFFF, 987654321, 12345, 1 << 31):
        for head in (0, 1, 7):
            hs = np.array([[_hash_scalar(seed, head, q, k) for k in keys] for q in rows],
                          dtype=np.uint64)
            seen.update(int(x) for x in hs.ravel())
            for p in (0.01, 0.3, 0.5, 0.9):
                pf = ar.p32(p)
                thresh = min(int(pf * 4294967296.0), 4294967295)
                got = attn_drop_mask(seed, pf, head, rows, keys)
                assert np.array_equal(np.asarray(got, bool), hs < thresh), (seed, head, p)
    assert len(seen) == 5 * 3 * 36


UNIT = [c for c in ar.all_cases() if c[0] == 'unit']


@pytest.mark.parametrize('case', UNIT, ids=lambda c: '-'.join(str(x) for x in c[1:4]) + ('-p0' if c[4] is None else f'-{c[4][0]}-{c[4][1]}'))
def test_unit_restatement_error(case):
    """In every unit case the fp32 restatement's per-element error is at most 1e-6 for o, dq,
    dk and dv, so 4 x it stays under the attention family's cap of 1e-5."""
    c = ar.case(*case)
    for name in ar.NAMES:
        assert 0 < c.e32[name] <= 1e-6, (name, c.e32[name])


@pytest.mark.parametrize('dh', [32, 64])
def test_all_dropped_rows(dh):
    """'self' at nhead 2: row 130 (the one-row segment) has one key, itself. (987654321, 0.3)
    drops it in exactly one head, (0, 0.9) and (0xFFFFFFFF, 0.9) in both; there o, dq, dk and
    dv of row 130 are exactly 0 with denominator 0."""
    from fgreg.autograd import attn_drop_mask
    assert ar.SEGS['self'][0][:3] == [130, 0, 1]
    for drop, want in zip(ar.DROPS[:3], (1, 2, 2)):
        dropped = [bool(attn_drop_mask(drop[0], ar.p32(drop[1]), h, [130], [130])[0, 0])
                   for h in range(2)]
        assert sum(dropped) == want, (drop, dropped)
        c = ar.case('unit', 'self', 2, dh, drop)
        for h in range(2):
            cols = slice(h * dh, (h + 1) * dh)
            for name in ar.NAMES:
                ref, den = c.ref[name][130, cols], c.dens[name][130, cols]
                if dropped[h]:
                    assert bool((ref == 0).all()) and bool((den == 0).all()), (drop, h, name)
                else:
                    assert bool((den > 0).all()), (drop, h, name)
    # no other element of these cases has a zero denominator
    c = ar.case('unit', 'self', 2, dh, ar.DROPS[1])
    for name in ar.NAMES:
        z = c.dens[name] == 0
        assert int(z.sum()) == 2 * dh and bool(z[130].all()), name


@pytest.mark.parametrize('drop', [None, ar.DROPS[0]])
@pytest.mark.parametrize('regime', ar.REGIMES)
def test_unattended_key_rows(regime, drop):
    """'mixed': the 129 rows of key segments 2 and 6 are attended by nobody; dk = dv = 0 exactly
    there, with denominator 0, and nowhere else."""
    qlens, klens, kv_seg = ar.SEGS['mixed']
    ko = np.cumsum([0] + klens)
    free = [j for j in range(len(klens)) if j not in kv_seg and klens[j] > 0]
    rows = np.concatenate([np.arange(ko[j], ko[j + 1]) for j in free])
    assert free == [2, 6] and len(rows) == 129
    c = ar.case(regime, 'mixed', 2, 32, drop)
    mask = torch.zeros(sum(klens), dtype=torch.bool)
    mask[torch.from_numpy(rows)] = True
    for name in ('dk', 'dv'):
        assert bool((c.ref[name][mask] == 0).all()) and bool((c.dens[name][mask] == 0).all())
        assert bool((c.dens[name][~mask] > 0).all())


def test_segmentations_are_inside_the_contract():
    """No non-empty query segment attends an empty key segment; at most 688 rows per case."""
    for name, (qlens, klens, kv_seg) in ar.SEGS.items():
        assert len(kv_seg) == len(qlens) and max(sum(qlens), sum(klens)) <= 688
        for i, j in enumerate(kv_seg):
            assert qlens[i] == 0 or klens[j] > 0, (name, i)
    assert sum(ar.SEGS['separate'][1]) == 330 and sum(ar.SEGS['separate'][0]) == 260
