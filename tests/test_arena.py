"""CPU self-test of tests/_arena.py: stand-in "kernels" written with torch ops on CPU tensors
show that the arena reports each class of footprint bug it exists for (with the offending role
and offset) and passes a correct kernel. The GPU footprint tests (test_gpu_footprint.py) rely
on exactly these checks."""
import pytest
import torch

from _arena import GUARD, SENTINEL, Arena, ArenaError, assert_both_equal, bit_equal, run_both

M, N, K = 5, 6, 7
LDA, LDC = K + 4, N + 4


def _operands(arena):
    g = torch.Generator().manual_seed(3)
    a = arena.put(torch.randn(M, K, generator=g), ld=LDA, name='a')
    w = arena.put(torch.randn(N, K, generator=g), name='w')
    c = arena.matrix(M, N, LDC, torch.float32, 'out', name='c')
    ws = arena.bytes(4 * M * N, name='ws')
    return a, w, c, ws


def _flat(view, n):
    """n elements of the storage starting at view[0, 0] (what a raw pointer + ld addresses)."""
    return torch.as_strided(view, (n,), (1,))


def good(arena):
    a, w, c, ws = _operands(arena)
    part = ws.view(torch.float32).view(M, N)         # writes the scratch before reading it
    torch.mm(a, w.t(), out=part)
    c.copy_(part)
    return c


def writes_column_n(arena):
    c = good(arena)
    _flat(c, 2 * LDC)[LDC + N] = 1.0                   # row 1, column N: a pad column
    return c


def writes_row_m(arena):
    c = good(arena)
    _flat(c, M * LDC + 1)[M * LDC] = 1.0               # row M, column 0
    return c


def writes_past_workspace(arena):
    a, w, c, ws = _operands(arena)
    torch.as_strided(ws, (ws.numel() + 4,), (1,))[ws.numel():] = 7      # 4 bytes past `need`
    c.copy_(a @ w.t())
    return c


def sums_k_plus_1(arena):
    a, w, c, ws = _operands(arena)
    a1 = torch.as_strided(a, (M, K + 1), (LDA, 1))     # reads pad column K of every row
    w1 = torch.cat([w, torch.zeros(N, 1)], 1)          # ... times the weight's zero K-padding
    c.copy_(a1 @ w1.t())
    return c


def reads_stale_scratch(arena):
    a, w, c, ws = _operands(arena)
    c.copy_(a @ w.t() + ws.view(torch.float32).view(M, N))      # accumulates into stale scratch
    return c


def leaves_row_unwritten(arena):
    a, w, c, ws = _operands(arena)
    c[:M - 1].copy_((a @ w.t())[:M - 1])
    return c


def test_correct_kernel_passes():
    clean, poisoned = run_both(good, 'cpu')
    assert_both_equal(clean, poisoned)
    g = torch.Generator().manual_seed(3)
    a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    assert torch.allclose(clean, a @ w.t(), atol=1e-6)


@pytest.mark.parametrize('kernel,role,where', [
    (writes_column_n, "role 'out' operand 'c'", f'byte offset {4 * (LDC + N)} (row 1, column {N}'),
    (writes_row_m, "role 'out' operand 'c'", f'byte offset {4 * M * LDC} ({4 * (LDC - N)} past'),
    (writes_past_workspace, "role 'scratch' operand 'ws'", f'byte offset {4 * M * N} (0 past'),
    (leaves_row_unwritten, "role 'out' operand 'c'",
     f'(row {M - 1}, column 0) at byte offset {4 * (M - 1) * LDC} was never written'),
])
def test_footprint_bug_is_reported(kernel, role, where):
    with pytest.raises(ArenaError) as e:
        run_both(kernel, 'cpu')
    assert role in str(e.value) and where in str(e.value), str(e.value)


@pytest.mark.parametrize('kernel', [sums_k_plus_1, reads_stale_scratch])
def test_dependence_on_pad_or_scratch_is_reported(kernel):
    """NaN * 0 in the pad column / 0xFF scratch: the poisoned run differs from the clean one.
    The clean run alone is right (zero pads, zero scratch), which is how such a kernel passes a
    value-only test."""
    clean, poisoned = run_both(kernel, 'cpu')
    g = torch.Generator().manual_seed(3)
    a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    assert torch.allclose(clean, a @ w.t(), atol=1e-6)
    with pytest.raises(ArenaError, match='depends on pad / guard / scratch'):
        assert_both_equal(clean, poisoned)


def test_layout_and_fills():
    for poison in (False, True):
        ar = Arena('cpu', poison)
        x = ar.matrix(3, 5, 9, torch.float32, 'in', misalign=4)
        assert x.data_ptr() % 16 == 4 and x.stride() == (9, 1)
        pad = torch.as_strided(x, (2, 4), (9, 1), x.storage_offset() + 5)
        assert bool(torch.isnan(pad).all()) == poison and (poison or bool((pad == 0).all()))
        idx = ar.matrix(4, 3, 8, torch.int64, 'in')
        ipad = torch.as_strided(idx, (3, 5), (8, 1), idx.storage_offset() + 3)
        assert bool((ipad > (1 << 40)).all()) == poison
        o = ar.matrix(2, 3, 7, torch.float32, 'out')
        assert bool((o.view(torch.int32) == SENTINEL).all()) and bool(torch.isnan(o).all())
        ws = ar.bytes(37)
        assert ws.numel() == 37 and ws.data_ptr() % 16 == 0
        assert bool((ws == (0xFF if poison else 0)).all())
        # the first byte past an exact-size payload is guard, and 64 KiB of it
        tail = torch.as_strided(ws, (GUARD,), (1,), ws.storage_offset() + 37)
        assert tail.numel() == GUARD
        with pytest.raises(ArenaError, match='never written'):
            ar.check()
        o.fill_(1.0)
        ar.check()
        tail[GUARD - 1] ^= 0xFF                      # the last guard byte is watched too
        with pytest.raises(ArenaError, match="role 'scratch'"):
            ar.check()


def test_bit_equal_treats_nan_bits():
    a = torch.tensor([float('nan'), 1.0])
    assert bit_equal(a, a.clone()) and not torch.equal(a, a.clone())
    assert not bit_equal(a, torch.tensor([float('nan'), 2.0]))
    assert bit_equal(torch.tensor(1.5), torch.tensor(1.5)) and not bit_equal(torch.tensor(1.5), torch.tensor(2.5))
