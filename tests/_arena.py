"""Guarded operand arena for tests that pin WHERE a kernel reads and writes.

Every operand handed to libfgreg is carved out of one uint8 allocation of its own, laid out
as ``[head guard | payload | tail guard]`` with 64 KiB guards, so an overreach of up to 64 KiB
on either side stays inside a live allocation (it is caught, it cannot fault). The payload is
exactly what the C ABI's contract says the operand spans -- ``(rows - 1) * ld + cols`` elements
for a strided matrix, ``n`` bytes for a workspace or an image -- so the first byte past it is
already guard.

Roles
  'out'      guards, the pad columns [cols, ld) of every row and the payload itself hold a
             32-bit sentinel (a quiet NaN with a recognisable payload). check() asserts every
             sentinel byte outside [0, rows) x [0, cols) is unchanged and, for outputs the
             kernel must define fully (``full=True``, the default), that no element inside is
             still the sentinel.
  'in'       guards and pad columns hold 0 (clean) or a poison (poisoned arena): quiet NaN for
             floating types, an out-of-range index for integer tables. Live entries are
             whatever the test copies in; the poison never touches them.
  'scratch'  the payload is prefilled with 0x00 (clean) or 0xFF bytes (poisoned: NaN in fp32,
             fp16 and bf16, -1 in every integer type); the guards hold the sentinel.

run_both(fn, device) runs ``fn(arena)`` once on a clean and once on a poisoned arena, checks
both arenas, and returns the two outputs; the test compares them bit for bit (bit_equal): a
kernel whose result depends on pad columns, rows past the end, stale scratch or (being two
launches) on a race differs. Not a conftest: imported by the tests that use it.
"""
import torch

SENTINEL = 0x7FC5A5A5                      # quiet NaN, payload 0x45A5A5
GUARD = 64 << 10
BAD_INDEX = (1 << 62) + 12345              # far outside any table an index could address
_SENT_BYTES = [(SENTINEL >> (8 * i)) & 0xFF for i in range(4)]      # little endian


class ArenaError(AssertionError):
    pass


class _Region:
    __slots__ = ('name', 'role', 'buf', 'start', 'nbytes', 'rows', 'cols', 'ld', 'itemsize',
                 'full', 'view')


class Arena:
    def __init__(self, device, poison=False):
        self.device = torch.device(device)
        self.poison = bool(poison)
        self.regions = []

    # ---- carving ---------------------------------------------------------------------------
    def _carve(self, nbytes, misalign):
        """One allocation; the payload starts ``misalign`` bytes past a 16-B boundary."""
        assert misalign % 4 == 0 and 0 <= misalign < 16
        total = GUARD + 16 + (nbytes + 15) // 16 * 16 + GUARD
        buf = torch.empty(total, dtype=torch.uint8, device=self.device)
        assert buf.data_ptr() % 16 == 0, 'allocator returned a block that is not 16-B aligned'
        return buf, GUARD + misalign

    def _fill_sentinel(self, buf):
        buf.view(torch.int32).fill_(SENTINEL)

    def matrix(self, rows, cols, ld, dtype, role, name=None, misalign=0, full=True):
        """The (rows, cols) view with row stride ld (elements) of a fresh region."""
        assert rows >= 1 and 1 <= cols <= ld and role in ('in', 'out')
        itemsize = torch.empty((), dtype=dtype).element_size()
        assert itemsize % 4 == 0 or role == 'in', 'out regions are checked in 32-bit words'
        assert misalign % itemsize == 0
        n_el = (rows - 1) * ld + cols
        buf, start = self._carve(n_el * itemsize, misalign)
        if role == 'out':
            self._fill_sentinel(buf)
        else:
            typed = buf.view(dtype)
            if not self.poison:
                typed.zero_()
            elif dtype.is_floating_point:
                typed.fill_(float('nan'))
            else:
                typed.fill_(min(BAD_INDEX, torch.iinfo(dtype).max))
        flat = buf[start:start + n_el * itemsize].view(dtype)
        view = torch.as_strided(flat, (rows, cols), (ld, 1))
        r = _Region()
        r.name, r.role, r.buf, r.start, r.nbytes = name or f'op{len(self.regions)}', role, buf, start, n_el * itemsize
        r.rows, r.cols, r.ld, r.itemsize, r.full, r.view = rows, cols, ld, itemsize, full, view
        self.regions.append(r)
        return view

    def vector(self, n, dtype, role, name=None, misalign=0, full=True):
        return self.matrix(1, n, n, dtype, role, name, misalign, full)[0]

    def put(self, t, ld=None, name=None, misalign=0):
        """An 'in' region holding the 1-D / 2-D tensor t (row stride ld, default dense)."""
        t2 = t.reshape(1, -1) if t.dim() == 1 else t
        assert t2.dim() == 2
        v = self.matrix(t2.shape[0], t2.shape[1], ld or t2.shape[1], t.dtype, 'in', name, misalign)
        v.copy_(t2)
        return v[0] if t.dim() == 1 else v

    def bytes(self, n, role='scratch', name=None):
        """An exact n-byte uint8 view, 16-B aligned (workspaces, weight and K/V images)."""
        assert n >= 1 and role == 'scratch'
        buf, start = self._carve(n, 0)
        self._fill_sentinel(buf)
        view = buf[start:start + n]
        view.fill_(0xFF if self.poison else 0x00)
        r = _Region()
        r.name, r.role, r.buf, r.start, r.nbytes = name or f'ws{len(self.regions)}', 'scratch', buf, start, n
        r.rows, r.cols, r.ld, r.itemsize, r.full, r.view = 1, n, n, 1, False, view
        self.regions.append(r)
        return view

    # ---- checking --------------------------------------------------------------------------
    def _where(self, r, byte):
        """Human-readable position of absolute buffer byte ``byte`` of region r."""
        off = byte - r.start
        if off < 0:
            return f'byte offset {off} (head guard)'
        if off >= r.nbytes:
            return f'byte offset {off} ({off - r.nbytes} past the {r.nbytes}-byte payload, tail guard)'
        row, col = divmod(off // r.itemsize, r.ld)
        return f'byte offset {off} (row {row}, column {col} of a ({r.rows}, {r.cols}) ld {r.ld} operand)'

    def check(self):
        """Raises ArenaError naming the role, region and offset of the first violation."""
        for r in self.regions:
            if r.role == 'in':
                continue
            buf = r.buf
            expected = torch.tensor(_SENT_BYTES, dtype=torch.uint8,
                                    device=buf.device).repeat(buf.numel() // 4)
            same = buf == expected
            live = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
            lv = torch.as_strided(live[r.start:], (r.rows, r.cols * r.itemsize),
                                  (r.ld * r.itemsize, 1))
            lv.fill_(True)
            bad = (~same) & (~live)
            if bool(bad.any()):
                first = int(torch.nonzero(bad)[0])
                raise ArenaError(f"role '{r.role}' operand '{r.name}': written outside its extent "
                                 f"at {self._where(r, first)}; {int(bad.sum())} bytes in all")
            if r.role == 'out' and r.full:
                sv = torch.as_strided(same[r.start:], (r.rows, r.cols, r.itemsize),
                                      (r.ld * r.itemsize, r.itemsize, 1))
                unset = sv.all(-1)
                if bool(unset.any()):
                    row, col = (int(v) for v in torch.nonzero(unset)[0])
                    raise ArenaError(f"role 'out' operand '{r.name}': element (row {row}, column "
                                     f"{col}) at byte offset {(row * r.ld + col) * r.itemsize} was "
                                     f"never written; {int(unset.sum())} elements in all")


def bit_equal(a, b):
    """Bitwise equality of two tensors (NaNs with equal bits are equal)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


def run_both(fn, device):
    """fn(arena) -> a tensor or a tuple of tensors (views into the arena are fine). Runs it on a
    clean and on a poisoned arena, checks each arena's guards after a device sync, and returns
    (clean outputs, poisoned outputs) as detached copies."""
    outs = []
    for poison in (False, True):
        arena = Arena(device, poison)
        out = fn(arena)
        if arena.device.type == 'cuda':
            torch.cuda.synchronize(arena.device)
        arena.check()
        single = torch.is_tensor(out)
        got = tuple(t.clone() for t in ((out,) if single else out))
        outs.append(got[0] if single else got)
    return outs[0], outs[1]


def assert_both_equal(clean, poisoned):
    """The bit-for-bit comparison of run_both's two results."""
    cs, ps = ((clean,), (poisoned,)) if torch.is_tensor(clean) else (clean, poisoned)
    for i, (c, p) in enumerate(zip(cs, ps)):
        if not bit_equal(c, p):
            diff = (c.contiguous().reshape(-1).view(torch.uint8) != p.contiguous().reshape(-1).view(torch.uint8))
            raise ArenaError(f'output {i} depends on pad / guard / scratch contents: '
                             f'{int(diff.sum())} bytes differ between the clean and the poisoned '
                             f'run (first at flat byte {int(torch.nonzero(diff.flatten())[0])})')
