"""Guard bands for the kernel contract tests (tests/test_05_kernel_contract_gpu.py).

A kernel test that allocates every buffer exactly as large as its logical shape cannot see a store one row past M, a vector store past
roundup8(N) or a read of the `ld` padding: all of that lands in the allocator's slack.  `guarded()` carves the logical [rows, cols] view
(row stride ld >= cols) out of ONE larger allocation with whole guard rows before and after it, so that an overrun stays inside the same
allocation -- never a memory fault -- and turns into a failed assertion:

    input flavour   fill="nan": guards and the [cols, ld) padding of every row are NaN; a kernel that reads them poisons its result.
                    fill=<int>:  index tensors (ids, positions, row maps): the guards hold a VALID index, chosen by the caller to point at
                                 a NaN row of the table it indexes, so a stray read shows up as a NaN and not as a wild access.
    output flavour  fill="sentinel": every byte holds a sentinel bit pattern (a NaN for the floating types).

`assert_untouched(g, written=...)` compares everything outside the declared write footprint with the snapshot taken by `seal()`, on the BIT
pattern (NaN != NaN), and names the first offending (row, col) relative to the logical tensor (negative rows / cols >= `cols` are guards and
padding).  The guards are deeper than the largest tile of the library (256 rows, 256 columns): GUARD_ROWS rows on both sides, an odd number
so that a tile-aligned overrun cannot hide; the base of the view stays 16-byte aligned as the ABI requires.
"""
import torch

GUARD_ROWS = 257          # > the largest tile (256 x 256) of the library, odd
_SENTINEL = {1: 0x5A, 2: 0x7DA5, 4: 0x7FA5A5A5, 8: 0x7FF5A5A5A5A5A5A5}      # NaN patterns for fp16 / fp32 / fp64, large values for integers
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def roundup8(n):
    return (n + 7) // 8 * 8


def bits(t):
    """Integer view of a tensor's bit patterns (same shape)."""
    return t if t.dtype in (torch.uint8, torch.int16, torch.int32, torch.int64) else t.view(_INT_VIEW[t.element_size()])


class Guarded(object):
    """view: the logical [rows, cols] tensor (row stride ld); full: [rows, ld] (logical columns + padding); buf2d: the whole allocation as
    [g0 + rows + g1, ld] with the logical row 0 at index g0.  1-D tensors are the rows = 1 case with `vec` as their [cols] view."""

    def __init__(self, rows, cols, ld, dtype, fill, guard_rows, device):
        assert rows >= 1 and cols >= 1 and ld >= cols
        es = torch.empty((), dtype=dtype).element_size()
        g0 = guard_rows
        while (g0 * ld * es) % 16:            # keep the view's base 16-byte aligned by growing the guard, never by shifting the base
            g0 += 1
        self.rows, self.cols, self.ld, self.dtype, self.g0, self.g1 = rows, cols, ld, dtype, g0, guard_rows
        self.buf = torch.empty((g0 + rows + guard_rows) * ld, dtype=dtype, device=device)
        self.fill_all(fill)
        self.buf2d = self.buf.view(-1, ld)
        self.full = self.buf2d[g0:g0 + rows]
        self.view = self.full[:, :cols]
        self.vec = self.view[0]
        assert self.view.data_ptr() % 16 == 0
        self._snap = None
        self.seal()

    def fill_all(self, fill):
        if isinstance(fill, str) and fill == "sentinel":
            bits(self.buf).fill_(_signed(_SENTINEL[self.buf.element_size()], self.buf.element_size()))
        elif isinstance(fill, str) and fill == "nan":
            assert self.buf.is_floating_point()
            self.buf.fill_(float("nan"))
        else:
            self.buf.fill_(fill)

    def set(self, t):
        """Copy `t` ([rows, cols], or [cols] for a vector) into the logical region and take the snapshot again."""
        self.view.copy_(t.reshape(self.rows, self.cols))
        return self.seal()

    def seal(self):
        """Snapshot the bit patterns: what assert_untouched compares against.  Call again after writing through .view / .full by hand."""
        self._snap = bits(self.buf).clone()
        return self


def _signed(v, nbytes):
    """The Python int whose two's-complement pattern in `nbytes` bytes is v (torch integer dtypes are signed, uint8 apart)."""
    return v if nbytes == 1 or v < (1 << (8 * nbytes - 1)) else v - (1 << (8 * nbytes))


def guarded(rows, cols, ld=None, dtype=torch.float16, fill="nan", guard_rows=GUARD_ROWS, device="cpu"):
    return Guarded(rows, cols, cols if ld is None else ld, dtype, fill, guard_rows, device)


def guarded_vec(n, dtype=torch.float32, fill="nan", guard=None, device="cpu"):
    """1-D form (bias, mean, rstd, lse, delta, dgamma, loss scalars, ids): `n` elements between two guards of `guard` elements each; the
    default guard is an odd number (513) of 16-byte units, so the base stays aligned and the guard is odd-sized.  Use `.vec`."""
    es = torch.empty((), dtype=dtype).element_size()
    unit = max(1, 16 // es)
    if guard is None:
        guard = 513 * unit
    assert guard % unit == 0 and guard >= 256
    g = Guarded.__new__(Guarded)
    g.rows, g.cols, g.ld, g.dtype, g.g0, g.g1 = 1, n, n, dtype, guard, guard
    g.buf = torch.empty(guard + n + guard, dtype=dtype, device=device)
    g.fill_all(fill)
    g.buf2d = None
    g.full = g.view = g.buf[guard:guard + n].view(1, n)
    g.vec = g.view[0]
    assert g.vec.data_ptr() % 16 == 0
    g._snap = None
    return g.seal()


def _where(g, flat):
    """(row, col) of flat element index `flat` of g.buf relative to the logical tensor."""
    if g.buf2d is None:
        return 0, flat - g.g0
    return flat // g.ld - g.g0, flat % g.ld


def footprint(g, written):
    """Boolean mask over g.buf of the elements a kernel may write.  written: None (nothing: an input), "logical" ([rows, cols]), "rows"
    (whole rows [rows, ld]), an int c (columns [0, c) of every row), or a bool tensor [rows, ld] / [rows, cols] / [cols]."""
    m = torch.zeros(g.buf.numel(), dtype=torch.bool, device=g.buf.device)
    if written is None:
        return m
    if g.buf2d is None:
        lo = m[g.g0:g.g0 + g.cols]
        if isinstance(written, str):
            assert written in ("logical", "rows")
            lo.fill_(True)
        elif isinstance(written, int):
            lo[:written] = True
        else:
            lo.copy_(written.reshape(-1))
        return m
    m2 = m.view(-1, g.ld)[g.g0:g.g0 + g.rows]
    if isinstance(written, str):
        assert written in ("logical", "rows")
        m2[:, :g.cols if written == "logical" else g.ld] = True
    elif isinstance(written, int):
        assert 0 <= written <= g.ld
        m2[:, :written] = True
    else:
        m2[:, :written.shape[-1]] = written.reshape(g.rows, -1)
    return m


def assert_untouched(g, written=None, name="buffer"):
    """Every element outside the declared write footprint still has the bit pattern it had at seal()."""
    bad = (bits(g.buf) != g._snap) & ~footprint(g, written)
    if bool(bad.any()):
        flat = int(torch.nonzero(bad)[0])
        r, c = _where(g, flat)
        raise AssertionError("%s: element (row %d, col %d) outside the write footprint was modified (%d elements in all; logical shape %d x %d, ld %d): "
                             "0x%x -> 0x%x" % (name, r, c, int(bad.sum()), g.rows, g.cols, g.ld,
                                               int(g._snap[flat]) & ((1 << (8 * g.buf.element_size())) - 1),
                                               int(bits(g.buf)[flat]) & ((1 << (8 * g.buf.element_size())) - 1)))


def assert_written(g, written="logical", name="buffer"):
    """Output flavour: no element of the footprint still holds the sentinel (the kernel left part of what it owes unwritten)."""
    es = g.buf.element_size()
    left = (bits(g.buf) == _signed(_SENTINEL[es], es)) & footprint(g, written)
    if bool(left.any()):
        flat = int(torch.nonzero(left)[0])
        r, c = _where(g, flat)
        raise AssertionError("%s: element (row %d, col %d) of the write footprint was never written (%d elements in all)" % (name, r, c, int(left.sum())))


def assert_zero_band(g, c0, c1, name="buffer"):
    """Columns [c0, c1) of every logical row hold exactly +0 (bit pattern 0)."""
    if c1 <= c0:
        return
    band = bits(g.full[:, c0:c1])
    if bool((band != 0).any()):
        r, c = [int(v) for v in torch.nonzero(band != 0)[0]]
        raise AssertionError("%s: zero band [%d, %d): element (row %d, col %d) holds 0x%x, not 0" % (name, c0, c1, r, c0 + c,
                                                                                                   int(band[r, c]) & ((1 << (8 * band.element_size())) - 1)))


def assert_finite(t, name="result"):
    """No NaN / Inf: with every byte a kernel has no business reading set to NaN, a non-finite result is a stray read."""
    t = t.float() if t.is_floating_point() else t
    ok = torch.isfinite(t)
    if not bool(ok.all()):
        idx = [int(v) for v in torch.nonzero(~ok)[0]]
        raise AssertionError("%s: non-finite value at %s (%d in all): a poisoned guard / padding element was read" % (name, idx, int((~ok).sum())))
