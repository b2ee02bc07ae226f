"""Guard bands for the C-ABI tests: a strided [rows, width] operand inside ONE flat allocation whose every other element holds
a fixed bit pattern.

    [ guard_rows * ld + lead elements | rows x ld (payload = the first `width` of each row) | guard_rows * ld elements ]

The pattern is a quiet NaN with a payload when read as fp32 (0x7FC0BEEF), a NaN when read as bf16 or fp16 (0x7FC1) and 0x5A
for bytes.  A kernel may LOAD the padding columns width .. ld and the rows before / after its operand; it must not let them
reach a result (a NaN would show) and must not STORE there (assert_untouched shows the first changed element).  256 guard
rows is the tallest output tile of the library (256 x 128 of the bf16x6 weight gradients, 128 x 256 of the wide row GEMM):
an overrun by a whole tile still lands in memory the test owns.

Not a conftest and no fixtures: tests import `guarded`."""
from __future__ import annotations

from typing import Optional

import torch

PATTERN_32 = 0x7FC0BEEF  # fp32: quiet NaN with a payload
PATTERN_16 = 0x7FC1      # bf16 and fp16: NaN
PATTERN_8 = 0x5A

_BITS = {4: (torch.int32, PATTERN_32), 2: (torch.int16, PATTERN_16), 1: (torch.int8, PATTERN_8)}


class Guarded:
    """`.view` ([rows, width], row stride `.ld`), `.ld`, `.assert_untouched(name)`; `.bits` is the whole allocation as integers
    of the element size and `.offset` the flat index of payload element (0, 0) (what the host tests plant their bit flips with)."""

    def __init__(self, rows: int, width: int, *, ld: int, dtype, device, lead: int = 4, guard_rows: int = 256,
                 live_rows: Optional[torch.Tensor] = None, any_width: bool = False):
        itemsize = torch.empty((), dtype=dtype).element_size()
        if itemsize not in _BITS:
            raise ValueError(f"guarded: unsupported dtype {dtype}")
        if rows < 0 or width <= 0 or ld < width:
            raise ValueError(f"guarded: need rows >= 0 and 0 < width <= ld (rows {rows} width {width} ld {ld})")
        if (ld * itemsize) % 16 and not any_width:  # any_width: operands the ABI addresses element by element ([*, 1] columns, routing words)
            raise ValueError(f"guarded: a row stride of {ld} x {itemsize} bytes breaks the 16-byte contract")
        bits_dtype, pattern = _BITS[itemsize]
        lead_elems = lead * 4 // itemsize  # `lead` counts floats (4 floats = 16 bytes)
        self.rows, self.width, self.ld, self.dtype = rows, width, ld, dtype
        self.offset = guard_rows * ld + lead_elems
        total = self.offset + rows * ld + guard_rows * ld
        self.pattern = pattern
        self.bits = torch.full((total,), pattern, dtype=bits_dtype, device=device)
        if self.bits.data_ptr() % 32:
            raise RuntimeError("guarded: the allocator returned a block that is not 32-byte aligned")
        typed = self.bits.view(dtype)
        self.view = typed[self.offset:self.offset + rows * ld].view(rows, ld)[:, :width]
        # everything that must keep the pattern: all but the payload (rows that live_rows marks False are guard as a whole:
        # the gap between the groups of a weight gradient)
        outside = torch.ones(total, dtype=torch.bool, device=device)
        live = outside[self.offset:self.offset + rows * ld].view(rows, ld)[:, :width]
        if live_rows is None:
            live.fill_(False)
        else:
            live_rows = torch.as_tensor(live_rows, dtype=torch.bool, device=device)
            if live_rows.shape != (rows,):
                raise ValueError("guarded: live_rows must have one entry per row")
            live.copy_(~live_rows[:, None].expand(rows, width))
        self._outside = outside
        self.live_rows = live_rows

    def data_ptr(self) -> int:
        return self.view.data_ptr()

    def fill(self, value) -> "Guarded":
        """payload := value (a scalar, or anything that broadcasts / copies into [rows, width]); guard rows of live_rows stay"""
        if self.live_rows is None:
            if torch.is_tensor(value):
                self.view.copy_(value)
            else:
                self.view.fill_(value)
        else:
            v = value if torch.is_tensor(value) else torch.full((1, 1), value, dtype=self.dtype)
            v = v.to(device=self.bits.device, dtype=self.dtype).expand(self.rows, self.width)
            self.view.copy_(torch.where(self.live_rows[:, None], v, self.view))
        return self

    def payload(self) -> torch.Tensor:
        """a contiguous copy of the payload (of the live rows)"""
        p = self.view if self.live_rows is None else self.view[self.live_rows]
        return p.clone()

    def _row_text(self, row: int) -> str:
        if row < 0:
            return f"-{-row}"
        return str(row) if row < self.rows else f"M+{row - self.rows}"

    def assert_untouched(self, name: str) -> None:
        """one bitwise comparison of everything outside the payload on the buffer's device, one synchronisation"""
        changed = (self.bits != self.pattern) & self._outside
        if not bool(changed.any()):  # the one sync
            return
        first = int(torch.nonzero(changed)[0])
        rel = first - self.offset
        row = rel // self.ld  # floor: elements in front of the payload get negative rows
        col = rel - row * self.ld
        mask = (1 << (8 * self.bits.element_size())) - 1
        raise AssertionError(
            f"{name}: {int(changed.sum())} element(s) outside the payload were written; the first is row {self._row_text(row)}, col {col} "
            f"(payload is {self.rows} x {self.width}, ld {self.ld}; flat element {first} now holds 0x{int(self.bits[first]) & mask:X}, "
            f"the pattern is 0x{self.pattern:X})")


def guarded(rows: int, width: int, *, ld: int, dtype, device, lead: int = 4, guard_rows: int = 256,
            live_rows: Optional[torch.Tensor] = None, any_width: bool = False) -> Guarded:
    """A [rows, width] operand with row stride ld inside one pattern-filled allocation.  With lead = 4 (floats) the view's
    data_ptr() is 16-byte aligned and NOT 32-byte aligned.  The payload starts out as the pattern too: an output element the
    kernel never writes reads back as NaN."""
    return Guarded(rows, width, ld=ld, dtype=dtype, device=device, lead=lead, guard_rows=guard_rows, live_rows=live_rows, any_width=any_width)
