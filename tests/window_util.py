"""Test plumbing: canary-guarded strided windows.  A kernel is handed ``Guarded(...).view`` -- a [rows, cols] window
of a larger buffer whose every other element holds a fixed NaN bit pattern -- and ``check()`` afterwards proves that
nothing outside the window was written.  Loaded with an input operand, the same buffer turns an over-read into a
neighbour column into a NaN in the output (a zero or finite neighbour would hide it)."""
import torch

# one fixed pattern per element type: a NaN in every floating type, so that an over-read shows in the result
PATTERN = {
    torch.float32: (torch.int32, 0x7FA5A5A5),
    torch.float16: (torch.int16, 0x7EA5),
    torch.bfloat16: (torch.int16, 0x7FA5),
    torch.float64: (torch.int64, 0x7FF5A5A5A5A5A5A5),
    torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A),
    torch.uint8: (torch.uint8, 0xA5),
}

# the largest row tile any kernel owns (128-row igemm tiles, the 256 pixels of a 16 x 16 patch): an overshoot by a
# whole tile still lands in guarded memory; the padded 3 x 3 gathers can form a negative row, hence the same in front
GUARD_ROWS = 256


class Guarded:
    def __init__(self, rows, cols, dtype, *, ld=None, c0=0, pre=GUARD_ROWS, post=GUARD_ROWS, device="cuda"):
        ld = cols if ld is None else ld
        assert rows > 0 and cols > 0 and c0 >= 0 and c0 + cols <= ld and pre >= 0 and post >= 0
        self.rows, self.cols, self.dtype, self.ld, self.c0, self.pre, self.post = rows, cols, dtype, ld, c0, pre, post
        self.itype, self.pattern = PATTERN[dtype]
        ibuf = torch.full((pre + rows + post, ld), self.pattern, dtype=self.itype, device=device)
        self.buf = ibuf.view(dtype)
        self.view = self.buf[pre:pre + rows, c0:c0 + cols]

    def load(self, t):
        """Copies the operand ``t`` ([rows, cols] or anything with as many elements) into the window; returns the view."""
        self.view.copy_(t.reshape(self.rows, self.cols).to(self.dtype))
        return self.view

    def regions(self):
        """(name, first row, first column, integer view) of the four regions outside the window."""
        ib = self.buf.view(self.itype)
        p, r, c, n = self.pre, self.rows, self.c0, self.cols
        return [("rows before", 0, 0, ib[:p]), ("rows after", p + r, 0, ib[p + r:]),
                ("columns left", p, 0, ib[p:p + r, :c]), ("columns right", p, c + n, ib[p:p + r, c + n:])]

    def clobbered(self):
        """None, or (region, row, column, bits found) of the first element outside the window that changed; row and
        column count from the window's first element (negative = before / left of it)."""
        for name, r0, c0, part in self.regions():
            if part.numel() == 0:
                continue
            bad = (part != self.pattern).nonzero()     # row-major order: the first entry is the first offender
            if bad.shape[0]:
                r, c = int(bad[0, 0]), int(bad[0, 1])
                bits = int(part[r, c]) & ((1 << (8 * part.element_size())) - 1)
                return name, r0 + r - self.pre, c0 + c - self.c0, bits
        return None

    def check(self, what="buffer"):
        hit = self.clobbered()
        assert hit is None, (f"{what}: write outside the window [{self.rows} x {self.cols}] (ld {self.ld}, c0 {self.c0}): "
                             f"{hit[0]}, row {hit[1]}, column {hit[2]} holds 0x{hit[3]:x}, not 0x{self.pattern:x}")


def guarded_flat(n, dtype, *, pre=1024, post=1024, device="cuda"):
    """A flat n-element buffer with the canary starting at element n: one row of n columns between guard elements."""
    g = Guarded(1, n, dtype, ld=pre + n + post, c0=pre, pre=0, post=0, device=device)
    g.flat = g.view.reshape(-1)
    return g


def layout(kind, cols, quantum, out_quantum=None):
    """(ld, c0) of the three layouts: 'dense' (row guards only), 'tight' (the smallest ld > cols and the smallest
    non-zero c0 the contract allows: ``out_quantum`` elements of stride over ``quantum`` elements of offset), 'wide'
    (c0 = cols, ld = 3 cols whatever the quanta: a caller that needs two wide windows of different stride, such as
    ldr != ldo, widens one of them itself)."""
    if kind == "dense":
        return cols, 0
    if kind == "tight":
        return cols + (out_quantum or quantum), quantum
    assert kind == "wide"
    return 3 * cols, cols
