"""Guarded buffers for the C ABI's memory contract (include/pg_directgcn.h: row-major matrices with an explicit
leading dimension, exact-size flat outputs). A helper module like pool_ref.py / pca_ref.py, not a conftest.

A kernel that stores outside its output -- a partial tile that writes row M, a 16-byte store that spills into the pad
columns, a pass that runs past its workspace -- lands in memory no value comparison reads. Here every output lives in
one allocation whose every element outside the [rows, cols] view is a guard holding a sentinel bit pattern, and
``check()`` compares the guards as integers (the sentinel is a NaN, which equals itself that way):

    front guard | row 0: head (shift) . view . pad | row 1: ... | ... | back guard

  * ``Guarded(rows, cols, dtype, device, ld, shift)``: an OUTPUT; view and guards start as the sentinel, so a result
    element the kernel never wrote is still the sentinel too (``assert_written`` / ``assert_untouched``).
  * ``Guarded.of(tensor, ld, shift)``: an INPUT; the view holds the tensor, the guards NaN: a kernel that folds a pad
    into a result shows up in the value comparison. That NaN has a payload of its own (INPUT_NAN): a sum that took in
    an input's guard and is stored into an output's guard then differs from the output's sentinel.
  * ``GuardedFlat(sizes, dtype, device)``: 1-D payloads of exact sizes at 16-byte aligned starts of one allocation,
    a guard gap in front of each and a tail behind the last.

The front guard is rounded up so that the first row starts on a 64-byte boundary whatever ld is: ``shift`` alone
decides the view's alignment.
"""
import torch

# dtype -> (integer dtype of the same size, sentinel bits). Quiet NaNs with a payload no arithmetic produces (the
# default NaN of the hardware and of torch has a zero payload); int32 has no NaN and takes a value no index reaches.
SENTINEL = {
    torch.float32: (torch.int32, 0x7FC5A5A5),
    torch.bfloat16: (torch.int16, 0x7FE5),
    torch.float16: (torch.int16, 0x7E5A),
    torch.float64: (torch.int64, 0x7FF8A5A5A5A5A5A5),
    torch.int32: (torch.int32, 0x5A5AA5A5),
}
# The NaN of INPUT guards carries another payload: arithmetic hands a NaN operand's payload on, so a kernel that reads
# an input's pad or guard row and stores the sum into an output guard would otherwise write the very bits it finds there.
INPUT_NAN = {
    torch.float32: 0x7FD3C3C3,
    torch.bfloat16: 0x7FD3,
    torch.float16: 0x7F3C,
    torch.float64: 0x7FFC3C3C3C3C3C3C,
    torch.int32: 0x3C3CC3C3,
}
DTYPES = tuple(SENTINEL)
ALIGN_BYTES = 64


class GuardError(AssertionError):
    pass


def _sentinel_buffer(n, dtype, device, bits=None):
    idt = SENTINEL[dtype][0]
    return torch.full((n,), SENTINEL[dtype][1] if bits is None else bits, dtype=idt, device=device).view(dtype)


def _first(mask):
    """Index of the first True of a 1-D bool tensor."""
    return int(torch.nonzero(mask)[0, 0])


class Guarded:
    """A [rows, cols] matrix view with leading dimension ld, `shift` elements into its first row, inside guards."""

    def __init__(self, rows, cols, dtype=torch.float32, device="cpu", ld=None, shift=0, guard_rows=2, name="buffer",
                 bits=None):
        ld = cols if ld is None else int(ld)
        if dtype not in SENTINEL:
            raise TypeError(f"no sentinel for {dtype}")
        if rows < 0 or cols < 0 or shift < 0 or shift + cols > ld or guard_rows < 1:
            raise ValueError("need 0 <= shift, shift + cols <= ld and at least one guard row")
        self.rows, self.cols, self.ld, self.shift, self.dtype, self.name = rows, cols, ld, shift, dtype, name
        es = torch.empty((), dtype=dtype).element_size()
        per = ALIGN_BYTES // es
        self.front = -(-max(guard_rows * ld, 1) // per) * per  # whole alignment units: row 0 starts aligned
        self.back = max(guard_rows * ld, 1)
        self.bits = SENTINEL[dtype][1] if bits is None else bits  # what every guard element holds
        self.buf = _sentinel_buffer(self.front + rows * ld + self.back, dtype, device, self.bits)
        self.view = self.buf.as_strided((rows, cols), (ld, 1), self.front + shift)
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=device)
        inside.as_strided((rows, cols), (ld, 1), self.front + shift).fill_(True)
        self._guard = ~inside

    @classmethod
    def of(cls, t, ld=None, shift=0, guard_rows=2, name="input"):
        """Input buffer: the view filled from the 2-D tensor t, NaN guards (INPUT_NAN's payload) around it."""
        g = cls(t.size(0), t.size(1), t.dtype, t.device, ld, shift, guard_rows, name, INPUT_NAN[t.dtype])
        g.view.copy_(t)
        return g

    def ptr(self):
        return self.view.data_ptr()

    def _bits(self):
        return self.buf.view(SENTINEL[self.dtype][0])

    def locate(self, off):
        """(region, row, column) of flat offset `off`; row / column count from the view's first element."""
        q = off - (self.front + self.shift)
        r, c = q // self.ld, q % self.ld
        if off < self.front:
            return "front rows", r, c
        if off >= self.front + self.rows * self.ld:
            return "back rows", r, c
        if off < self.front + self.shift:
            return "head of the first row", r, c
        return ("view" if c < self.cols else "pad columns"), r, c

    def check(self):
        """Every guard element still holds the sentinel bits; GuardError names the region and the first (row, col)."""
        bad = (self._bits() != self.bits) & self._guard
        n = int(bad.sum())
        if n:
            region, r, c = self.locate(_first(bad))
            raise GuardError(f"{self.name}: {n} guard element(s) overwritten, first in the {region} at (row {r}, "
                             f"column {c}) of the [{self.rows}, {self.cols}] view (ld {self.ld}, shift {self.shift})")

    def assert_untouched(self):
        """View and guards alike still hold the sentinel (a call that must return before it launches)."""
        bad = self._bits() != self.bits
        n = int(bad.sum())
        if n:
            region, r, c = self.locate(_first(bad))
            raise GuardError(f"{self.name}: {n} element(s) written by a call that must not launch, first in the "
                             f"{region} at (row {r}, column {c})")

    def assert_written(self):
        """No element of the view is NaN (for int32: none still holds the sentinel): every element was written with
        a number. Then the guards are checked."""
        if self.dtype == torch.int32:
            bad = self.view == self.bits
        else:
            bad = torch.isnan(self.view)
        n = int(bad.sum())
        if n:
            r, c = (int(v) for v in torch.nonzero(bad)[0])
            raise GuardError(f"{self.name}: {n} NaN / unwritten element(s) in the result, first at (row {r}, "
                             f"column {c})")
        self.check()


class GuardedFlat:
    """Exact-size 1-D payloads (work, grads, dW, partial sums, a loss scalar...) carved at 16-byte aligned starts out
    of one sentinel-filled allocation: a gap of `gap` elements in front of each and a tail behind the last."""

    def __init__(self, sizes, dtype=torch.float32, device="cpu", gap=64, name="flat"):
        single = isinstance(sizes, int)
        sizes = [sizes] if single else [int(s) for s in sizes]
        if dtype not in SENTINEL or any(s < 0 for s in sizes):
            raise ValueError("sizes >= 0 of a dtype with a sentinel")
        es = torch.empty((), dtype=dtype).element_size()
        per = 16 // es if es <= 16 else 1
        gap = -(-max(int(gap), 1) // per) * per
        self.dtype, self.name, self.sizes, self.starts = dtype, name, sizes, []
        o = 0
        for s in sizes:
            o = -(-(o + gap) // per) * per
            self.starts.append(o)
            o += s
        self.buf = _sentinel_buffer(o + gap, dtype, device)
        self.views = [self.buf[a:a + s] for a, s in zip(self.starts, sizes)]
        self.view = self.views[0]
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=device)
        for a, s in zip(self.starts, sizes):
            inside[a:a + s] = True
        self._guard = ~inside

    def ptr(self, i=0):
        return self.views[i].data_ptr()

    def _bits(self):
        return self.buf.view(SENTINEL[self.dtype][0])

    def locate(self, off):
        """(region, tensor index, distance): 'tail' = behind payload i by `distance` elements (1 = the element right
        after it), 'front' = before payload i by `distance`, 'payload' = inside it at `distance`."""
        for i, (a, s) in enumerate(zip(self.starts, self.sizes)):
            if off < a:
                prev_end = self.starts[i - 1] + self.sizes[i - 1] if i else None
                if prev_end is not None and off - prev_end < a - off:
                    return "tail", i - 1, off - prev_end + 1
                return "front", i, a - off
            if off < a + s:
                return "payload", i, off - a
        last = len(self.sizes) - 1
        return "tail", last, off - (self.starts[last] + self.sizes[last]) + 1

    def check(self):
        bad = (self._bits() != SENTINEL[self.dtype][1]) & self._guard
        n = int(bad.sum())
        if n:
            region, i, d = self.locate(_first(bad))
            raise GuardError(f"{self.name}: {n} guard element(s) overwritten, first in the {region} of tensor {i} "
                             f"({self.sizes[i]} elements), {d} element(s) from it")

    def assert_untouched(self):
        bad = self._bits() != SENTINEL[self.dtype][1]
        n = int(bad.sum())
        if n:
            region, i, d = self.locate(_first(bad))
            raise GuardError(f"{self.name}: {n} element(s) written by a call that must not launch, first in the "
                             f"{region} of tensor {i} at {d}")

    def assert_written(self):
        """No payload element is NaN (int32: none still holds the sentinel); then the guards are checked."""
        for i, v in enumerate(self.views):
            bad = (v == SENTINEL[self.dtype][1]) if self.dtype == torch.int32 else torch.isnan(v)
            n = int(bad.sum())
            if n:
                raise GuardError(f"{self.name}: {n} NaN / unwritten element(s) in tensor {i}, first at {_first(bad)}")
        self.check()
