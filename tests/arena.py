"""Tensors carved out of one poisoned allocation, for the memory-contract tests
(tests/test_gpu_memory_contract.py, tests/test_gpu_learner_layouts.py).

An Arena owns one uint8 buffer filled with the byte 0xFF.  Read as fp32, fp64 or
bf16 that pattern is a NaN; read as int32 / int64 it is -1 and as uint8 255, values
no kernel input takes.  carve() hands out a tensor of exactly the asked shape,
16-byte aligned, with `guard` bytes of pattern before and after it; carve_view() a
strided view of exactly the asked logical shape whose inter-row gaps keep the
pattern.  After a kernel ran on such tensors:

  * a value it USED from outside a view (a step past the slice's end, a row of the
    episode padding) is a NaN, which spreads to an output: the tests assert finite
    outputs that equal, bit for bit, a run on dense tensors;
  * a byte it WROTE outside a tensor's logical elements is found by check(), which
    compares every such byte of the buffer with the pattern and names the tensor
    whose guard or gap changed.

Outputs and workspaces are not cleared when carved: an output element the kernel
never wrote stays a NaN, so "finite" also means "every element written".

The guard is a condition, not a measurement: at least one full 16-row tile of the
widest record any kernel writes, 16 x 4E floats of the FFN hidden at the default
network (E = 32: 8 KiB).  A kernel that overruns by one tile then stays inside the
arena's own allocation and shows up as a failed check, never as a fault.
"""
import torch

PATTERN = 0xFF
ALIGN = 16
# one 16-row tile of the FFN hidden (4E floats per row) at the default network, E = 32
GUARD = 16 * 4 * 32 * 4
FLOAT_STRIDE_MULTIPLE = 4  # elements: what the kernels' 16-byte loads of a row need


class ArenaError(AssertionError):
    pass


def _round_up(n, m):
    return (n + m - 1) // m * m


class Arena:
    def __init__(self, nbytes, device="cpu"):
        self.device = torch.device(device)
        self.buf = torch.full((int(nbytes) + ALIGN,), PATTERN, dtype=torch.uint8, device=self.device)
        # bytes that belong to a carved tensor's logical elements (check() skips them)
        self.owned = torch.zeros_like(self.buf, dtype=torch.bool)
        self.top = (-self.buf.data_ptr()) % ALIGN  # first 16-byte aligned offset
        self.entries = []  # (name, lo, base, end, hi): [lo, base) guard, [base, end) span, [end, hi) guard

    # -- carving ---------------------------------------------------------------
    def carve(self, shape, dtype=torch.float32, guard=GUARD, name=None):
        """A contiguous tensor of exactly `shape`, 16-byte aligned, `guard` bytes of
        pattern on either side.  Its elements hold the pattern."""
        shape = tuple(int(s) for s in shape)
        strides, n = [], 1
        for s in reversed(shape):
            strides.append(n)
            n *= s
        return self._carve(shape, dtype, tuple(reversed(strides)), guard, name, 1)

    def carve_view(self, shape, dtype, strides, guard=GUARD, name=None, stride_multiple=None):
        """A view of exactly `shape` with the given element strides (positive, the
        logical elements distinct); everything between them keeps the pattern.  The
        base is 16-byte aligned; every stride of a float tensor, other than those of its
        dense inner axes, must be a multiple of `stride_multiple` elements (default 4:
        the rows stay 16-byte aligned)."""
        shape = tuple(int(s) for s in shape)
        strides = tuple(int(s) for s in strides)
        if len(shape) != len(strides) or any(s < 1 for s in strides):
            raise ValueError(f"carve_view: shape {shape} / strides {strides}")
        if stride_multiple is None:
            stride_multiple = FLOAT_STRIDE_MULTIPLE if dtype.is_floating_point else 1
        dense = 1  # (the dense inner axes of a row, e.g. [a][n_ent * F], are the tensor's own shape)
        for n, s in zip(reversed(shape), reversed(strides)):
            if n > 1 and s != dense and s % stride_multiple:
                raise ValueError(f"carve_view: stride {s} of a {dtype} tensor is not a multiple of {stride_multiple}")
            dense = dense * n if s == dense else 0
        return self._carve(shape, dtype, strides, guard, name, stride_multiple)

    def place(self, src, strides=None, guard=GUARD, name=None, stride_multiple=None):
        """carve (strides None) or carve_view a tensor like `src` and copy src into it."""
        if strides is None:
            t = self.carve(src.shape, src.dtype, guard, name)
        else:
            t = self.carve_view(src.shape, src.dtype, strides, guard, name, stride_multiple)
        t.copy_(src)
        return t

    def _carve(self, shape, dtype, strides, guard, name, _mult):
        if guard < GUARD:
            raise ValueError(f"guard {guard} B is under one 16-row tile of the widest record ({GUARD} B)")
        item = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        span = (1 + sum((n - 1) * s for n, s in zip(shape, strides))) if numel else 0
        lo = self.top
        base = _round_up(lo + guard, ALIGN)
        end = base + span * item
        hi = _round_up(end + guard, ALIGN)
        if hi > self.buf.numel():
            raise ArenaError(f"arena of {self.buf.numel()} B is full: {name or shape} needs bytes up to {hi}")
        self.top = hi
        name = name or f"#{len(self.entries)}{list(shape)}"
        self.entries.append((name, lo, base, end, hi))
        if not numel:
            return torch.empty(shape, dtype=dtype, device=self.device)
        t = self.buf[base:end].view(dtype).as_strided(shape, strides)
        assert t.data_ptr() % ALIGN == 0
        own = self.owned[base:end].as_strided(shape + (item,), tuple(s * item for s in strides) + (1,))
        own.fill_(True)
        if int(self.owned[base:end].sum()) != numel * item:
            raise ValueError(f"carve_view: strides {strides} make elements of shape {shape} overlap")
        return t

    # -- checking --------------------------------------------------------------
    def check(self, what=""):
        """Every byte outside the carved tensors' logical elements still holds the
        pattern; else ArenaError naming the tensor and the first offset."""
        bad = (self.buf != PATTERN) & ~self.owned
        if not bool(bad.any()):
            return
        off = int(torch.nonzero(bad)[0])
        n = int(bad.sum())
        where = f"byte {off}, outside every carved tensor"
        for name, lo, base, end, hi in self.entries:
            if lo <= off < hi:
                if off < base:
                    where = f"the guard before {name}: {base - off} B before its first element"
                elif off >= end:
                    where = f"the guard after {name}: {off - end} B past its last element"
                else:
                    where = f"a gap between the rows of {name}: byte {off - base} of its span"
                break
        raise ArenaError(f"{what + ': ' if what else ''}{n} byte(s) written outside the carved tensors, the first in "
                         f"{where} (arena offset {off})")
