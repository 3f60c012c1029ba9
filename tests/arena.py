"""A guarded arena for bounds tests: every buffer a launch is handed is a view of ONE uint8 tensor, cut to exactly its
stated size, with a band of a known pattern in front of it and behind it.

* A write outside a buffer lands in a band and `check()` names the buffer, the side and the byte.
* A stray read that reaches a result shows when the same launch is run under two patterns (`run_twice`): the bands,
  and every "don't care" region a test poisons inside a buffer, hold pattern A in one run and pattern B in the other, so
  any output bit that depends on them differs between the runs.

Patterns (16 bits, repeated by absolute byte offset so that a read at any element size sees the same thing):
  A = 0x7FC1: a NaN as bf16; doubled (0x7FC17FC1) a NaN as fp32; its high byte 0x7F is NaN as e4m3.
  B = 0x3F80: 1.0 as bf16; doubled ~1.0 as fp32; both bytes finite as e4m3.
A band next to an `index` buffer (ids, lists, counts, length records) holds the integer 0 under A and 1 under B at the
buffer's element size: both are valid indices wherever an id, a count or a length could be used, so a stray read of them
picks a wrong row and never forms a wild address.

The guard width is a condition a test has to meet, not a measurement: it must exceed the largest overshoot a clamped load
or a short size formula can produce at the shapes used — one 16-row tile of the widest row in fp32.  `need_guard` states
that bound and `Arena.require_guard` asserts it per case.

Works on any device (the CPU tests of the helper itself use "cpu"); the allocator does not matter."""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, Optional

import torch

PATTERNS = {"A": 0x7FC1, "B": 0x3F80}
INDEX_VALUE = {"A": 0, "B": 1}
KINDS = ("float", "index", "bytes")
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def need_guard(widest_row_elems: int) -> int:
    """Bytes a stray access can overshoot by at the shapes of a case: one 16-row tile of its widest row, in fp32."""
    return 16 * widest_row_elems * 4


def _itemsize(dtype) -> int:
    return torch.empty(0, dtype=dtype).element_size()


def _align_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def pattern_bytes(kind: str, itemsize: int, which: str, start: int, n: int) -> torch.Tensor:
    """The n pattern bytes (uint8, CPU) of a band that begins at absolute arena offset `start`."""
    if kind == "index":
        unit = list(int(INDEX_VALUE[which]).to_bytes(itemsize, "little"))
    else:
        unit = list(PATTERNS[which].to_bytes(2, "little"))
    period = len(unit)
    reps = (n + 2 * period) // period + 1
    return torch.tensor(unit, dtype=torch.uint8).repeat(reps)[start % period:start % period + n].clone()


_pattern_cache: dict = {}


def _pattern_on(device, kind: str, itemsize: int, which: str, start: int, n: int) -> torch.Tensor:
    """pattern_bytes on `device`, kept: the bands of an arena repeat a few (phase, length) pairs."""
    period = itemsize if kind == "index" else 2
    key = (str(device), kind == "index", period, which, start % period, n)
    if key not in _pattern_cache:
        if len(_pattern_cache) > 256:
            _pattern_cache.clear()
        _pattern_cache[key] = pattern_bytes(kind, itemsize, which, start % period, n).to(device)
    return _pattern_cache[key]


def pattern_scalar(dtype, kind: str, which: str) -> int:
    """The pattern as ONE element of `dtype`, as the integer of the same width (what `poison` stores)."""
    size = _itemsize(dtype)
    if kind == "index":
        return INDEX_VALUE[which]
    p = PATTERNS[which]
    if size == 1:
        return p >> 8                       # 0x7F (NaN as e4m3) / 0x3F
    v = 0
    for i in range(size // 2):
        v |= p << (16 * i)
    if v >= 1 << (8 * size - 1):
        v -= 1 << (8 * size)
    return v


class _Buf:
    __slots__ = ("name", "start", "end", "lo", "hi", "kind", "itemsize", "view")

    def __init__(self, name, start, end, lo, hi, kind, itemsize, view):
        self.name, self.start, self.end, self.lo, self.hi = name, start, end, lo, hi
        self.kind, self.itemsize, self.view = kind, itemsize, view


class Arena:
    """One uint8 tensor of `nbytes`; `take` cuts exact views out of it, each between two guard bands of >= `guard` bytes.
    The band in front spans [lo, start) — the guard plus the alignment padding — and the band behind spans exactly
    [end, end + guard): it begins at the view's last byte plus one, not at a rounded address."""

    def __init__(self, nbytes: int, device, guard: int = 65536):
        assert guard > 0 and nbytes > 0
        self.guard = int(guard)
        self.mem = torch.zeros(int(nbytes), dtype=torch.uint8, device=device)
        assert self.mem.data_ptr() % 16 == 0
        self.bufs: Dict[str, _Buf] = {}
        self.cursor = 0
        self.which = None

    @staticmethod
    def bytes_for(sizes: Iterable[int], guard: int = 65536, align: int = 256) -> int:
        """An arena size that holds views of the given byte sizes (each with its two bands and alignment slack)."""
        return sum(int(s) + 2 * guard + align for s in sizes) + align

    def require_guard(self, widest_row_elems: int) -> None:
        need = need_guard(widest_row_elems)
        assert self.guard > need, f"guard of {self.guard} bytes does not exceed one 16-row fp32 tile ({need} bytes)"

    def take(self, name: str, shape, dtype, align: int = 256, kind: str = "float", init=None) -> torch.Tensor:
        assert kind in KINDS and name not in self.bufs, (name, kind)
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        itemsize = _itemsize(dtype)
        assert align % itemsize == 0 and align % 2 == 0
        nbytes = math.prod(shape) * itemsize
        base = self.mem.data_ptr()
        lo = self.cursor
        start = _align_up(base + lo + self.guard, align) - base
        end = start + nbytes
        hi = end + self.guard
        assert hi <= self.mem.numel(), f"arena of {self.mem.numel()} bytes is full at {name!r} (needs {hi})"
        view = self.mem[start:end].view(dtype).view(shape)
        self.bufs[name] = _Buf(name, start, end, lo, hi, kind, itemsize, view)
        self.cursor = hi
        if init is not None:
            view.fill_(init)
        if self.which is not None:
            self._fill(self.bufs[name], self.which)
        return view

    def __getitem__(self, name: str) -> torch.Tensor:
        return self.bufs[name].view

    # ---- guards
    def _bands(self, b: _Buf):
        return (("before", b.lo, b.start), ("after", b.end, b.hi))

    def _fill(self, b: _Buf, which: str) -> None:
        for _, lo, hi in self._bands(b):
            self.mem[lo:hi].copy_(_pattern_on(self.mem.device, b.kind, b.itemsize, which, lo, hi - lo))

    def fill_guards(self, which: str) -> None:
        assert which in PATTERNS
        self.which = which
        for b in self.bufs.values():
            self._fill(b, which)

    def check(self, names=None) -> None:
        """Every guard byte still holds its pattern; otherwise names the buffer, the side and the first byte."""
        assert self.which is not None, "fill_guards first"
        for name in (names if names is not None else self.bufs):
            b = self.bufs[name]
            for side, lo, hi in self._bands(b):
                want = _pattern_on(self.mem.device, b.kind, b.itemsize, self.which, lo, hi - lo)
                got = self.mem[lo:hi]
                if torch.equal(got, want):
                    continue
                first = int((got != want).nonzero()[0]) + lo
                off = first - b.end if side == "after" else first - b.start      # >= 0 behind, < 0 in front
                raise AssertionError(
                    f"guard {side} buffer {name!r} overwritten: first at byte {off:+d} relative to the view's "
                    f"{'end' if side == 'after' else 'start'} (arena offset {first}), holds "
                    f"0x{int(self.mem[first]):02x}, pattern {self.which} has 0x{int(want[first - lo]):02x}; "
                    f"{int((got != want).sum())} guard bytes differ")

    def snapshot(self, names=None) -> Dict[str, torch.Tensor]:
        """Byte copies of the named views (all by default): what `unchanged` compares against after a launch."""
        return {n: self.mem[self.bufs[n].start:self.bufs[n].end].clone() for n in (names or self.bufs)}

    def unchanged(self, snap: Dict[str, torch.Tensor]) -> None:
        for n, old in snap.items():
            b = self.bufs[n]
            now = self.mem[b.start:b.end]
            if not torch.equal(now, old):
                first = int((now != old).nonzero()[0])
                raise AssertionError(f"buffer {n!r} was written: first at byte {first} of {b.end - b.start}")

    def poison(self, t: torch.Tensor, where, which: str, kind: Optional[str] = None) -> None:
        poison(t, where, which, kind)


def poison(t: torch.Tensor, where, which: str, kind: Optional[str] = None) -> None:
    """Fill a "don't care" region of `t` with pattern `which`: `where` is a bool mask of t's shape, one index (a slice or a
    tuple of slices), or a list of them.  Integer tensors wider than a byte count as `index` unless `kind` says otherwise."""
    if kind is None:
        kind = "index" if t.dtype in (torch.int32, torch.int64) else "float"
    ti = t.view(_INT_OF_SIZE[t.element_size()])
    val = pattern_scalar(t.dtype, kind, which)
    if isinstance(where, torch.Tensor):
        ti[where] = val
        return
    for idx in (where if isinstance(where, list) else [where]):
        ti[idx] = val


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor as integers of its element size: equality that tells NaNs apart and -0 from +0."""
    t = t.contiguous()
    return t if not t.is_floating_point() else t.view(_INT_OF_SIZE[t.element_size()])


def _first_diff(a: torch.Tensor, b: torch.Tensor) -> str:
    ne = (bits(a) != bits(b))
    idx = ne.nonzero()[0].tolist()
    return f"{int(ne.sum())} of {ne.numel()} elements differ, first at {idx}: {a[tuple(idx)].item()!r} vs {b[tuple(idx)].item()!r}"


def run_twice(arena: Arena, make_inputs: Callable[[str], None], launch: Callable[[], None],
              outputs: Callable[[], Dict[str, torch.Tensor]], valid: Optional[Callable[[], Dict[str, torch.Tensor]]] = None,
              sync: Optional[Callable[[], None]] = None) -> Dict[str, torch.Tensor]:
    """Three runs of one launch: guards A, guards A again, guards B.

    make_inputs(which) rewrites EVERY buffer the launch reads or writes from scratch — inputs, sentinel-filled outputs,
    residual streams, caches, zeroed tickets — and poisons the don't-care regions with pattern `which`.  outputs()
    returns the tensors to compare, whole, sentinels included (views are fine: they are cloned here; an output whose
    contents the contract leaves open in some region is passed as the slices it does specify); valid() optionally
    returns, per floating-point output, a bool mask of the elements the reference calls valid (without valid(): all).
    Asserts: guards intact after runs 1 and 3; the two A runs bit-equal ("not reproducible" otherwise); run 3 bit-equal
    to them (a stray read reached the result otherwise); every valid floating-point element finite.
    Returns the clones of run 1."""
    runs = []
    for phase, which in enumerate(("A", "A", "B")):
        arena.fill_guards(which)
        make_inputs(which)
        launch()
        if sync is not None:
            sync()
        if phase != 1:
            arena.check()
        runs.append({k: v.detach().clone() for k, v in outputs().items()})
    masks = valid() if valid is not None else {}
    for name, first in runs[0].items():
        a1, a2, b = (r[name].reshape(-1) if r[name].dim() == 0 else r[name] for r in runs)
        assert torch.equal(bits(a1), bits(a2)), f"{name}: not reproducible under one pattern: {_first_diff(a1, a2)}"
        assert torch.equal(bits(a1), bits(b)), \
            f"{name}: depends on guard / don't-care contents (pattern A vs B): {_first_diff(a1, b)}"
        m = masks.get(name)
        if first.is_floating_point() and (m is not None or valid is None):
            v = (first[m] if m is not None else first).float()
            assert bool(torch.isfinite(v).all()), f"{name}: {int((~torch.isfinite(v)).sum())} valid elements are not finite"
    return runs[0]
