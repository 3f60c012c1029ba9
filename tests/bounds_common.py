"""Scaffolding shared by the GPU bounds tests (test_hip_bounds_*.py): an arena sized from a case's buffers, the run under
two guard patterns, and the comparison against a run on ordinary, four times larger, zeroed workspaces.

The three properties every bounds test states (tests/arena.py has the mechanism):
  W  no write outside: all guards intact, and inside the outputs everything the header calls "not written" keeps its
     sentinel (the outputs are compared whole, sentinels included);
  R  no stray read reaches the result: outputs bit-equal under guard patterns A and B, the patterns also filling every
     "don't care" region the header names;
  S  the size formula suffices: every workspace is an arena view of exactly the library's own figure, and the outputs
     equal, bit for bit, those of the same launch on torch.zeros workspaces of four times the size."""
import torch

import arena as A

BF16, F32, I32, I64, U8 = torch.bfloat16, torch.float32, torch.int32, torch.int64, torch.uint8


def dev():
    return torch.device("cuda", 0)


def cuda_gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def small_ints(shape, seed, lo=-2, hi=2):
    """bf16 integers in [lo, hi] drawn on the device: every product and fp32 sum of them is exact."""
    return torch.randint(lo, hi + 1, shape, generator=cuda_gen(seed), device=dev(), dtype=torch.int8).to(BF16)


def nbytes(shape, dtype):
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = torch.empty(0, dtype=dtype).element_size()
    for s in shape:
        n *= s
    return n


class Case:
    """An arena whose guard exceeds one 16-row fp32 tile of the case's widest row (asserted), sized from a plan of
    (name, shape, dtype[, kind[, init]]) buffers which are then taken in order: `c.name` is the view."""

    def __init__(self, widest_row: int, plan):
        guard = A.need_guard(widest_row) + 256
        self.arena = A.Arena(A.Arena.bytes_for([nbytes(p[1], p[2]) for p in plan], guard), dev(), guard)
        self.arena.require_guard(widest_row)
        assert self.arena.mem.numel() < 1 << 29, "the arena of a bounds case stays well under 1 GB"
        for p in plan:
            name, shape, dtype = p[:3]
            kind = p[3] if len(p) > 3 else "float"
            init = p[4] if len(p) > 4 else None
            setattr(self, name, self.arena.take(name, shape, dtype, kind=kind, init=init))

    def run(self, make_inputs, launch, outputs, valid=None, finite=True):
        """run_twice on this arena.  finite=False: the outputs hold NaN sentinels (or NaN by construction) and the test
        asserts finiteness of the valid elements itself; otherwise `valid` masks (default: everything) must be finite."""
        if not finite:
            valid = dict                                   # no masks: run_twice then asserts nothing about finiteness
        return A.run_twice(self.arena, make_inputs, launch, outputs, valid, sync=torch.cuda.synchronize)

    def same_on_big_workspaces(self, make_inputs, launch_with, ws_names, outputs, res):
        """S: launch_with(**workspaces) on torch.zeros tensors of four times each arena view's size gives the bits `res`
        (run 1 of `run`) holds."""
        big = {n: torch.zeros(4 * getattr(self, n).numel(), dtype=getattr(self, n).dtype, device=dev()) for n in ws_names}
        make_inputs("A")
        launch_with(**big)
        torch.cuda.synchronize()
        for name, t in outputs().items():
            assert torch.equal(A.bits(t), A.bits(res[name])), \
                f"{name}: differs between exact-size and 4x workspaces: {A._first_diff(t, res[name])}"


def check_launch(widest_row, plan, make, launch, out_names, ws_names=()):
    """W, R and S for a launch written as launch(t) over a namespace t of tensors: run inside the arena (t = the Case:
    make(c, which) fills its views), then once more on ordinary torch allocations holding the same bytes — clones of the
    views, the workspaces named in ws_names as torch.zeros of four times their size (four times the leading dimension,
    so that row strides stay) — whose outputs must equal the arena's bit for bit.  The outputs may hold NaN sentinels:
    finiteness of the valid elements is the calling test's to assert.  Returns (the Case, the outputs of the first run)."""
    from types import SimpleNamespace
    c = Case(widest_row, plan)
    names = [p[0] for p in plan]
    # (an output is a buffer's name, or (label, function of the namespace) for the part of a buffer the launch specifies)
    outs = lambda t: {(n if isinstance(n, str) else n[0]): (getattr(t, n) if isinstance(n, str) else n[1](t))      # noqa: E731
                      for n in out_names}
    assert all(n in names for n in ws_names), ws_names
    res = c.run(lambda which: make(c, which), lambda: launch(c), lambda: outs(c), finite=False)
    make(c, "A")

    def big(v):
        return torch.zeros((4 * v.shape[0],) + tuple(v.shape[1:]), dtype=v.dtype, device=dev())
    twin = SimpleNamespace(**{n: (big(getattr(c, n)) if n in ws_names else getattr(c, n).clone()) for n in names})
    launch(twin)
    torch.cuda.synchronize()
    for n, t in outs(twin).items():
        assert torch.equal(A.bits(t), A.bits(res[n])), f"{n}: arena and ordinary allocation differ: {A._first_diff(t, res[n])}"
    return c, res


def frag16(x):
    """[16, K] rows -> the frag16 layout [K/8][16][8] as a flat tensor (what dfl_pack_rows writes), by plain indexing."""
    K = x.shape[1]
    return x.view(16, K // 8, 8).permute(1, 0, 2).reshape(-1).contiguous()


def first_argmax(lg):
    m = lg.max(dim=-1, keepdim=True).values
    idx = torch.arange(lg.shape[-1], device=lg.device).expand_as(lg)
    return torch.where(lg == m, idx, lg.shape[-1]).min(dim=-1).values
