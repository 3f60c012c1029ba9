"""The guarded arena itself (tests/arena.py), on the CPU: view sizes and alignment, the guard patterns, what `check`
reports for a planted write, and that `run_twice` catches fake "kernels" (torch functions) which read past their input or
leave a masked row unmasked — the detections the GPU bounds tests rely on, and the stand-ins for kernel mutants whose stray
access cannot be shown to stay inside the guard (profiles/bounds_tests.txt)."""
import pytest
import torch

import arena as A

BF16 = torch.bfloat16


def _arena(guard=4096):
    return A.Arena(1 << 20, "cpu", guard=guard)


def test_views_are_exact_and_aligned():
    ar = _arena()
    specs = [("a", (3, 5), BF16, 256, "float"), ("b", 7, torch.uint8, 2, "bytes"), ("c", (2, 8), torch.int32, 64, "index"),
             ("d", (1,), torch.int64, 4096, "index"), ("e", (16, 33), torch.float32, 16, "float")]
    prev_end = 0
    for name, shape, dt, align, kind in specs:
        v = ar.take(name, shape, dt, align=align, kind=kind)
        b = ar.bufs[name]
        n = v.numel() * v.element_size()
        assert tuple(v.shape) == ((shape,) if isinstance(shape, int) else shape) and v.dtype == dt
        assert b.end - b.start == n and v.untyped_storage().data_ptr() == ar.mem.untyped_storage().data_ptr()
        assert v.data_ptr() == ar.mem.data_ptr() + b.start and v.data_ptr() % align == 0
        assert b.start - b.lo >= ar.guard and b.hi - b.end == ar.guard       # the band behind starts at the last byte + 1
        assert b.lo == prev_end                                              # no byte between two buffers is unguarded
        prev_end = b.hi
    with pytest.raises(AssertionError):
        ar.take("a", 4, BF16)                                                # a name is taken once
    with pytest.raises(AssertionError, match="full"):
        ar.take("big", 1 << 20, torch.uint8)
    z = ar.take("z", 64, torch.int32, kind="index", init=0)
    assert int(z.abs().sum()) == 0


def test_guard_patterns_read_as_documented():
    ar = _arena()
    ar.take("f", 5, BF16)                       # 10 bytes
    ar.take("odd", 3, torch.uint8, align=2, kind="bytes")
    ar.take("i4", 3, torch.int32, kind="index")
    ar.take("i8", 3, torch.int64, kind="index")
    f, odd, i4, i8 = (ar.bufs[n] for n in ("f", "odd", "i4", "i8"))
    ar.fill_guards("A")
    behind = ar.mem[f.end:f.end + 64].clone()          # (a copy: views at other element sizes need an aligned offset)
    assert torch.isnan(behind.view(BF16).float()).all() and torch.isnan(behind.view(torch.float32)).all()
    assert int(behind.view(torch.int16)[0]) == 0x7FC1 and int(behind[1]) == 0x7F
    assert torch.isnan(ar.mem[f.start - 64:f.start].clone().view(BF16).float()).all()
    # behind an odd-sized byte buffer the pattern keeps its phase by absolute offset: the next even address is a NaN
    assert odd.end % 2 == 1 and torch.isnan(ar.mem[odd.end + 1:odd.end + 33].clone().view(BF16).float()).all()
    assert int(ar.mem[i4.end:i4.end + 64].clone().view(torch.int32).abs().sum()) == 0
    ar.fill_guards("B")
    assert torch.all(ar.mem[f.end:f.end + 64].clone().view(BF16).float() == 1.0)
    assert torch.all((ar.mem[f.end:f.end + 64].clone().view(torch.float32) - 1.0).abs() < 1e-2)
    assert torch.all(ar.mem[i4.end:i4.end + 64].clone().view(torch.int32) == 1)
    assert torch.all(ar.mem[i4.start - 64:i4.start].clone().view(torch.int32) == 1)
    assert torch.all(ar.mem[i8.end:i8.end + 64].clone().view(torch.int64) == 1)
    ar.check()
    late = ar.take("late", 4, torch.float32)        # taken after the fill: guarded at once
    assert torch.all(ar.mem[ar.bufs["late"].end:ar.bufs["late"].end + 8].clone().view(BF16).float() == 1.0) and late.numel() == 4
    ar.check()


def test_need_guard_is_a_condition():
    assert A.need_guard(8192) == 16 * 8192 * 4 == 8 * 65536
    ar = A.Arena(1 << 16, "cpu", guard=4096)
    ar.require_guard(63)
    with pytest.raises(AssertionError, match="does not exceed"):
        ar.require_guard(64)                        # 16 * 64 * 4 == 4096: not exceeded


@pytest.mark.parametrize("which", ["A", "B"])
def test_check_names_a_planted_write(which):
    ar = _arena()
    ar.take("first", 10, BF16)
    ar.take("mid", (4, 6), torch.float32)
    ar.take("idx", 9, torch.int32, kind="index")
    ar.fill_guards(which)
    ar.check()
    mid, idx = ar.bufs["mid"], ar.bufs["idx"]

    def planted(off, value):
        old = int(ar.mem[off])
        ar.mem[off] = value
        try:
            with pytest.raises(AssertionError) as e:
                ar.check()
        finally:
            ar.mem[off] = old
        ar.check()
        return str(e.value)
    msg = planted(mid.end, 0x55)                                     # the byte at view_end
    assert "after buffer 'mid'" in msg and "byte +0 " in msg and "0x55" in msg
    msg = planted(mid.start - 1, 0x55)                               # the byte before view_start
    assert "before buffer 'mid'" in msg and "byte -1 " in msg
    msg = planted(mid.hi - 1, 0x55)                                  # the last guard byte
    assert "after buffer 'mid'" in msg and f"byte +{ar.guard - 1} " in msg
    msg = planted(idx.end + 4, 7)                                    # an index band: one element behind
    assert "after buffer 'idx'" in msg and "byte +4 " in msg
    ar.mem[mid.end] = 0x55
    ar.check(names=["first"])                                        # only the named buffers are looked at
    with pytest.raises(AssertionError, match="'mid'"):
        ar.check(names=["mid"])


def test_snapshot_and_poison():
    ar = _arena()
    x = ar.take("x", (4, 8), BF16, init=2.0)
    y = ar.take("y", 6, torch.int64, kind="index", init=5)
    q = ar.take("q", 8, torch.uint8, kind="bytes", init=3)
    w = ar.take("w", (2, 3), torch.float32, init=0.5)
    snap = ar.snapshot(["x", "y"])
    ar.unchanged(snap)
    A.poison(x, (slice(2, None), slice(None)), "A")
    assert torch.isnan(x[2:].float()).all() and torch.all(x[:2] == 2.0)
    assert torch.all(x[2:].view(torch.int16) == 0x7FC1)
    with pytest.raises(AssertionError, match="'x' was written: first at byte 32"):
        ar.unchanged(snap)
    A.poison(x, (slice(2, None), slice(None)), "B")
    assert torch.all(x[2:] == 1.0)
    m = torch.zeros(6, dtype=torch.bool)
    m[4:] = True
    A.poison(y, m, "B")
    assert y.tolist() == [5, 5, 5, 5, 1, 1]
    A.poison(y, m, "A")
    assert y.tolist() == [5, 5, 5, 5, 0, 0]
    A.poison(q, [slice(0, 2), slice(6, 8)], "A")
    assert q.tolist() == [0x7F, 0x7F, 3, 3, 3, 3, 0x7F, 0x7F]
    A.poison(w, (1, slice(None)), "A")
    assert torch.isnan(w[1]).all() and torch.all(w[1].view(torch.int32) == 0x7FC17FC1) and torch.all(w[0] == 0.5)
    A.poison(w, (1, slice(None)), "B")
    assert torch.all((w[1] - 1.0).abs() < 1e-2)


# ---- fake kernels: a row sum over an input of `n` valid rows out of 16 ---------------------------------------------
ROWS, K = 16, 32


def _setup(n_valid=5):
    ar = _arena()
    x = ar.take("x", (ROWS, K), BF16)
    cnt = ar.take("cnt", 1, torch.int32, kind="index")
    out = ar.take("out", (ROWS,), torch.float32)
    g = torch.Generator().manual_seed(1)
    data = torch.randint(-3, 4, (ROWS, K), generator=g).to(BF16)

    def make_inputs(which):
        x.copy_(data)
        A.poison(x, (slice(n_valid, None), slice(None)), which)     # rows at or past the count: don't care
        cnt.fill_(n_valid)
        out.fill_(-7.0)
    return ar, x, cnt, out, data, make_inputs


def _flat_after(ar, name, n, dtype):
    """What a kernel sees when it runs n bytes past the end of a view."""
    b = ar.bufs[name]
    return ar.mem[b.end:b.end + n].view(dtype)


def test_run_twice_passes_an_honest_kernel():
    ar, x, cnt, out, data, make_inputs = _setup()

    def honest():
        n = int(cnt[0])
        loaded = x.float()                                           # all 16 rows are loaded ...
        mask = (torch.arange(ROWS) < n)[:, None]
        out[:n] = torch.where(mask, loaded, torch.zeros(())).sum(1)[:n]   # ... and masked behind the load
    res = A.run_twice(ar, make_inputs, honest, lambda: {"out": out},
                      valid=lambda: {"out": torch.arange(ROWS) < 5})
    assert torch.equal(res["out"][:5], data[:5].float().sum(1)) and torch.all(res["out"][5:] == -7.0)


def test_run_twice_catches_a_read_past_the_input():
    ar, x, cnt, out, data, make_inputs = _setup(n_valid=16)

    def one_past():
        flat = torch.cat([x.reshape(-1), _flat_after(ar, "x", 2, BF16)]).float()     # K + 1 elements of the last row
        out[:] = x.float().sum(1)
        out[15] = flat[15 * K:16 * K + 1].sum()
    with pytest.raises(AssertionError, match="out: (depends on guard|.*not finite)"):
        A.run_twice(ar, make_inputs, one_past, lambda: {"out": out})


def test_run_twice_catches_an_unmasked_row():
    ar, x, cnt, out, data, make_inputs = _setup(n_valid=5)

    def off_by_one_mask():
        n = int(cnt[0])
        mask = (torch.arange(ROWS) <= n)[:, None]                     # row n gets in
        s = torch.where(mask, x.float(), torch.zeros(())).sum(1)
        out[:n] = s[:n] + s[n:].sum()                                 # a column reduction over the "zero" rows
    with pytest.raises(AssertionError, match="out: depends on guard / don't-care contents"):
        A.run_twice(ar, make_inputs, off_by_one_mask, lambda: {"out": out})


def test_run_twice_catches_a_write_past_the_output_and_a_short_workspace():
    ar, x, cnt, out, data, make_inputs = _setup(n_valid=16)

    def one_more_row():
        out[:] = x.float().sum(1)
        _flat_after(ar, "out", 4, torch.float32)[0] = 1.0             # a store-side count test loosened by one
    with pytest.raises(AssertionError, match="guard after buffer 'out' overwritten: first at byte \\+0 "):
        A.run_twice(ar, make_inputs, one_more_row, lambda: {"out": out})

    # a workspace formula 16 bytes short: the kernel's last ticket lies behind the view
    ar2 = _arena()
    ws = ar2.take("ws", 64 - 4, torch.int32, kind="index", init=0)
    o2 = ar2.take("o", 4, torch.float32)

    def tickets():
        full = torch.cat([ws, _flat_after(ar2, "ws", 16, torch.int32)])
        o2[:] = float(full[63])                                       # reads its ticket behind the view: 0 or 1
        _flat_after(ar2, "ws", 16, torch.int32)[3] = 0                # and "leaves it at zero again"
    with pytest.raises(AssertionError):
        A.run_twice(ar2, lambda which: (ws.zero_(), o2.fill_(-1.0)), tickets, lambda: {"o": o2})


def test_run_twice_reports_a_launch_that_is_not_reproducible():
    ar, x, cnt, out, data, make_inputs = _setup(n_valid=16)
    calls = []

    def drifting():
        calls.append(1)
        out[:] = x.float().sum(1) + (1.0 if len(calls) == 2 else 0.0)
    with pytest.raises(AssertionError, match="out: not reproducible"):
        A.run_twice(ar, make_inputs, drifting, lambda: {"out": out})


def test_run_twice_requires_finite_valid_elements_only():
    ar, x, cnt, out, data, make_inputs = _setup(n_valid=5)

    def nan_sentinel(which):
        make_inputs(which)
        out.fill_(float("nan"))

    def honest():
        out[:5] = x[:5].float().sum(1)
    A.run_twice(ar, nan_sentinel, honest, lambda: {"out": out}, valid=lambda: {"out": torch.arange(ROWS) < 5})
    with pytest.raises(AssertionError, match="not finite"):
        A.run_twice(ar, nan_sentinel, honest, lambda: {"out": out}, valid=lambda: {"out": torch.arange(ROWS) < 6})
