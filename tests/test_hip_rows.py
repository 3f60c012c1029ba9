"""csrc/rows.hip and the row stages of csrc/prefill.hip, launched directly, against tests/rows_ref.py (torch fp64 on the
CPU): every compiled form of dfl_norm_pack, every argument form the product uses (row_off, h_out2 / ld2 taps, in-place
residual, ctx_rows_override / row_base, kv-only context), pos0 != S everywhere, positions near 40000, and rows small
enough that eps decides rstd.  Every buffer a launch may write starts as NaN, so "left alone" is checked bit for bit;
every valid row of every case is compared.  tests/test_rows_cpu.py shows that each planted fault of rows_ref.FAULTS
fails these very checks on these very inputs."""
import pytest
import torch

import helpers as H
import rows_ref as R

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops as o
    return o


def dev():
    return torch.device("cuda", 0)


def nans(*shape):
    return torch.full(shape, NAN, dtype=BF16, device=dev())


def g_(t):
    return None if t is None else t.to(dev())


def record(words: dict) -> torch.Tensor:
    """A length record whose other words hold a value no case uses for a count."""
    d = torch.full((8,), 13, dtype=I32)
    for k, v in words.items():
        d[k] = v
    return d.to(dev())


def test_norm_pack_form_of_each_width():
    """The k_norm_pack<N> named in the ids: N x 256 threads-worth of 8-column chunks, as dfl_norm_pack picks it."""
    assert [R.norm_pack_kernel(h) for h in (8, 4096, 4104, 5120, 8192, 8200, 16384)] == [2, 2, 4, 4, 4, 8, 8]
    assert {R.norm_pack_kernel(c.H) for c in R.norm_pack_cases()} == {2, 4, 8}


# ---------------------------------------------------------------- dfl_norm_pack
@pytest.mark.parametrize("c", R.norm_pack_cases(), ids=lambda c: c.id)
def test_norm_pack(ops, c):
    inp = R.norm_pack_inputs(c)
    want = R.norm_pack_ref(c, inp)
    nv = 16 if c.nv is None else c.nv
    frag = nans(16 * c.H)
    kw = dict(norm_w=g_(inp.w), frag=frag, H=c.H, eps=c.eps)
    if inp.part is not None:
        kw.update(part=g_(inp.part), nsplit=c.nsplit, part_split=c.part_split, ldp=c.ldp, row_off=c.row_off)
    resid = g_(inp.resid)
    if resid is not None:
        kw.update(resid_in=resid)
    if inp.embed is not None:
        kw.update(embed=g_(inp.embed), ids=g_(inp.ids))
    if c.nv is not None:
        kw.update(dyn=record({c.dyn_word: c.nv}), dyn_word=c.dyn_word)
    h_out, wide, want_h = None, None, want["h"]
    if c.out in ("h_out", "tap"):
        h_out = nans(16, c.H)
    elif c.out in ("inplace", "inplace_tap"):           # target.py: h_out IS the residual tensor; rows >= n_valid keep theirs
        h_out = resid
        want_h = want["h"].clone()
        want_h[nv:] = inp.resid[nv:]
    if h_out is not None:
        kw.update(h_out=h_out)
    if c.out in ("tap", "inplace_tap"):                 # a column slice of a wider buffer: only the slice may change
        wide = nans(16, c.ld2)
        kw.update(h_out2=wide[:, c.tap_off:c.tap_off + c.H], ld2=c.ld2)
    ops.norm_pack(**kw)
    torch.cuda.synchronize()
    R.check_norm_pack(c.id, {"h": h_out, "frag": H.unfrag(frag, c.H)}, {"h": want_h, "frag": want["frag"]})
    R.assert_bits(f"{c.id} zero fragments", H.unfrag(frag, c.H)[nv:], torch.zeros(16 - nv, c.H, dtype=BF16))
    if wide is not None:
        img = torch.full((16, c.ld2), NAN, dtype=BF16)
        img[:, c.tap_off:c.tap_off + c.H] = want["h"]
        R.assert_bits(f"{c.id} h_out2", wide, img)


# ---------------------------------------------------------------- dfl_pack_rows
@pytest.mark.parametrize("c", R.pack_rows_cases(), ids=lambda c: c.id)
def test_pack_rows(ops, c):
    x = torch.full((16, c.ldx), NAN, dtype=BF16)
    x[:, :c.K] = R.unit((16, c.K), R.gen(c.K + c.rows))
    xd = x.to(dev())
    frag = nans(16 * c.K)
    dyn = None if c.nv is None else record({6: c.nv})
    ops.pack_rows(xd[:, :c.K], c.rows, frag, dyn, 6)
    n = c.rows if c.nv is None else min(c.rows, c.nv)
    want = torch.zeros(16, c.K, dtype=BF16)
    want[:n] = x[:n, :c.K]
    R.assert_bits(c.id, H.unfrag(frag, c.K), want)


# ---------------------------------------------------------------- dfl_qknorm_rope_append
@pytest.mark.parametrize("c", R.append_cases(), ids=lambda c: c.id)
def test_qknorm_rope_append(ops, c):
    inp = R.append_inputs(c)
    want = R.append_ref(c, inp)
    assert c.pos0 != c.S and c.tau <= 16 and c.bs <= 16
    cos, sin = g_(inp.cos), g_(inp.sin)
    assert cos.shape[0] >= c.max_pos and c.cache_rows <= c.cache_alloc and (c.n_kv == 1 or c.cache_rows == c.cache_alloc)
    kc, vc = nans(c.n_kv, c.cache_alloc, 128), nans(c.n_kv, c.cache_alloc, 128)
    q_out = nans(c.n_q, 16, 128) if c.q_col >= 0 else None
    dyn = record({0: c.S, 1: c.tau, 2: c.bs, 3: c.pos0, 4: c.pos0 + c.tau})
    # max_pos = the tables' rows, cache_rows = the caches' rows as the wrapper passes them: leading views are the
    # shorter table (NaN rows behind it) and, with one kv head, the shorter cache (sentinel rows behind it)
    ops.qknorm_rope_append(qkv=g_(inp.part), nsplit=c.nsplit, split_stride=c.split_stride, ld=c.ld, q_col=c.q_col, k_col=c.k_col,
                           v_col=c.v_col, ctx_row0=c.ctx_row0, blk_row0=c.blk_row0, n_q=c.n_q, n_kv=c.n_kv, q_norm_w=g_(inp.qw),
                           k_norm_w=g_(inp.kw), eps=c.eps, cos_tab=cos[:c.max_pos], sin_tab=sin[:c.max_pos], q_out=q_out,
                           kcache=kc[:, :c.cache_rows], vcache=vc[:, :c.cache_rows], dyn=dyn, ctx_rows_override=c.ovr,
                           row_base=c.row_base)
    torch.cuda.synchronize()
    R.check_append(c.id, {"q": q_out, "k": kc, "v": vc}, want, c.norm)
    written = ~torch.isnan(want["v"])
    assert torch.isfinite(kc.cpu()[written].float()).all(), "a NaN table row behind max_pos was used"


# ---------------------------------------------------------------- dfl_prefill_norm_pack
@pytest.mark.parametrize("c", R.prefill_norm_cases(), ids=lambda c: c.id)
def test_prefill_norm_pack(ops, c):
    inp = R.prefill_norm_inputs(c)
    Pp = ops.prefill_rows_padded(c.P)
    want = R.prefill_norm_ref(c, inp, Pp)
    xf = nans(Pp * c.H + 256)
    ops.prefill_norm_pack(g_(inp.rows), c.P, c.H, g_(inp.w), c.eps, xf)
    torch.cuda.synchronize()
    got = H.unpack_tiles(xf[:Pp * c.H], Pp, c.H)
    (R.assert_normed if c.norm else R.assert_bits)(c.id, got, want)
    R.assert_bits(f"{c.id} padded tiles", got[c.P:], torch.zeros(Pp - c.P, c.H, dtype=BF16))
    R.assert_bits(f"{c.id} behind the padded rows", xf[Pp * c.H:], torch.full((256,), NAN, dtype=BF16))


def test_prefill_norm_pack_refuses_wide_rows(ops):
    """H = 8224 > 8192: DFL_EINVAL (-22), nothing launched."""
    from dflash_amd._lib import lib
    P, Hd = 3, 8224
    rows = torch.ones(P, Hd, dtype=BF16, device=dev())
    w = torch.ones(Hd, dtype=BF16, device=dev())
    xf = nans(ops.prefill_rows_padded(P) * Hd)
    rc = lib().dfl_prefill_norm_pack(rows.data_ptr(), Hd, P, Hd, w.data_ptr(), 1e-6, xf.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -22
    assert bool(torch.isnan(xf.float()).all())
    with pytest.raises(RuntimeError):
        ops.prefill_norm_pack(rows, P, Hd, w, 1e-6, xf)


# ---------------------------------------------------------------- dfl_prefill_qk_rope
@pytest.mark.parametrize("c", R.prefill_rope_cases(), ids=lambda c: c.id)
def test_prefill_qk_rope(ops, c):
    inp = R.prefill_rope_inputs(c)
    want = R.prefill_rope_ref(c, inp)
    assert c.pos0 != c.row0 and c.row0 + c.P <= c.cache_rows
    cos, sin = g_(inp.cos), g_(inp.sin)
    assert cos.shape[0] >= c.max_pos
    buf = g_(inp.rows)
    kc, vc = nans(c.n_kv, c.cache_rows, 128), nans(c.n_kv, c.cache_rows, 128)
    ops.prefill_qk_rope(buf, c.P, c.q_col, c.k_col, c.v_col, c.n_q, c.n_kv, g_(inp.qw), g_(inp.kw), c.eps, cos[:c.max_pos],
                        sin[:c.max_pos], c.pos0, kc, vc, c.row0)
    torch.cuda.synchronize()
    R.check_prefill_rope(c.id, {"rows": buf, "k": kc, "v": vc}, want, c)
    written = ~torch.isnan(want["v"])
    assert torch.isfinite(kc.cpu()[written].float()).all(), "a NaN table row behind max_pos was used"
