"""The row stages between the GEMMs, restated plainly in torch fp64 on the CPU, with the rounding points
include/dflash_hip.h and the kernel comments state (csrc/rows.hip, csrc/prefill.hip).  Nothing here needs a GPU.

Row stage (dfl_norm_pack, dfl_norm_frag_batch, dfl_prefill_norm_pack, the mode-2 row source):
    v    = bf16(fp32 sum of the parts in order k = 0, 1, .., starting from 0.0f)
    h    = bf16(resid_or_embed + v)                      (or v / the row alone)
    frag = bf16(w * bf16(h * rstd)),  rstd = rsqrt(mean(h^2) + eps) in fp64
Head stage (every per-head norm + RoPE + cache append site):
    x    = bf16(sum of the parts), or the finished bf16 row
    n    = bf16(w * bf16(x * rstd)) over the head's 128 values (optional)
    out  = bf16(bf16(n * cos) + bf16(rotate_half(n) * sin))     -- torch bf16 elementwise ops
    RoPE position pos0 + rel (clamped to max_pos - 1), cache row S + rel (dropped at >= cache_rows)
Everything but rstd is bit-reproducible: a product of two bf16 values and the fixed-order fp32 part sum are exact
(or identically rounded) in fp32.  rstd is fp64 here and fp32 (another summation order, the hardware's rsqrt) in the
kernels: it may flip bf16(h * rstd) at a rounding boundary, hence the two bars below.

FAULTS make the reference wrong in one way each; test_rows_cpu.py shows that every one of them fails the very helper
the GPU tests call on the very inputs they use, and that the two eps faults pass on unit-scale rows (the blind spot
the older tests had)."""
from __future__ import annotations

import functools
import os
from types import SimpleNamespace as NS

import numpy as np
import torch

import helpers as H
from attn_keys_ref import bf16_steps

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
SHARE_BAR = 2e-3                     # share of elements that may differ at all (same_but_for_rare_ulps, test_hip_prefill)
STEP_BAR = 2                         # bf16 steps: one flip of bf16(h * rstd), one more rounding behind the weight
ROPE_MAX_REL, ROPE_MEAN_REL = 4e-3, 1e-5

FAULTS = ("eps_dropped", "eps_fixed_1e-6", "pos_from_S", "row_from_pos0", "pos_plus_one", "rotate_sign",
          "weight_before_rounding", "sum_unrounded", "row_off_ignored", "row_base_ignored", "dyn_tau_over_override")


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------- comparison helpers
def _measure(name: str, got: torch.Tensor, ref: torch.Tensor, cls: str, log: bool) -> dict:
    """NaN in `ref` marks sentinel elements a launch must leave alone (bit for bit); everything else is measured."""
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    assert got.dtype == BF16 and ref.dtype == BF16 and got.shape == ref.shape, (name, got.dtype, tuple(got.shape), tuple(ref.shape))
    gi, ri = got.view(torch.int16), ref.view(torch.int16)
    sent = torch.isnan(ref.float())
    rec = dict(what=name, cls=cls, sentinel_ok=bool(torch.equal(gi[sent], ri[sent])), n=int((~sent).sum()), share=0.0,
               steps=0, max_rel=0.0, mean_rel=0.0, scale=0.0)
    if rec["n"]:
        g, r = got[~sent], ref[~sent]
        d = (g.float() - r.float()).abs()
        scale = float(r.float().abs().max())
        rec.update(share=float((gi[~sent] != ri[~sent]).float().mean()), steps=int(bf16_steps(g, r).max()), scale=scale,
                   max_rel=float(d.max()) / max(scale, 1e-30), mean_rel=float(d.mean()) / max(scale, 1e-30))
    if log:
        print(f"[parity] {name} ({cls}): {rec['share']:.3e} of {rec['n']} differ, worst {rec['steps']} bf16 steps, "
              f"max {rec['max_rel']:.3e} mean {rec['mean_rel']:.3e} of scale {rec['scale']:.3g}")
        H._log_parity({"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], **rec})
    assert rec["sentinel_ok"], f"{name}: elements the launch must not write were written (or valid ones were not)"
    return rec


def assert_bits(name: str, got: torch.Tensor, ref: torch.Tensor, log: bool = True) -> dict:
    """Bit equality on the int16 views; NaN sentinels compare equal to themselves."""
    rec = _measure(name, got, ref, "bits", log)
    assert rec["share"] == 0.0, f"{name}: {rec['share']:.3e} of the elements differ (worst {rec['steps']} bf16 steps)"
    return rec


def assert_normed(name: str, got: torch.Tensor, ref: torch.Tensor, log: bool = True) -> dict:
    """Norm, no RoPE: every element within STEP_BAR bf16 steps, fewer than SHARE_BAR of them different at all."""
    rec = _measure(name, got, ref, "normed", log)
    assert rec["steps"] <= STEP_BAR, f"{name}: {rec['steps']} bf16 steps from the reference (bar {STEP_BAR})"
    assert rec["share"] < SHARE_BAR, f"{name}: {rec['share']:.3e} of the elements differ (bar {SHARE_BAR:.0e})"
    return rec


def assert_roped(name: str, got: torch.Tensor, ref: torch.Tensor, log: bool = True) -> dict:
    """Norm + RoPE: the same share, and max / mean error of scale as test_prefill_norm_and_rope_match_the_oracle."""
    rec = _measure(name, got, ref, "roped", log)
    assert rec["share"] < SHARE_BAR, f"{name}: {rec['share']:.3e} of the elements differ (bar {SHARE_BAR:.0e})"
    if rec["n"]:
        sent = torch.isnan(ref.detach().float().cpu())
        g, r = got.detach().cpu()[~sent], ref.detach().cpu()[~sent]
        if log:
            H.assert_close(name, g, r, max_rel=ROPE_MAX_REL, mean_rel=ROPE_MEAN_REL)
        assert rec["max_rel"] <= ROPE_MAX_REL, f"{name}: max-abs error {rec['max_rel']:.3e} of scale exceeds {ROPE_MAX_REL:.1e}"
        assert rec["mean_rel"] <= ROPE_MEAN_REL, f"{name}: mean-abs error {rec['mean_rel']:.3e} of scale exceeds {ROPE_MEAN_REL:.1e}"
    return rec


# ---------------------------------------------------------------- the two operations
def part_sum(parts: torch.Tensor) -> torch.Tensor:
    """fp32 sum of parts[k] in order k = 0, 1, .., starting from 0.0f (not yet rounded)."""
    v = torch.zeros_like(parts[0], dtype=F32)
    for k in range(parts.shape[0]):
        v = v + parts[k].float()
    return v


def rms(h: torch.Tensor, w: torch.Tensor, eps: float, fault: str = "") -> torch.Tensor:
    """bf16(w * bf16(h * rstd)) over the last axis, rstd in fp64.  h: bf16 (or, for a fault, the unrounded fp32 row)."""
    h64 = h.double()
    e = 0.0 if fault == "eps_dropped" else 1e-6 if fault == "eps_fixed_1e-6" else float(eps)
    rstd = torch.rsqrt((h64 * h64).mean(-1, keepdim=True) + e)
    if fault == "weight_before_rounding":
        return (w.double() * h64 * rstd).to(BF16)
    return (w.double() * (h64 * rstd).to(BF16).double()).to(BF16)


def rotate_half(x: torch.Tensor) -> torch.Tensor:
    return torch.cat((-x[..., 64:], x[..., :64]), dim=-1)


def rope(x: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, max_pos: int, fault: str = "") -> torch.Tensor:
    """x bf16 [n, heads, 128], pos int64 [n]; cos / sin bf16 [>= max_pos, 64].  bf16 elementwise ops, as torch rounds them."""
    if fault == "pos_plus_one":
        pos = pos + 1
    p = pos.clamp(max=max_pos - 1)
    c = torch.cat([cos[p], cos[p]], -1)[:, None, :]
    s = torch.cat([sin[p], sin[p]], -1)[:, None, :]
    rh = rotate_half(x)
    if fault == "rotate_sign":
        rh = -rh
    return (x * c) + (rh * s)


def head_stage(x: torch.Tensor, x32, w, eps: float, pos, cos, sin, max_pos: int, fault: str = "") -> torch.Tensor:
    """x bf16 [n, heads, 128] (x32: the unrounded fp32 sums, for the sum_unrounded fault) -> normed, rotated bf16."""
    n = x
    if w is not None:
        n = rms(x32 if (fault == "sum_unrounded" and x32 is not None) else x, w, eps, fault)
    return rope(n, pos, cos, sin, max_pos, fault)


@functools.lru_cache(maxsize=None)
def tables(max_pos: int):
    """The product's own tables (theta 1e6, head_dim 128) on the CPU: bf16 [max_pos, 64] each."""
    from dflash_amd.model import _rope_tables
    return _rope_tables(128, 1e6, max_pos, "cpu")


def tables_nan_behind(max_pos: int, extra: int = 8):
    """[max_pos + extra, 64] tables whose rows behind max_pos hold NaN: the clamp probe never leaves the allocation."""
    cos, sin = tables(max_pos)
    pad = torch.full((extra, 64), NAN, dtype=BF16)
    return torch.cat([cos, pad]), torch.cat([sin, pad])


# ---------------------------------------------------------------- input builders
def unit(shape, g, dtype=BF16) -> torch.Tensor:
    return torch.randn(*shape, generator=g, dtype=F32).to(dtype)


def bounded(shape, g) -> torch.Tensor:
    """+-[0.5, 1.5) uniformly: mean square ~1.08 for every row length, however short."""
    mag = 0.5 + torch.rand(*shape, generator=g, dtype=F32)
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return mag * sign


def small_scale(eps: float) -> float:
    """Small rows: unit-scale data times 2^-10 for eps = 1e-6, 2^-8 for eps = 1e-5 (exact in bf16)."""
    return {1e-6: 2.0 ** -10, 1e-5: 2.0 ** -8}[eps]


def assert_small(x: torch.Tensor, eps: float, what: str = "") -> None:
    """Every row's (head's) mean square lies within a factor 4 of eps: eps then moves rstd by tens of percent."""
    ms = (x.double() ** 2).mean(-1)
    assert ms.numel() == 0 or (float(ms.min()) >= eps / 4 and float(ms.max()) <= eps * 4), (what, float(ms.min()), float(ms.max()), eps)


def norm_weight(n: int, g) -> torch.Tensor:
    return (1 + 0.1 * torch.randn(n, generator=g)).to(BF16)


def head_norm_weight(g) -> torch.Tensor:
    """1 + 0.1 randn with every 32nd dimension doubled (real q/k norm weights spread more than that).  The max-abs bar
    of assert_roped is 4e-3 of the reference's largest value, and ONE bf16 step in the top binade of that value is
    2^-8 .. 2^-7 of it: a single legitimate flip there would miss the bar.  With all weights near 1 the top binade of a
    normed head tensor holds several percent of its elements; with a few larger weights it holds about 0.1 %, so the
    bar measures what it is meant to (flips below the top binade are <= 2^-8 of scale)."""
    w = 1 + 0.1 * torch.randn(128, generator=g)
    w[::32] *= 2
    return w.to(BF16)


FAMILIES = {"unit": (1e-6, None), "small6": (1e-6, 1e-6), "small5": (1e-5, 1e-5)}   # family -> (eps passed, eps the rows are sized for)


def _amp(family: str) -> float:
    return 1.0 if family == "unit" else small_scale(FAMILIES[family][1])


# ---------------------------------------------------------------- dfl_norm_pack
def norm_pack_kernel(H_: int) -> int:
    """The k_norm_pack<N> form dfl_norm_pack launches: N x 256 chunks of 8 columns per row."""
    chunks = H_ // 8
    return 2 if chunks <= 512 else 4 if chunks <= 1024 else 8


VARIANTS = ("part", "part_resid", "part_embed", "resid", "embed")
OUTS = ("none", "h_out", "inplace", "tap", "inplace_tap")


def _np_case(H_, variant, out, nv, family, nsplit=1, row_off=0, seed=0):
    assert variant in VARIANTS and out in OUTS and (out not in ("inplace", "inplace_tap") or "resid" in variant)
    c = NS(H=H_, variant=variant, out=out, nv=nv, family=family, eps=FAMILIES[family][0], nsplit=nsplit, row_off=row_off,
           ldp=H_ + 12, ld2=H_ + 40, tap_off=16, dyn_word=2 if nv in (None, 11) else 5, seed=seed)
    c.part_split = 32 * c.ldp + 20
    nvs = "dynNULL" if nv is None else f"nv{nv}"
    c.id = f"k{norm_pack_kernel(H_)}-H{H_}-{variant}-ns{nsplit}-off{row_off}-{out}-{nvs}-{family}"
    return c


def norm_pack_cases() -> list:
    C = _np_case
    cases = [
        C(8, "part_resid", "h_out", None, "unit"), C(8, "resid", "none", 11, "small6"),
        C(4096, "part_resid", "inplace_tap", 11, "small5", nsplit=3, row_off=16), C(4096, "embed", "h_out", 16, "unit"),
        C(4104, "part_resid", "tap", 1, "small6"), C(4104, "part", "none", 0, "unit", nsplit=3),
        C(8192, "part_resid", "h_out", 16, "small5", nsplit=3, row_off=16), C(8192, "resid", "inplace_tap", 11, "small6"),
        C(8200, "part_resid", "inplace", 11, "small6"), C(8200, "embed", "tap", None, "unit"),
        C(16384, "part_resid", "inplace_tap", 11, "small5", nsplit=3, row_off=16), C(16384, "part", "none", 1, "unit"),
    ]
    for H_, fams in ((1024, ("small6", "small5", "unit", "small5", "small6")), (5120, ("small5", "small6", "small5", "unit", "small5"))):
        cases += [C(H_, "part", "h_out", 11, fams[0], nsplit=3, row_off=16), C(H_, "part_resid", "inplace_tap", 16, fams[1], nsplit=3),
                  C(H_, "part_embed", "tap", 11, fams[2], row_off=16), C(H_, "resid", "inplace", None, fams[3]),
                  C(H_, "embed", "h_out", 1, fams[4])]
    for i, c in enumerate(cases):
        c.seed = 100 + i
    return cases


def norm_pack_inputs(c) -> NS:
    """part: the flat fp32 buffer [nsplit][32 rows][ldp] (+ slack between the splits), NaN in every pad element."""
    g = gen(c.seed)
    a = _amp(c.family)
    both = c.variant in ("part_resid", "part_embed")
    inp = NS(part=None, resid=None, embed=None, ids=None, w=norm_weight(c.H, g))
    if "part" in c.variant:
        buf = torch.full((c.nsplit * c.part_split,), NAN, dtype=F32)
        view = buf.as_strided((c.nsplit, 32, c.H), (c.part_split, c.ldp, 1))
        view.copy_(bounded((c.nsplit, 32, c.H), g) * (a * (0.7 if both else 1.0) / c.nsplit ** 0.5))
        inp.part, inp.part_view = buf, view
    if "resid" in c.variant:
        inp.resid = (bounded((16, c.H), g) * (0.7 if both else 1.0)).to(BF16) * a
    if "embed" in c.variant:
        inp.embed = (bounded((23, c.H), g) * (0.7 if both else 1.0)).to(BF16) * a
        inp.ids = torch.randint(0, 23, (16,), generator=g)
    if c.family != "unit":
        assert_small(norm_pack_ref(c, inp)["h_all"], FAMILIES[c.family][1], c.id)
    return inp


def norm_pack_ref(c, inp, fault: str = "") -> dict:
    """Images of what a launch leaves: h [16, H] (NaN sentinel in rows >= n_valid) and frag [16, H] (zero rows there)."""
    nv = 16 if c.nv is None else c.nv
    src = inp.embed[inp.ids] if inp.embed is not None else inp.resid
    v32 = None
    if inp.part is not None:
        off = 0 if fault == "row_off_ignored" else c.row_off
        v32 = part_sum(inp.part_view[:, off:off + 16])
    if v32 is None:
        h = src
    elif src is None:
        h = v32.to(BF16)
    elif fault == "sum_unrounded":
        h = (src.float() + v32).to(BF16)
    else:
        h = src + v32.to(BF16)
    frag = rms(h, inp.w, c.eps, fault)
    h_img = torch.full((16, c.H), NAN, dtype=BF16)
    h_img[:nv] = h[:nv]
    f_img = torch.zeros(16, c.H, dtype=BF16)
    f_img[:nv] = frag[:nv]
    return dict(h=h_img, frag=f_img, h_all=h[:nv])


def norm_pack_faults(c) -> list:
    f = ["weight_before_rounding"]
    if c.family != "unit":
        f.append("eps_dropped")
    if c.family == "small5":
        f.append("eps_fixed_1e-6")                  # (at eps = 1e-6 this fault IS the truth)
    if c.variant in ("part_resid", "part_embed"):
        f.append("sum_unrounded")
    if "part" in c.variant and c.row_off:
        f.append("row_off_ignored")
    return f if (c.nv is None or c.nv > 0) else []


def check_norm_pack(name: str, got: dict, want: dict, log: bool = True) -> list:
    """got / want: {"h": [16, H] or None, "frag": [16, H]} images."""
    recs = []
    if got.get("h") is not None:
        recs.append(assert_bits(f"{name} h", got["h"], want["h"], log))
    recs.append(assert_normed(f"{name} frag", got["frag"], want["frag"], log))
    return recs


# ---------------------------------------------------------------- dfl_qknorm_rope_append
TABLE_ROWS = 40960


def _ap_case(heads, form, nsplit, family, norm=True, S=40, tau=5, bs=12, pos0=1040, ovr=-1, row_base=0, max_pos=TABLE_ROWS,
             cache_rows=None, cache_alloc=None, swap_rows=False, tag=""):
    n_q, n_kv = heads
    c = NS(n_q=n_q, n_kv=n_kv, form=form, nsplit=nsplit, family=family, eps=FAMILIES[family][0], norm=norm, S=S, tau=tau, bs=bs,
           pos0=pos0, ovr=ovr, row_base=row_base, max_pos=max_pos)
    # k | gap | q | gap | v inside rows wider than q|k|v; the splits further apart than rows x ld
    c.k_col = 8
    c.q_col = c.k_col + n_kv * 128 + 24
    c.v_col = c.q_col + n_q * 128 + 8
    c.ld = c.v_col + n_kv * 128 + 16
    c.split_stride = 32 * c.ld + 40
    c.ctx_row0, c.blk_row0 = (16, 0) if swap_rows else (0, 16)
    if form in ("kv_ctx", "override"):
        c.q_col, c.blk_row0 = -1, -1
    n_new = (ovr + row_base) if ovr >= 0 else tau + bs
    c.cache_alloc = cache_alloc or S + n_new + 7
    c.cache_rows = cache_rows or c.cache_alloc
    c.id = (f"{form}-h{n_q}x{n_kv}-ns{nsplit}-{'norm' if norm else 'nonorm'}-{family}-S{S}-pos{pos0}"
            + (f"-ovr{ovr}-base{row_base}" if ovr >= 0 else "") + (f"-{tag}" if tag else ""))
    return c


def append_cases() -> list:
    C = _ap_case
    cases = [
        C((4, 2), "ctx_blk", 2, "small6"), C((4, 2), "ctx_blk", 1, "unit", norm=False, swap_rows=True),
        C((8, 1), "ctx_blk", 3, "small5", pos0=40000 - 3), C((32, 8), "ctx_blk", 2, "small5", S=301, pos0=17),
        C((4, 2), "blk_only", 3, "small5", tau=0), C((8, 1), "blk_only", 1, "small6", tau=0, bs=16, pos0=40000),
        C((32, 8), "blk_only", 2, "unit", tau=0, bs=1, norm=False),
        C((4, 2), "kv_ctx", 2, "small5", tau=16, bs=12), C((32, 8), "kv_ctx", 1, "small6", tau=9, bs=3, pos0=40000),
        C((8, 1), "kv_ctx", 3, "unit", tau=1, bs=0, norm=False),
        C((4, 2), "override", 2, "small5", tau=3, bs=7, ovr=16, row_base=0), C((4, 2), "override", 1, "small6", tau=7, bs=12, ovr=9, row_base=16),
        C((32, 8), "override", 2, "small5", tau=3, bs=7, ovr=16, row_base=48, pos0=40000 - 60),
        C((8, 1), "override", 3, "unit", tau=12, bs=5, ovr=9, row_base=48, norm=False),
        # the two edges: positions run over max_pos (the table rows behind hold NaN); cache rows run over cache_rows
        C((4, 2), "ctx_blk", 2, "small5", pos0=1040, max_pos=1048, tag="clamp"),
        C((8, 1), "ctx_blk", 2, "small5", cache_rows=40 + 9, cache_alloc=40 + 24, tag="cachelimit"),
        C((8, 1), "override", 1, "small6", tau=3, bs=7, ovr=16, row_base=16, cache_rows=40 + 20, cache_alloc=40 + 40, tag="cachelimit"),
    ]
    for i, c in enumerate(cases):
        c.seed = 200 + i
    return cases


def append_inputs(c) -> NS:
    g = gen(c.seed)
    a = _amp(c.family)
    buf = torch.full((c.nsplit * c.split_stride,), NAN, dtype=F32)
    view = buf.as_strided((c.nsplit, 32, c.ld), (c.split_stride, c.ld, 1))
    cols = [(c.k_col, c.n_kv * 128), (c.v_col, c.n_kv * 128)] + ([(c.q_col, c.n_q * 128)] if c.q_col >= 0 else [])
    for c0, wd in cols:                                            # gap columns stay NaN: reading one shows
        view[:, :, c0:c0 + wd] = unit((c.nsplit, 32, wd), g, F32) * (a / c.nsplit ** 0.5)
    inp = NS(part=buf, part_view=view, qw=head_norm_weight(g) if c.norm else None, kw=head_norm_weight(g) if c.norm else None)
    inp.cos, inp.sin = tables_nan_behind(c.max_pos) if c.max_pos < TABLE_ROWS else tables(c.max_pos)
    if c.family != "unit":
        x = part_sum(view).to(BF16)
        for c0, wd in cols:
            assert_small(x[:, c0:c0 + wd].reshape(32, -1, 128), FAMILIES[c.family][1], c.id)
    return inp


def append_ref(c, inp, fault: str = "") -> dict:
    """Images: q [n_q, 16, 128], k / v [n_kv, cache_alloc, 128]; NaN wherever the launch must not write."""
    tau, bs = c.tau, c.bs
    if c.ovr >= 0 and fault != "dyn_tau_over_override":
        tau, bs = c.ovr, 0
    if c.blk_row0 < 0:
        bs = 0
    tau = min(tau, 16)
    rb = 0 if fault == "row_base_ignored" else c.row_base
    x32 = part_sum(inp.part_view)
    xb = x32.to(BF16)
    rel = torch.cat([rb + torch.arange(tau), tau + torch.arange(bs)])
    brow = torch.cat([c.ctx_row0 + torch.arange(tau), c.blk_row0 + torch.arange(bs)])
    pos = (c.S if fault == "pos_from_S" else c.pos0) + rel
    crow = (c.pos0 if fault == "row_from_pos0" else c.S) + rel
    n = rel.numel()

    def heads(t, col, nh, rows):
        return t[rows, col:col + nh * 128].reshape(rows.numel(), nh, 128)

    out = dict(q=torch.full((c.n_q, 16, 128), NAN, dtype=BF16), k=torch.full((c.n_kv, c.cache_alloc, 128), NAN, dtype=BF16),
               v=torch.full((c.n_kv, c.cache_alloc, 128), NAN, dtype=BF16))
    if n:
        ke = head_stage(heads(xb, c.k_col, c.n_kv, brow), heads(x32, c.k_col, c.n_kv, brow), inp.kw, c.eps, pos, inp.cos, inp.sin,
                        c.max_pos, fault)
        keep = crow < c.cache_rows
        out["k"][:, crow[keep]] = ke[keep].transpose(0, 1)
        out["v"][:, crow[keep]] = heads(xb, c.v_col, c.n_kv, brow)[keep].transpose(0, 1)
    if c.q_col >= 0 and bs:
        qe = head_stage(heads(xb, c.q_col, c.n_q, brow[tau:]), heads(x32, c.q_col, c.n_q, brow[tau:]), inp.qw, c.eps, pos[tau:],
                        inp.cos, inp.sin, c.max_pos, fault)
        out["q"][:, :bs] = qe.transpose(0, 1)
    return out


def append_faults(c) -> list:
    f = ["pos_plus_one", "rotate_sign"]
    if c.pos0 != c.S:
        f += ["pos_from_S", "row_from_pos0"]
    if c.norm:
        f += ["weight_before_rounding", "sum_unrounded"]
        if c.family != "unit":
            f.append("eps_dropped")
        if c.family == "small5":
            f.append("eps_fixed_1e-6")
    if c.ovr >= 0:
        f.append("dyn_tau_over_override")
        if c.row_base:
            f.append("row_base_ignored")
    return f


def check_append(name: str, got: dict, want: dict, normed: bool, log: bool = True) -> list:
    """got / want: {"q" (or None), "k", "v"} images.  V bit-equal always; q and K bit-equal without norm weights."""
    recs = [assert_bits(f"{name} V", got["v"], want["v"], log)]
    cmp = assert_roped if normed else assert_bits
    recs.append(cmp(f"{name} K", got["k"], want["k"], log))
    if got.get("q") is not None:
        recs.append(cmp(f"{name} q", got["q"], want["q"], log))
    return recs


# ---------------------------------------------------------------- dfl_pack_rows
def pack_rows_cases() -> list:
    cases = []
    for K, rows, nv in ((8, 16, None), (8, 1, 0), (4096, 16, 11), (4096, 0, None), (4096, 1, None), (25600, 16, None),
                        (25600, 16, 1), (25600, 1, 0)):
        cases.append(NS(K=K, rows=rows, nv=nv, ldx=K + 24, id=f"K{K}-rows{rows}-" + ("dynNULL" if nv is None else f"nv{nv}")))
    return cases


# ---------------------------------------------------------------- dfl_prefill_norm_pack
def prefill_norm_cases() -> list:
    cases = []
    for H_, P, family, norm in ((32, 1, "small6", True), (32, 17, "unit", False), (32, 300, "small5", True), (4096, 16, "small5", True),
                                (4096, 129, "unit", True), (5120, 127, "small6", True), (5120, 128, "unit", False),
                                (8192, 17, "small5", True), (8192, 300, "small6", True)):
        c = NS(H=H_, P=P, family=family, norm=norm, eps=FAMILIES[family][0], ldh=H_ + 24, seed=300 + len(cases))
        c.id = f"H{H_}-P{P}-{'norm' if norm else 'packonly'}-{family}"
        cases.append(c)
    return cases


def prefill_norm_inputs(c) -> NS:
    g = gen(c.seed)
    rows = torch.full((c.P, c.ldh), NAN, dtype=BF16)
    rows[:, :c.H] = bounded((c.P, c.H), g).to(BF16) * _amp(c.family)
    if c.family != "unit":
        assert_small(rows[:, :c.H], FAMILIES[c.family][1], c.id)
    return NS(rows=rows, w=norm_weight(c.H, g) if c.norm else None)


def prefill_norm_ref(c, inp, Pp: int, fault: str = "") -> torch.Tensor:
    """[Pp, H]: the P rows (normed, or as they are) and zero rows behind them."""
    h = inp.rows[:, :c.H]
    out = torch.zeros(Pp, c.H, dtype=BF16)
    out[:c.P] = rms(h, inp.w, c.eps, fault) if c.norm else h
    return out


def prefill_norm_faults(c) -> list:
    if not c.norm:
        return []
    return ["weight_before_rounding"] + (["eps_dropped"] if c.family != "unit" else []) + (["eps_fixed_1e-6"] if c.family == "small5" else [])


# ---------------------------------------------------------------- dfl_prefill_qk_rope
def _pq_case(P, heads, family, norm, pos0, row0, max_pos=TABLE_ROWS, tag=""):
    n_q, n_kv = heads
    c = NS(P=P, n_q=n_q, n_kv=n_kv, family=family, norm=norm, eps=FAMILIES[family][0], pos0=pos0, row0=row0, max_pos=max_pos)
    c.v_col = 8
    c.q_col = c.v_col + n_kv * 128 + 16
    c.k_col = c.q_col + n_q * 128 + 8
    c.ld = c.k_col + n_kv * 128 + 24
    c.cache_rows = row0 + P + 5
    c.id = f"P{P}-h{n_q}x{n_kv}-{'norm' if norm else 'nonorm'}-{family}-pos{pos0}-row{row0}" + (f"-{tag}" if tag else "")
    return c


def prefill_rope_cases() -> list:
    C = _pq_case
    cases = [C(1, (4, 2), "small6", True, 5, 9), C(3, (32, 8), "small5", True, 40000, 2), C(77, (4, 2), "small5", True, 40000, 9),
             C(77, (2, 1), "unit", False, 5, 0), C(300, (2, 1), "small6", True, 5, 9), C(300, (0, 2), "small5", True, 40000, 3),
             C(3, (0, 2), "unit", False, 5, 9), C(77, (32, 8), "unit", True, 5, 9),
             C(77, (4, 2), "small5", True, 1000, 9, max_pos=1048, tag="clamp")]
    for i, c in enumerate(cases):
        c.seed = 400 + i
    return cases


def prefill_rope_inputs(c) -> NS:
    g = gen(c.seed)
    rows = unit((c.P, c.ld), g) * _amp(c.family)         # gap columns hold data too: they must come back unchanged
    inp = NS(rows=rows, qw=head_norm_weight(g) if c.norm else None, kw=head_norm_weight(g) if c.norm else None)
    inp.cos, inp.sin = tables_nan_behind(c.max_pos) if c.max_pos < TABLE_ROWS else tables(c.max_pos)
    if c.family != "unit":
        for c0, nh in ((c.q_col, c.n_q), (c.k_col, c.n_kv)):
            assert_small(rows[:, c0:c0 + nh * 128].reshape(c.P, nh, 128), FAMILIES[c.family][1], c.id)
    return inp


def prefill_rope_ref(c, inp, fault: str = "") -> dict:
    """rows: the row buffer afterwards (q rewritten in place, everything else as it was); k / v: cache images."""
    r = torch.arange(c.P)
    pos = (c.row0 if fault == "pos_from_S" else c.pos0) + r
    crow = (c.pos0 if fault == "row_from_pos0" else c.row0) + r
    x = inp.rows
    out = dict(rows=x.clone(), k=torch.full((c.n_kv, c.cache_rows, 128), NAN, dtype=BF16),
               v=torch.full((c.n_kv, c.cache_rows, 128), NAN, dtype=BF16))
    k = x[:, c.k_col:c.k_col + c.n_kv * 128].reshape(c.P, c.n_kv, 128)
    keep = crow < c.cache_rows
    out["k"][:, crow[keep]] = head_stage(k, None, inp.kw, c.eps, pos, inp.cos, inp.sin, c.max_pos, fault)[keep].transpose(0, 1)
    out["v"][:, crow[keep]] = x[:, c.v_col:c.v_col + c.n_kv * 128].reshape(c.P, c.n_kv, 128)[keep].transpose(0, 1)
    if c.n_q:
        q = x[:, c.q_col:c.q_col + c.n_q * 128].reshape(c.P, c.n_q, 128)
        out["rows"][:, c.q_col:c.q_col + c.n_q * 128] = head_stage(q, None, inp.qw, c.eps, pos, inp.cos, inp.sin, c.max_pos,
                                                                   fault).reshape(c.P, -1)
    return out


def prefill_rope_faults(c) -> list:
    f = ["pos_plus_one", "rotate_sign"]
    if c.pos0 != c.row0:
        f += ["pos_from_S", "row_from_pos0"]
    if c.norm:
        f.append("weight_before_rounding")
        if c.family != "unit":
            f.append("eps_dropped")
        if c.family == "small5":
            f.append("eps_fixed_1e-6")
    return f


def check_prefill_rope(name: str, got: dict, want: dict, c, log: bool = True) -> list:
    """got / want: {"rows", "k", "v"}.  V, and every column of the row buffer but q's, bit-equal."""
    recs = [assert_bits(f"{name} V", got["v"], want["v"], log)]
    cmp = assert_roped if c.norm else assert_bits
    recs.append(cmp(f"{name} K", got["k"], want["k"], log))
    qs = slice(c.q_col, c.q_col + c.n_q * 128)
    g, w = got["rows"].detach().cpu().clone(), want["rows"].clone()
    if c.n_q:
        recs.append(cmp(f"{name} q", got["rows"].detach().cpu()[:, qs], want["rows"][:, qs], log))
        g[:, qs] = 0
        w[:, qs] = 0
    recs.append(assert_bits(f"{name} other columns", g, w, log))
    return recs


# ---------------------------------------------------------------- an fp32 model of the kernels' norm (headroom of the bars)
def rms_fp32_model(h: torch.Tensor, w: torch.Tensor, eps: float, ulp: int = 0) -> torch.Tensor:
    """What a kernel computes: fp32 squares summed in ANOTHER order (64 strided lanes, then a tree), an fp32 rsqrt moved
    by `ulp` fp32 steps (the hardware's is within 1 ulp), an fp32 product rounded to bf16, times w, rounded again."""
    x = h.float().numpy().astype(np.float32)
    n = x.shape[-1]
    pad = (-n) % 64
    sq = np.pad(x * x, [(0, 0)] * (x.ndim - 1) + [(0, pad)]).reshape(*x.shape[:-1], -1, 64)
    lanes = np.zeros(sq.shape[:-2] + (64,), dtype=np.float32)
    for i in range(sq.shape[-2]):
        lanes = (lanes + sq[..., i, :]).astype(np.float32)
    while lanes.shape[-1] > 1:
        half = lanes.shape[-1] // 2
        lanes = (lanes[..., :half] + lanes[..., half:]).astype(np.float32)
    ms = (lanes / np.float32(n) + np.float32(eps)).astype(np.float32)
    rstd = (np.float32(1) / np.sqrt(ms.astype(np.float64))).astype(np.float32)
    for _ in range(abs(ulp)):
        rstd = np.nextafter(rstd, np.float32(np.inf if ulp > 0 else -np.inf)).astype(np.float32)
    y = torch.from_numpy((x * rstd).astype(np.float32)).to(BF16)
    return (w.float() * y.float()).to(BF16)
