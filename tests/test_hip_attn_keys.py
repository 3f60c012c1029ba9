"""Every attention kernel key by key: the census and needle inputs of attn_keys_ref (exact answers, one mishandled key
moves the output by many bf16 steps) through dfl_block_attn, dfl_attn_fused, dfl_attn_fused_batch, dfl_attn_head with its
_oproj, _cand, _batch and _batch_f32 forms, and dfl_prefill_attn, at the smallest shapes that reach each launch form
(the host rules of csrc/attn_head.hip are mirrored in attn_keys_ref.head_form and named in the test ids).

Each case runs, on ONE workspace (the arrival tickets re-arm between launches): the census with the lane code and with
the tile code, the needle launches, and for causal forms the leak probes.  Where q and the new rows' K come from Linear
rows they are passed with no norm weights and rotation tables of cos = 1, sin = 0, so they reach the kernel unchanged;
the norm and RoPE path stays covered by the randn tests against the oracle (test_hip_kernels.py,
test_hip_batch_kernels.py).  By-products: the appended K / V rows are bit-equal to the Linear rows and every other cache
row is untouched; cache rows past the keys hold NaN wherever the kernel does not write them."""
import dataclasses
import functools
import os
import re

import pytest
import torch

import attn_keys_ref as R
import helpers as H

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NAN = float("nan")


def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _tables(max_pos):
    cos, sin = R.rope_tables_identity(max_pos)
    return cos.to(dev()), sin.to(dev())


@functools.lru_cache(maxsize=8)
def _problem_set(S, tau, bs, causal, n_q, n_kv, prefill=False):
    seed = 7 * S + 3 * tau + bs + n_q
    ps = [R.census_problem(S, tau, bs, causal, n_q, n_kv, code, seed=seed) for code in ("lane", "tile")]
    ps += R.needle_problems(S, tau, bs, causal, n_q, n_kv, seed=seed, prefill=prefill)
    if causal:
        ps.append(R.leak_problem(S, tau, bs, causal, n_q, n_kv, seed=seed, prefill=prefill))
    return tuple(ps)


def _bits(x):
    return x.contiguous().view(torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------- a problem as kernel inputs
def _dims(p):
    qd, kd = p.n_q * 128, p.n_kv * 128
    return qd, kd, qd + 2 * kd


def _block_rows(p, rows=16):
    """The block rows' Linear outputs q | k | v: bf16 [rows, ld] (rows >= bs are zero)."""
    qd, kd, ld = _dims(p)
    x = torch.zeros(rows, ld, dtype=BF16)
    x[:p.bs, :qd] = p.q.reshape(p.bs, qd)
    x[:p.bs, qd:qd + kd] = p.k[:, p.S + p.tau:].transpose(0, 1).reshape(p.bs, kd)
    x[:p.bs, qd + kd:] = p.v[:, p.S + p.tau:].transpose(0, 1).reshape(p.bs, kd)
    return x


def _ctx_rows(p, rows=32):
    """The context rows' Linear outputs (k | v at the same columns as the block rows')."""
    qd, kd, ld = _dims(p)
    x = torch.zeros(rows, ld, dtype=BF16)
    x[:p.tau, qd:qd + kd] = p.k[:, p.S:p.S + p.tau].transpose(0, 1).reshape(p.tau, kd)
    x[:p.tau, qd + kd:] = p.v[:, p.S:p.S + p.tau].transpose(0, 1).reshape(p.tau, kd)
    return x


def _caches(p, rows, upto=None):
    """K / V caches [n_kv, rows, 128]: the first `upto` keys (default: the S cached ones), NaN behind them."""
    upto = p.S if upto is None else upto
    kc = torch.full((p.n_kv, rows, 128), NAN, dtype=BF16)
    vc = torch.full((p.n_kv, rows, 128), NAN, dtype=BF16)
    kc[:, :upto], vc[:, :upto] = p.k[:, :upto], p.v[:, :upto]
    return kc, vc


def _check_caches(p, kc, vc, name):
    """After a launch that appends: keys [0, n_keys) bit-equal to the problem's (cached rows untouched, new rows equal to
    the Linear rows), NaN behind them."""
    kc, vc = kc.cpu(), vc.cpu()
    n = p.n_keys
    assert _same_bits(kc[:, :n], p.k) and _same_bits(vc[:, :n], p.v), f"{name}: cache rows differ"
    assert bool(torch.isnan(kc[:, n:].float()).all()) and bool(torch.isnan(vc[:, n:].float()).all()), f"{name}: rows past the keys written"


class Tally:
    """What a case saw: the worst census distance, the needle rows checked, the worst leak error."""

    def __init__(self, name):
        self.name, self.steps, self.off, self.rows, self.leak, self.launches = name, 0, 0, 0, 0.0, 0

    def check(self, p, out, leak_bar=2.0 ** -6, tag=""):
        name = f"{self.name} {tag}{p.kind} S={p.S} tau={p.tau} bs={p.bs}"
        self.launches += 1
        if p.kind.startswith("census"):
            st = R.check_census(p, out, name)
            self.steps, self.off = max(self.steps, st["worst_steps"]), self.off + st["off"]
        elif p.kind == "needle":
            self.rows += R.check_needle(p, out, name)
        else:
            self.leak = max(self.leak, R.check_leak(p, out, leak_bar, name))

    def report(self):
        print(f"[parity] attn keys {self.name}: {self.launches} launches, census worst {self.steps} bf16 steps "
              f"({self.off} elements off), {self.rows} needle rows bit-exact, leak max {self.leak:.3e} of scale")
        H._log_parity({"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "what": f"attn keys {self.name}",
                       "launches": self.launches, "census_worst_steps": self.steps, "census_off": self.off,
                       "needle_rows": self.rows, "leak_max_rel": self.leak})


def _rows_out(frag, p):
    """frag16 tile(s) [tiles, 16 * qd] -> bf16 [bs, n_q, 128] on the CPU."""
    qd = p.n_q * 128
    return torch.cat([H.unfrag(t, qd) for t in frag.view(-1, 16 * qd)])[:p.bs].reshape(p.bs, p.n_q, 128).cpu()


# ---------------------------------------------------------------- dfl_block_attn
BLOCK_CASES = [(S, causal, ms) for S in (0, 31, 32, 33, 1000) for causal in (False, True) for ms in (32, 2)]


@pytest.mark.parametrize("S,causal,max_splits", BLOCK_CASES,
                         ids=[f"S{S}-{'causal' if c else 'full'}-ms{ms}" for S, c, ms in BLOCK_CASES])
def test_block_attn_keys(S, causal, max_splits):
    """dfl_block_attn, heads (8, 2): q and the whole cache (new rows included) are given directly.  Context rows (tau = 5)
    in the non-causal draft form; 11-row blocks at the odd lengths."""
    from dflash_amd import ops
    n_q, n_kv = 8, 2
    tau, bs = (0 if causal else 5), (16 if S % 32 == 0 or S == 1000 else 11)
    t = Tally(f"block_attn ({n_q},{n_kv}) S{S} tau{tau} bs{bs} {'causal' if causal else 'full'} ms{max_splits}")
    ws = ops.attn_ws(n_q, max_splits, dev())
    dyn = torch.zeros(8, dtype=torch.int32, device=dev())
    ops.set_dyn(dyn, S, tau, bs, S)
    for p in _problem_set(S, tau, bs, causal, n_q, n_kv):
        kc, vc = _caches(p, p.n_keys + 40, upto=p.n_keys)
        q = torch.zeros(n_q, 16, 128, dtype=BF16)
        q[:, :bs] = p.q.transpose(0, 1)
        out = torch.full((16 * n_q * 128,), NAN, dtype=BF16, device=dev())
        ops.block_attn(q=q.to(dev()), kcache=kc.to(dev()), vcache=vc.to(dev()), n_q=n_q, n_kv=n_kv, scale=R.SCALE, dyn=dyn,
                       kv_len_max=p.n_keys, ws=ws, max_splits=max_splits, out_frag=out, causal=causal)
        t.check(p, _rows_out(out, p))
    t.report()


# ---------------------------------------------------------------- dfl_attn_fused
FUSED_CASES = [(1, 1, 40, 3), (2, 1, 41, 0), (4, 1, 39, 16), (8, 1, 40, 5), (8, 2, 1100, 0), (8, 2, 1101, 5), (8, 2, 1099, 16)]


def _parts(rows_bf16, nsplit):
    """fp32 K parts whose bf16 sum is the given rows: the values in part 0, zeros behind."""
    parts = torch.zeros(nsplit, *rows_bf16.shape, dtype=torch.float32)
    parts[0] = rows_bf16.float()
    return parts


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("n_q,n_kv,S,tau", FUSED_CASES, ids=[f"G{q // kv}-({q},{kv})-S{S}-tau{tau}" for q, kv, S, tau in FUSED_CASES])
def test_attn_fused_keys(n_q, n_kv, S, tau, causal):
    """dfl_attn_fused: one case per GQA instantiation at S ~ 40, and S ~ 1100 with tau in {0, 5, 16}; context rows at
    buffer rows 0.., block rows at 16.., two fp32 parts."""
    from dflash_amd import ops
    bs = 16 if tau != 16 or S > 1000 else 13
    t = Tally(f"attn_fused ({n_q},{n_kv}) S{S} tau{tau} bs{bs} {'causal' if causal else 'full'}")
    ws = ops.attn_fused_ws(n_q, n_kv, 32, dev())
    cos, sin = _tables(2048)
    dyn = torch.zeros(8, dtype=torch.int32, device=dev())
    ops.set_dyn(dyn, S, tau, bs, S)
    for p in _problem_set(S, tau, bs, causal, n_q, n_kv):
        qd, kd, ld = _dims(p)
        kc, vc = (x.to(dev()) for x in _caches(p, p.n_keys + 8))
        rows = torch.cat([_ctx_rows(p, 16), _block_rows(p, 16)])
        out = torch.full((16 * qd,), NAN, dtype=BF16, device=dev())
        ops.attn_fused(qkv=_parts(rows, 2).to(dev()), nsplit=2, split_stride=32 * ld, ld=ld, q_col=0, k_col=qd, v_col=qd + kd,
                       ctx_row0=0, blk_row0=16, n_q=n_q, n_kv=n_kv, q_norm_w=None, k_norm_w=None, eps=1e-6, cos_tab=cos,
                       sin_tab=sin, kcache=kc, vcache=vc, scale=R.SCALE, dyn=dyn, kv_len_max=p.n_keys, ws=ws, max_splits=32,
                       out_frag=out, causal=causal)
        t.check(p, _rows_out(out, p))
        _check_caches(p, kc, vc, t.name)
    t.report()


# ---------------------------------------------------------------- the ragged-batch forms
L_LAYERS, LAYER = 2, 1


def _request_sets(lens, bss, causal, n_q, n_kv):
    """One problem set per request; the launches are zipped, a request with fewer needle launches repeats its census."""
    sets = [_problem_set(S, 0, bs, causal, n_q, n_kv) for S, bs in zip(lens, bss)]
    n = max(len(s) for s in sets)
    leak = 1 if causal else 0
    out = []
    for i in range(n - leak):
        out.append([s[i] if i < len(s) - leak else s[i % 2] for s in sets])
    if leak:
        out.append([s[-1] for s in sets])
    return out


def _batch_inputs(ps, QS, rows, q_tiles=1):
    """Request-major inputs of one launch: block rows [QS, 16 q_tiles, ld], 5-D caches (NaN past each request's keys, the
    other layer and the spare request slots NaN throughout), the per-request records."""
    from dflash_amd import ops
    p0 = ps[0]
    ld = _dims(p0)[2]
    x = torch.zeros(QS, 16 * q_tiles, ld, dtype=BF16)
    kc = torch.full((QS, L_LAYERS, p0.n_kv, rows, 128), NAN, dtype=BF16)
    vc = torch.full_like(kc, NAN)
    dyn = torch.zeros(QS, 8, dtype=torch.int32)
    for r, p in enumerate(ps):
        x[r] = _block_rows(p, 16 * q_tiles)
        kc[r, LAYER, :, :p.S], vc[r, LAYER, :, :p.S] = p.k[:, :p.S], p.v[:, :p.S]
        dyn[r, ops.DYN_S], dyn[r, ops.DYN_BS], dyn[r, ops.DYN_POS0] = p.S, p.bs, p.S
    return x, kc.to(dev()), vc.to(dev()), dyn.to(dev())


def _check_batch_caches(ps, kc, vc, name):
    kc, vc = kc.cpu(), vc.cpu()
    for r, p in enumerate(ps):
        _check_caches(p, kc[r, LAYER], vc[r, LAYER], f"{name} r{r}")
    assert bool(torch.isnan(kc[:, 1 - LAYER].float()).all()) and bool(torch.isnan(kc[len(ps):].float()).all()), name
    assert bool(torch.isnan(vc[:, 1 - LAYER].float()).all()) and bool(torch.isnan(vc[len(ps):].float()).all()), name


def _batch_form(n_q, n_kv, R_, kvmax, q_tiles=1):
    """attn_head_launch's pair rule for a ragged-batch launch (test_hip_batch_kernels._attn_form)."""
    return R.head_form(n_q, n_kv, kvmax - 16 * q_tiles, 16, 32, q_tiles=q_tiles, n_cand=R_, dyn=True)["kernel"]


# name: form, heads, lens, bss, cache rows (= kv_len_max), q_tiles
BATCH_LENS = (300, 0, 17, 600)
BATCH_CASES = {
    "f32-R4": ("f32", (32, 8), BATCH_LENS, (16, 16, 5, 12), 700, 1),
    "f32-R2": ("f32", (32, 8), (300, 600), (16, 9), 700, 1),
    "bf16-R4": ("bf16", (32, 8), BATCH_LENS, (16, 7, 16, 12), 700, 1),
    "bf16-R2": ("bf16", (32, 8), (0, 600), (16, 16), 700, 1),
    "bf16-R4-qt2": ("bf16", (32, 8), BATCH_LENS, (17, 32, 25, 30), 700, 2),
    "fused-R4": ("fused", (8, 2), BATCH_LENS, (16, 16, 5, 12), 700, 1),
    "fused-R2-G8": ("fused", (8, 1), (33, 0), (9, 16), 64, 1),
}


def _batch_id(name):
    form, (n_q, n_kv), lens, _, rows, qt = BATCH_CASES[name]
    return name if form == "fused" else f"{name}-{_batch_form(n_q, n_kv, len(lens), rows, qt)}"


def test_batch_cases_reach_the_pair_and_the_head_form():
    assert [_batch_id(n) for n in BATCH_CASES][:5] == ["f32-R4-pair", "f32-R2-head1", "bf16-R4-pair", "bf16-R2-head1",
                                                       "bf16-R4-qt2-head2"]


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("name", list(BATCH_CASES), ids=[_batch_id(n) for n in BATCH_CASES])
def test_attn_batch_keys(name, causal):
    """dfl_attn_head_batch_f32 / dfl_attn_head_batch (kv_len_max = cache rows: R = 4 reaches k_attn_head_pair, R = 2
    k_attn_head; q_tiles = 2 on the bf16 form) and dfl_attn_fused_batch (per-tile records, as batch.py's _attend passes
    them), ragged lengths including 0.  The f32 form gets the values in part 0 and zeros in part 1."""
    from dflash_amd import ops
    form, (n_q, n_kv), lens, bss, rows, qt = BATCH_CASES[name]
    R_, QS = len(lens), 4
    qd, kd = n_q * 128, n_kv * 128
    ld = qd + 2 * kd
    t = Tally(f"attn {name} ({n_q},{n_kv}) {'causal' if causal else 'full'}")
    cos, sin = _tables(2048)
    ws = (ops.attn_fused_batch_ws(QS, n_q, n_kv, 32, dev()) if form == "fused"
          else ops.attn_head_batch_ws(QS, n_q, 32, dev(), q_tiles=qt))
    for ps in _request_sets(lens, bss, causal, n_q, n_kv):
        x, kc, vc, dyn = _batch_inputs(ps, QS, rows, qt)
        out = torch.full((QS * qt, 16 * qd), NAN, dtype=BF16, device=dev())
        common = dict(q_col=0, k_col=qd, v_col=qd + kd, R=R_, n_q=n_q, n_kv=n_kv, q_norm_w=None, k_norm_w=None, eps=1e-6,
                      cos_tab=cos, sin_tab=sin, kcache=kc, vcache=vc, layer=LAYER, scale=R.SCALE, causal=causal, dyn=dyn,
                      kv_len_max=rows, ws=ws, max_splits=32, out_frag=out)
        if form == "f32":
            ops.attn_head_batch_f32(qkv_parts=_parts(x.view(QS * 16, ld), 2).to(dev()), nparts=2, MT=QS, ld=ld, **common)
        elif form == "bf16":
            ops.attn_head_batch(xq=x.view(QS * qt, 16, ld).to(dev()), q_tiles=qt, **common)
        else:
            ops.attn_fused_batch(qkv=_parts(x.view(QS * 16, ld), 2).to(dev()), nsplit=2, split_stride=QS * 16 * ld, ld=ld, **common)
        for r, p in enumerate(ps):
            t.check(p, _rows_out(out[r * qt:(r + 1) * qt], p), tag=f"r{r} ")
        _check_batch_caches(ps, kc, vc, t.name)
    t.report()


# ---------------------------------------------------------------- dfl_attn_head, single request
# (n_q, n_kv, S, tau, bs, max_splits, q_tiles, dyn bound or None)
HEAD_CASES = (
    [(4, 2, S, tau, 16, 8, 1, bound) for S, tau in ((0, 3), (33, 0), (1041, 16)) for bound in (None, S)]
    + [(4, 2, 9001, 0, 16, 8, 1, None),                     # each wave walks several tiles on both ping-pong buffers
       (4, 2, 300, 5, 16, 8, 1, 4000), (4, 2, 0, 0, 16, 8, 1, 4000)]        # the bound far above the record
    + [(8, 2, 70, tau, bs, 8, 2, None) for bs in (17, 32) for tau in (0, 32)]
    + [(8, 2, 5300, 0, 16, 32, 1, None), (16, 8, 5300, 0, 16, 32, 1, None), (16, 8, 5300, 7, 16, 32, 1, 5300)])


def _head_id(c):
    n_q, n_kv, S, tau, bs, ms, qt, bound = c
    form = R.head_form_id(n_q, n_kv, S if bound is None else bound, bs, ms, q_tiles=qt, dyn=bound is not None)
    return f"({n_q},{n_kv})-S{S}-tau{tau}-bs{bs}-{'imm' if bound is None else f'dyn{bound}'}-{form}"


def test_head_cases_reach_their_forms():
    forms = [R.head_form(c[0], c[1], c[2] if c[7] is None else c[7], c[4], c[5], q_tiles=c[6], dyn=c[7] is not None) for c in HEAD_CASES]
    assert forms[6] == dict(kernel="head1", ns=7, tiles_per_wave=6)
    assert [f["kernel"] for f in forms[9:13]] == ["head2"] * 4
    # k_attn_head_pair needs the workgroup budget, not the tile count, to limit the splits: 224 / n_q - 1 < tiles / 8, i.e.
    # n_q >= 16 at 5300 keys; (8, 2) at 5300 keys stays on k_attn_head with 21 splits
    assert [f["kernel"] for f in forms[13:]] == ["head1", "pair", "pair"]


def _head_args(p, cos, sin, xq, xc):
    qd, kd, _ = _dims(p)
    return dict(xq=xq, q_col=0, k_col=qd, v_col=qd + kd, xc=xc if p.tau else None, ck_col=qd, cv_col=qd + kd, n_q=p.n_q,
                n_kv=p.n_kv, q_norm_w=None, k_norm_w=None, eps=1e-6, cos_tab=cos, sin_tab=sin, scale=R.SCALE, causal=p.causal,
                tau=p.tau, bs=p.bs, pos0=p.S)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("case", HEAD_CASES, ids=[_head_id(c) for c in HEAD_CASES])
def test_attn_head_keys(case, causal):
    """dfl_attn_head: k_attn_head<1> with the lengths as immediates and from the record (also with a bound far above
    the recorded length), S = 9001 with max_splits = 8 (six tiles per wave), k_attn_head<2> (blocks of 17 and 32 rows, up
    to 64 new rows), and ~5300 cached keys on k_attn_head and on k_attn_head_pair."""
    from dflash_amd import ops
    n_q, n_kv, S, tau, bs, ms, qt, bound = case
    t = Tally(f"attn_head {_head_id(case)} {'causal' if causal else 'full'}")
    ws = ops.attn_head_ws(n_q, ms, qt, dev())
    cos, sin = _tables(16384)
    rows = (S if bound is None else bound) + tau + bs + 8
    dyn = None
    if bound is not None:
        dyn = torch.zeros(8, dtype=torch.int32, device=dev())
        ops.set_dyn(dyn, S, tau, bs, S)
    for p in _problem_set(S, tau, bs, causal, n_q, n_kv):
        kc, vc = (x.to(dev()) for x in _caches(p, rows))
        out = torch.full((qt, 16 * n_q * 128), NAN, dtype=BF16, device=dev())
        ops.attn_head(**_head_args(p, cos, sin, _block_rows(p, 16 * qt).to(dev()), _ctx_rows(p).to(dev())), kcache=kc, vcache=vc,
                      S=S if bound is None else bound, dyn=dyn, ws=ws, max_splits=ms, out_frag=out, q_tiles=qt,
                      out_tile_stride=out.stride(0) if qt == 2 else 0)
        t.check(p, _rows_out(out, p))
        _check_caches(p, kc, vc, t.name)
    t.report()


def test_checks_see_one_wrong_cache_row():
    """The path from a launch to the checks is sensitive: dfl_attn_head at 1041 cached keys with ONE cache row altered
    behind the problem's back — a census V row zeroed, a needle's two V rows swapped — fails the census with the lost
    key's residue and tile named, and the needle."""
    from dflash_amd import ops
    n_q, n_kv, S, bs, ms = 4, 2, 1041, 16, 8
    ws = ops.attn_head_ws(n_q, ms, 1, dev())
    cos, sin = _tables(16384)
    ps = _problem_set(S, 0, bs, True, n_q, n_kv)

    def run(p, spoil):
        kc, vc = _caches(p, S + bs + 8)
        spoil(vc)
        kc, vc = kc.to(dev()), vc.to(dev())
        out = torch.full((1, 16 * n_q * 128), NAN, dtype=BF16, device=dev())
        ops.attn_head(**_head_args(p, cos, sin, _block_rows(p).to(dev()), None), kcache=kc, vcache=vc, S=S, dyn=None, ws=ws,
                      max_splits=ms, out_frag=out)
        return _rows_out(out, p)

    def zero_row(vc):
        vc[:, 500] = 0

    for p, what in ((ps[0], "residue key % 128 = 116: lost 1"), (ps[1], "tile (key // 32) % 128 = 15: lost 1")):
        with pytest.raises(AssertionError, match=re.escape(what)):
            R.check_census(p, run(p, zero_row), "spoiled")
    needle = ps[2]
    key = next(k for _, _, k in needle.probes if k < S)

    def swap_rows(vc):
        vc[:, [key, key + 1]] = vc[:, [key + 1, key]]

    with pytest.raises(AssertionError, match=f"the output equals V row\\(s\\) \\[{key + 1}"):
        R.check_needle(needle, run(needle, swap_rows), "spoiled")
    R.check_needle(needle, run(needle, lambda vc: None), "clean")


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("S,tau", [(40, 0), (1100, 9)])
def test_attn_head_oproj_keys(S, tau, causal):
    """dfl_attn_head_oproj (4-wave attention workgroups beside the o_proj ones), heads (8, 2), H = 512: attn_frag only —
    the GEMM behind it is test_attn_head_oproj_equals_two_launches' — and the fail word stays 0."""
    from dflash_amd import ops
    n_q, n_kv, Hd, bs, ms = 8, 2, 512, 16, 16
    t = Tally(f"attn_head_oproj (8,2) S{S} tau{tau} {R.head_form_id(n_q, n_kv, S, bs, ms, oproj=True)} {'causal' if causal else 'full'}")
    g = H.gen(S)
    wop = ops.pack_weight((torch.randn(Hd, n_q * 128, generator=g) * (n_q * 128) ** -0.5).to(BF16).to(dev()))
    h0 = torch.randn(16, Hd, generator=g).to(BF16).to(dev())
    ws = ops.attn_head_ws(n_q, ms, 1, dev())
    sync = torch.zeros(ops.ATTN_OPROJ_SYNC_WORDS, dtype=torch.int32, device=dev())
    cos, sin = _tables(2048)
    for p in _problem_set(S, tau, bs, causal, n_q, n_kv):
        kc, vc = (x.to(dev()) for x in _caches(p, p.n_keys + 8))
        out = torch.full((16 * n_q * 128,), NAN, dtype=BF16, device=dev())
        h, ss = h0.clone(), torch.zeros(Hd, dtype=torch.float32, device=dev())
        ops.attn_head_oproj(**_head_args(p, cos, sin, _block_rows(p).to(dev()), _ctx_rows(p).to(dev())), kcache=kc, vcache=vc, S=S,
                            ws=ws, max_splits=ms, attn_frag=out, wo=wop, H=Hd, h_io=h, ss_out=ss, sync=sync)
        assert int(sync[ops.ATTN_OPROJ_FAIL_WORD]) == 0 and int(sync.abs().sum()) == 0, t.name
        t.check(p, _rows_out(out, p))
        _check_caches(p, kc, vc, t.name)
    t.report()


def _variant(p, c):
    """Candidate c of a problem on the SAME cached prefix: the heads of each kv group rotated by c and, where V is random,
    fresh V values on the block rows."""
    G = p.n_q // p.n_kv
    if c == 0 or p.kind.startswith("census"):
        return p
    perm = torch.tensor([(h // G) * G + (h % G + c) % G for h in range(p.n_q)])      # new head h takes old head perm[h]'s q
    inv = {int(o): h for h, o in enumerate(perm)}
    v = p.v.clone()
    v[:, p.S:] = torch.randn(p.n_kv, p.n_new, 128, generator=H.gen(c)).to(BF16)
    return dataclasses.replace(p, q=p.q[:, perm].contiguous(), v=v, probes=[(r, inv[h], k) for r, h, k in p.probes])


def test_attn_head_cand_keys():
    """dfl_attn_head_cand: C = 4 candidate blocks on one cached prefix of 300 keys (causal): every candidate's rows, the
    staged K / V rows bit-equal to its Linear rows, the shared cache read-only."""
    from dflash_amd import ops
    n_q, n_kv, S, bs, C, ms = 8, 2, 300, 16, 4, 16
    qd, kd = n_q * 128, n_kv * 128
    t = Tally(f"attn_head_cand (8,2) S{S} C{C} {R.head_form_id(n_q, n_kv, S, bs, ms, n_cand=C)}")
    ws = ops.attn_head_batch_ws(C, n_q, ms, dev())
    cos, sin = _tables(2048)
    for p in _problem_set(S, 0, bs, True, n_q, n_kv):
        ps = [_variant(p, c) for c in range(C)]
        kc, vc = (x.to(dev()) for x in _caches(p, S + 8))           # no room for the block rows: they must not go there
        kc0, vc0 = kc.clone(), vc.clone()
        xq = torch.stack([_block_rows(pc) for pc in ps]).to(dev())
        out = torch.full((C, 16 * qd), NAN, dtype=BF16, device=dev())
        k_out = torch.full((C, n_kv, 16, 128), NAN, dtype=BF16, device=dev())
        v_out = torch.full_like(k_out, NAN)
        ops.attn_head_cand(xq=xq, q_col=0, k_col=qd, v_col=qd + kd, n_q=n_q, n_kv=n_kv, q_norm_w=None, k_norm_w=None, eps=1e-6,
                           cos_tab=cos, sin_tab=sin, kcache=kc, vcache=vc, scale=R.SCALE, S=S, bs=bs, ws=ws, max_splits=ms,
                           out_frag=out, k_out=k_out, v_out=v_out)
        assert _same_bits(kc, kc0) and _same_bits(vc, vc0), t.name
        for c, pc in enumerate(ps):
            t.check(pc, _rows_out(out[c], pc), tag=f"c{c} ")
            assert _same_bits(k_out[c, :, :bs].cpu(), pc.k[:, S:]) and _same_bits(v_out[c, :, :bs].cpu(), pc.v[:, S:]), (t.name, c)
    t.report()


# ---------------------------------------------------------------- dfl_prefill_attn
@pytest.mark.parametrize("P", [17, 45, 300, 1024])
@pytest.mark.parametrize("n_q,n_kv", [(2, 2), (4, 2), (8, 2)], ids=["hq1", "hq2", "hq4"])
def test_prefill_attn_keys(n_q, n_kv, P):
    """dfl_prefill_attn (k_pattn's 4-stage LDS ring): census row i counts i + 1 keys; every row probes itself (the causal
    diagonal), the first key of its tile, the same lane of the tile before and row i / 2; leak probes at row i + 1 for
    the first tile, both sides of every tile edge and the last rows, against the kernel's own 1e-2 bar."""
    from dflash_amd import ops
    t = Tally(f"prefill_attn ({n_q},{n_kv}) P{P}")
    Pp = ops.prefill_rows_padded(P)
    qd = n_q * 128
    for p in _problem_set(0, 0, P, True, n_q, n_kv, True):
        if p.kind.startswith("census"):
            assert torch.equal(R.census_expected(p)[1], torch.arange(1, P + 1))
        qkv = torch.zeros(Pp, qd + 2 * n_kv * 128, dtype=BF16)
        qkv[:P, :qd] = p.q.reshape(P, qd)
        kc, vc = (x.to(dev()) for x in _caches(p, P + 40, upto=P))
        xf = torch.full((Pp * qd,), NAN, dtype=BF16, device=dev())
        ops.prefill_attn(qkv.to(dev()), P, 0, kc, vc, n_q, n_kv, R.SCALE, xf)
        t.check(p, H.unpack_tiles(xf, P, qd).reshape(P, n_q, 128).cpu(), leak_bar=1e-2)
    t.report()
