"""Constructed inputs that make every single key of an attention launch visible in its output, and the plain fp64
reference they are checked against.  torch on the CPU and numpy only; nothing here imports dflash_amd.ops or needs a GPU.

With ~1000 keys a softmax spreads its mass over hundreds of them, so the whole-tensor bar of the randn tests (max-abs
error <= 2^-6 of the output scale) cannot see one key dropped, counted twice, let through a causal mask or multiplied
into the neighbouring V row.  Two families of inputs for which the exact answer is known:

  census   every key is 0, so every visible score is exactly 0 and every weight exactly 1 (q is random: it must not
           matter).  V[key, d] = 1 iff d == code(key), code = key % 128 (lane) or (key // 32) % 128 (tile).  The
           output is count_d / n_visible: the kernel's fp32 sums are exact integers, the only inexact steps are the
           final division and the bf16 rounding.
  needle   every (query row, query head of a kv group) gets a two-hot code (a, b): q = 32 (e_a + e_b), ONE probed key
           = 16 (e_a + e_b), every other key 0 or another probe's code.  With scale = 128^-0.5 the probed key leads every
           other visible key by >= 65 in log2 units (a key sharing one dimension: 512 * scale * log2 e = 65.3), its
           weight is 1 to far below fp32 resolution and the output row is bit-equal to the probed V row (V is random).
  leak     (causal forms) row j's needle sits at block row j + 1, which row j must not see: the row then equals the
           fp64 reference under the mask; a leak is off by O(1).  One-hot codes, so no other key shares a dimension.

q and the new rows' K reach the kernels unchanged when no norm weights are passed and the rotation tables are
cos = 1, sin = 0 (rope_tables_identity); the norm and RoPE path stays covered by the existing tests against the oracle.

Key order of a decode launch: S cached rows, tau context rows, bs block rows.  Block row j sees cached and context
rows always and block row i iff not causal or i <= j.  A prefill of P rows is the same thing with S = tau = 0, bs = P,
causal."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
D = 128
SCALE = 128 ** -0.5
Q_AMP, K_AMP = 32.0, 16.0
MAX_LAUNCHES = 8
CENSUS_MAX_KEYS = 12800
TOP_WEIGHT_MIN = 1.0 - 2.0 ** -20


def bf16_steps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance in bf16 steps between two bf16 tensors (the bit patterns mapped onto a monotonic integer line)."""
    def line(x):
        i = x.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


# ---------------------------------------------------------------- visibility and the plain reference
def decode_visibility(S: int, tau: int, bs: int, causal: bool) -> torch.Tensor:
    """[bs, S + tau + bs] bool: block row j sees cached and context rows always, block row i iff not causal or i <= j."""
    vis = torch.ones(bs, S + tau + bs, dtype=torch.bool)
    if causal:
        i = torch.arange(bs)
        vis[:, S + tau:] = i[None, :] <= i[:, None]
    return vis


def prefill_visibility(P: int) -> torch.Tensor:
    """Row i sees rows <= i."""
    return decode_visibility(0, 0, P, True)


def attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, vis: torch.Tensor, scale: float = SCALE, kv_of=None):
    """Plain fp64 softmax attention with GQA and an explicit visibility mask.  q [rows, n_q, 128], k / v
    [n_kv, keys, 128], vis [rows, keys] -> (out fp64 [rows, n_q, 128], largest weight of each row fp64 [rows, n_q]).
    kv_of (the CPU mutants of test_attn_keys_cpu only): the kv head of query head h, for h // G."""
    rows, n_q, _ = q.shape
    G = n_q // k.shape[0]
    kv_of = kv_of or (lambda h: h // G)
    out = torch.empty(rows, n_q, D, dtype=F64)
    top = torch.empty(rows, n_q, dtype=F64)
    for h in range(n_q):
        sc = (q[:, h].double() @ k[kv_of(h)].double().T) * scale
        sc = sc.masked_fill(~vis, float("-inf"))
        p = torch.softmax(sc, dim=-1)
        out[:, h] = p @ v[kv_of(h)].double()
        top[:, h] = p.max(dim=-1).values
    return out, top


# ---------------------------------------------------------------- one launch's inputs
@dataclass
class Problem:
    """One request of one launch.  q [bs, n_q, 128]; k / v [n_kv, S + tau + bs, 128] hold ALL keys in key order (the
    cached rows, then what the context and block rows' Linear k / v columns must carry); vis [bs, keys]."""
    kind: str
    S: int
    tau: int
    bs: int
    causal: bool
    n_q: int
    n_kv: int
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    vis: torch.Tensor
    code: str = ""
    probes: list = field(default_factory=list)      # needle / leak: (row, head, key)

    @property
    def n_keys(self) -> int:
        return self.S + self.tau + self.bs

    @property
    def n_new(self) -> int:
        return self.tau + self.bs


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _randn_bf16(shape, g) -> torch.Tensor:
    return torch.randn(*shape, generator=g, dtype=F32).to(BF16)


def key_code(keys: torch.Tensor, code: str) -> torch.Tensor:
    if code == "lane":
        return keys % D
    assert code == "tile", code
    return (keys // 32) % D


def census_problem(S, tau, bs, causal, n_q, n_kv, code, seed=0) -> Problem:
    n = S + tau + bs
    assert n <= CENSUS_MAX_KEYS, n
    v = torch.zeros(n_kv, n, D, dtype=BF16)
    keys = torch.arange(n)
    v[:, keys, key_code(keys, code)] = 1.0
    return Problem(f"census-{code}", S, tau, bs, causal, n_q, n_kv, _randn_bf16((bs, n_q, D), _gen(seed)),
                   torch.zeros(n_kv, n, D, dtype=BF16), v, decode_visibility(S, tau, bs, causal), code=code)


def census_expected(p: Problem):
    """(count_d int64 [bs, 128], n_visible int64 [bs]): by counting, no softmax."""
    keys = torch.arange(p.n_keys)
    onehot = torch.zeros(p.n_keys, D, dtype=F64)
    onehot[keys, key_code(keys, p.code)] = 1.0
    counts = (p.vis.double() @ onehot).round().long()
    return counts, p.vis.sum(dim=1)


def check_census(p: Problem, out: torch.Tensor, name: str = "") -> dict:
    """out bf16 [bs, n_q, 128].  (1) every element within ONE bf16 step of bf16(count_d / n_visible): the sums are exact,
    the division (or reciprocal and product) is within a few fp32 ulps of count / n, which can move the one bf16 rounding
    behind it by a step where count / n lies within those ulps of a rounding boundary; (2) round(out * n_visible) ==
    count_d: a bf16 value half a step (2^-8 of the value at most, and only just above a power of two) from count / n,
    times n, is less than count * 2^-8 <= 1/2 from count while count <= 128 (asserted, with the reference's own
    rounding); a lost or gained key moves it by 1."""
    counts, nvis = census_expected(p)
    assert int(counts.max()) <= 128, (name, int(counts.max()))
    want = (counts.double() / nvis.double()[:, None]).to(BF16)
    assert torch.equal((want.double() * nvis[:, None]).round().long(), counts), f"{name}: the reference itself is not countable"
    want = want[:, None, :].expand(p.bs, p.n_q, D)
    out = out.detach().cpu()
    assert out.shape == want.shape and out.dtype == BF16, (name, tuple(out.shape), out.dtype)
    assert torch.isfinite(out.float()).all(), f"{name}: non-finite output"
    steps = bf16_steps(out, want.contiguous())
    got = (out.double() * nvis[:, None, None]).round().long()
    diff = got - counts[:, None, :]
    if bool((diff != 0).any()):
        unit = "residue key % 128" if p.code == "lane" else "tile (key // 32) % 128"
        bad = diff.nonzero()[:12].tolist()
        what = ", ".join(f"row {r} head {h} {unit} = {d}: {'gained' if diff[r, h, d] > 0 else 'lost'} "
                         f"{abs(int(diff[r, h, d]))} of {int(counts[r, d])}" for r, h, d in bad)
        raise AssertionError(f"{name} census-{p.code}: {int((diff != 0).sum())} counts differ — {what}")
    worst = int(steps.max())
    assert worst <= 1, f"{name} census-{p.code}: {worst} bf16 steps from bf16(count / n)"
    return dict(worst_steps=worst, off=int((steps > 0).sum()), signal_steps=single_key_signal_steps(p))


def single_key_signal_steps(p: Problem) -> float:
    """The smallest change, in bf16 steps of the output, that one lost key makes in the column that counted it."""
    counts, nvis = census_expected(p)
    c = counts.double().clamp(min=1)
    val = c / nvis.double()[:, None]
    step = torch.exp2(torch.floor(torch.log2(val)) - 7)
    change = (val - (c - 1) / (nvis.double()[:, None] - 1).clamp(min=1)).abs() / step
    return float(change[counts > 0].min())


# ---------------------------------------------------------------- needle
def _pairs(seed: int):
    pairs = [(a, b) for a in range(D) for b in range(a + 1, D)]
    assert len(pairs) == 8128
    order = np.random.RandomState(seed).permutation(len(pairs))
    return [pairs[i] for i in order]


def probe_positions(S: int, tau: int) -> list:
    """Cached and context keys to probe: 0, S - 1, every context row, 32 m - 1, 32 m, 32 m + 1 around every tile edge
    (S <= 1100) or every multiple of 256 (longer), all 32 offsets of the first tile, a middle tile and the last
    (ragged) tile of the cached rows."""
    n = S + tau
    pos = set(range(S, n)) | {0, S - 1}
    step = 32 if S <= 1100 else 256
    for m in range(0, S + step, step):
        pos |= {m - 1, m, m + 1}
    nt = (S + 31) // 32
    for t in {0, nt // 2, nt - 1}:
        pos |= set(range(32 * t, 32 * t + 32))
    return sorted(x for x in pos if 0 <= x < n)


def _patterns(bs: int, causal: bool, prefill: bool):
    """Maps block row j -> probed block row, every one legal under the causal mask."""
    j = torch.arange(bs)
    if prefill:
        return [j, j - j % 32, (j - 32).clamp(min=0), j // 2]
    anti = bs - 1 - j
    return [j, torch.where(anti <= j, anti, torch.full_like(j, -1)) if causal else anti]


def needle_slot_keys(S, tau, bs, causal, G, prefill=False) -> list:
    """Per launch an int64 [bs, G] table: the key (row j, head g of the kv group) probes, -1: none.  Slot k = launch * G
    + g: the first slots walk the block rows by pattern (the causal diagonal first), the others share out the cached
    and context positions, and once those run out the slots left in a launch walk the block rows again (a group
    larger than the slots there are to fill: every launch still probes every head); at most MAX_LAUNCHES launches (the
    positions are thinned evenly beyond that)."""
    pats = _patterns(bs, causal, prefill)
    free = [] if prefill else probe_positions(S, tau)
    cap = MAX_LAUNCHES * G * bs - len(pats) * bs
    if len(free) > cap:
        free = [free[i * len(free) // cap] for i in range(cap)]
    launches, nxt, k = [], 0, 0
    while k < len(pats) or nxt < len(free):
        tab = torch.full((bs, G), -1, dtype=torch.long)
        for g in range(G):
            if k < len(pats) or nxt >= len(free):       # nothing left for this slot: the block rows again, so that every
                blk = pats[k % len(pats)]               # launch probes EVERY head of the group (G > the slots there are)
                tab[:, g] = torch.where(blk >= 0, S + tau + blk, blk)
            for j in range(bs):
                if tab[j, g] < 0 and nxt < len(free):
                    tab[j, g] = free[nxt]
                    nxt += 1
            k += 1
        launches.append(tab)
        assert len(launches) <= MAX_LAUNCHES
    return launches


def needle_problem(S, tau, bs, causal, n_q, n_kv, slot_keys: torch.Tensor, seed=0) -> Problem:
    G = n_q // n_kv
    n = S + tau + bs
    g = _gen(seed)
    v = _randn_bf16((n_kv, n, D), g)
    v[v == 0] = 1.0     # an element that is exactly 0 cannot come back bit-equal: the other keys' 2^-65 weights show beside it
    k = torch.zeros(n_kv, n, D, dtype=BF16)
    q = torch.zeros(bs, n_q, D, dtype=BF16)
    codes = _pairs(seed)
    code_of, probes = {}, []
    for j in range(bs):
        for gg in range(G):
            key = int(slot_keys[j, gg])
            if key < 0:
                continue
            a, b = code_of.setdefault(key, codes[len(code_of)])
            k[:, key, a] = k[:, key, b] = K_AMP
            for kvh in range(n_kv):
                q[j, kvh * G + gg, a] = q[j, kvh * G + gg, b] = Q_AMP
                probes.append((j, kvh * G + gg, key))
    return Problem("needle", S, tau, bs, causal, n_q, n_kv, q, k, v, decode_visibility(S, tau, bs, causal), probes=probes)


def needle_problems(S, tau, bs, causal, n_q, n_kv, seed=0, prefill=False) -> list:
    return [needle_problem(S, tau, bs, causal, n_q, n_kv, tab, seed=seed + 101 * i)
            for i, tab in enumerate(needle_slot_keys(S, tau, bs, causal, n_q // n_kv, prefill))]


def check_needle(p: Problem, out: torch.Tensor, name: str = "") -> int:
    """Every probe row of out bf16 [bs, n_q, 128] is bit-equal to V[kv head, probed key]; on the fp64 reference the
    probed key's weight is >= 1 - 2^-20 (so the construction, not luck, makes the row exact).  Returns the rows checked."""
    out = out.detach().cpu()
    G = p.n_q // p.n_kv
    rows = torch.tensor([r for r, _, _ in p.probes])
    heads = torch.tensor([h for _, h, _ in p.probes])
    keys = torch.tensor([kk for _, _, kk in p.probes])
    assert bool(p.vis[rows, keys].all()), f"{name}: a probe is not visible to its row"
    ref, top = attention_ref(p.q, p.k, p.v, p.vis)
    assert float(top[rows, heads].min()) >= TOP_WEIGHT_MIN, (name, float(top[rows, heads].min()))
    want = p.v[heads // G, keys]
    assert torch.equal(ref[rows, heads].to(BF16), want), f"{name}: the reference does not return the probed rows"
    got = out[rows, heads]
    bad = (got.view(torch.int16) != want.view(torch.int16)).any(dim=-1)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        r, h, kk = p.probes[i]
        src = (p.v[h // G].view(torch.int16) == got[i].view(torch.int16)).all(dim=-1).nonzero().flatten().tolist()
        raise AssertionError(f"{name} needle: {int(bad.sum())} of {len(p.probes)} probe rows differ from their V row; first: "
                             f"row {r} head {h} key {kk} (S={p.S} tau={p.tau}) — the output equals V row(s) {src[:4]}")
    return len(p.probes)


def leak_rows(bs: int, prefill: bool) -> list:
    """Rows j whose needle sits at block row j + 1.  One code per row and 128 one-hot codes: every row of a decode
    block; for a prefill the first tile, both sides of every 32-row tile edge up to 127 rows in all, and the last rows."""
    if bs - 1 <= D:
        return list(range(bs - 1))
    rows = set(range(31)) | {bs - 2, bs - 3}
    for m in range(32, bs, 32):
        rows |= {m - 2, m - 1, m}
    rows = sorted(r for r in rows if 0 <= r < bs - 1)
    if len(rows) > D:
        rows = rows[:D - 2] + rows[-2:]
    return rows


def leak_problem(S, tau, bs, causal, n_q, n_kv, seed=0, prefill=False) -> Problem:
    assert causal
    n = S + tau + bs
    g = _gen(seed + 7)
    v = _randn_bf16((n_kv, n, D), g)
    k = torch.zeros(n_kv, n, D, dtype=BF16)
    q = torch.zeros(bs, n_q, D, dtype=BF16)
    probes = []
    dims = np.random.RandomState(seed).permutation(D)
    for c, j in enumerate(leak_rows(bs, prefill)):
        k[:, S + tau + j + 1, dims[c]] = K_AMP
        q[j, :, dims[c]] = Q_AMP
        probes += [(j, h, S + tau + j + 1) for h in range(n_q)]
    return Problem("leak", S, tau, bs, causal, n_q, n_kv, q, k, v, decode_visibility(S, tau, bs, causal), probes=probes)


def check_leak(p: Problem, out: torch.Tensor, bar: float = 2.0 ** -6, name: str = "") -> float:
    """Every row against the fp64 reference under the mask, max-abs error <= bar of the reference's largest value.  The
    construction is checked first: no probe is visible, and a row that took its hidden needle's V row instead would miss
    the bar tenfold on every probe row."""
    out = out.detach().cpu()
    rows = torch.tensor([r for r, _, _ in p.probes])
    heads = torch.tensor([h for _, h, _ in p.probes])
    keys = torch.tensor([kk for _, _, kk in p.probes])
    ref, _ = attention_ref(p.q, p.k, p.v, p.vis)
    scale = float(ref.abs().max())
    if len(p.probes):
        assert not bool(p.vis[rows, keys].any()), name
        G = p.n_q // p.n_kv
        leaked = p.v[heads // G, keys].double()
        assert float((leaked - ref[rows, heads]).abs().max(dim=-1).values.min()) > 10 * bar * scale, name
    err = float((out.double() - ref).abs().max()) / scale
    assert torch.isfinite(out.float()).all(), f"{name}: non-finite output"
    if err > bar:
        d = (out.double() - ref).abs().amax(dim=-1)
        r, h = [int(x) for x in (d == d.max()).nonzero()[0]]
        raise AssertionError(f"{name} leak: max-abs error {err:.3e} of scale exceeds {bar:.1e}; worst row {r} head {h}")
    return err


def rope_tables_identity(max_pos: int):
    """cos = 1, sin = 0: bf16(bf16(x * 1) + bf16(+-x' * 0)) == x, the rows reach the kernel unchanged."""
    return torch.ones(max_pos, 64, dtype=BF16), torch.zeros(max_pos, 64, dtype=BF16)


# ---------------------------------------------------------------- host rules of csrc/attn_head.hip, for the test ids
def head_form(n_q, n_kv, S, bs, max_splits, q_tiles=1, n_cand=1, oproj=False, dyn=False) -> dict:
    """attn_head_launch: the kernel and the old-key splits a launch sized for S cached keys gets."""
    G = n_q // n_kv
    nt = (S + 31) // 32
    tiles = 4 if oproj else 8
    wgs = 256 if (oproj or n_cand > 1) else 224
    ns = min(-(-nt // tiles), max(1, wgs // (n_q * n_cand) - 1))
    pair = (not oproj) and q_tiles == 1 and G % 2 == 0 and bs <= 16 and nt > tiles * ns and (nt > 160 or n_cand > 2)
    if pair:
        ns = min(-(-nt // tiles), max(1, wgs // ((n_q // 2) * n_cand) - 1))
    ns = min(ns, max_splits - 1)
    if nt == 0 and not dyn:
        ns = 0
    waves = 4 if oproj else 8
    per_wave = -(-(-(-nt // ns)) // waves) if ns else 0
    kernel = "pair" if pair else "oproj" if oproj else f"head{q_tiles}"
    return dict(kernel=kernel, ns=ns, tiles_per_wave=per_wave)


def head_form_id(*a, **kw) -> str:
    f = head_form(*a, **kw)
    return f"{f['kernel']}-ns{f['ns']}-tpw{f['tiles_per_wave']}"


# ---------------------------------------------------------------- a tile-wise flash emulation with planted faults
FAULTS = ("drop_tile_last_key", "double_split_first_key", "causal_strict", "v_row_plus_one", "stale_tile")


def flash_emulation(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, vis: torch.Tensor, n_split: int = 4,
                    fault: str = "", fault_tile: int = -1, scale: float = SCALE) -> torch.Tensor:
    """One query head the way the kernels walk it: 32-key tiles, fp32 scores in log2 units, exp2, P rounded to bf16 for
    the PV product, online max and sum in fp32, n_split key splits merged by log-sum-exp, a bf16 output.
    q [rows, 128], k / v [keys, 128] bf16, vis [rows, keys].  fault (on tile fault_tile, default the middle one):
      drop_tile_last_key      the tile's last key is masked
      double_split_first_key  the first key of the split that holds the tile is accumulated twice
      causal_strict           `<` for `<=`: a row does not see its own key (every tile)
      v_row_plus_one          inside the tile, weight r meets V row r + 1
      stale_tile              the tile's K and V come from four tiles back (a 4-stage ring read too early)"""
    assert fault in ("",) + FAULTS, fault
    rows, n = q.shape[0], k.shape[0]
    nt = (n + 31) // 32
    ft = fault_tile if fault_tile >= 0 else nt // 2
    qf = q.float().numpy()
    kf, vf = k.float().numpy(), v.float().numpy()
    visn = vis.numpy().copy()
    if fault == "causal_strict":
        last = visn.shape[1] - 1 - np.argmax(visn[:, ::-1], axis=1)        # each row's last visible key: its own
        full = visn.all(axis=1)
        visn[np.arange(rows)[~full], last[~full]] = False
    sl2 = np.float32(scale * 1.4426950408889634)
    tps = -(-nt // n_split)
    parts = []
    for s in range(n_split):
        m = np.full(rows, -np.inf, dtype=np.float32)
        l = np.zeros(rows, dtype=np.float32)
        o = np.zeros((rows, D), dtype=np.float32)
        for t in range(s * tps, min((s + 1) * tps, nt)):
            src = t - 4 if (fault == "stale_tile" and t == ft and t >= 4) else t
            lo = 32 * src
            width = min(32 * t + 32, n) - 32 * t
            kt, vt = kf[lo:lo + width], vf[lo:lo + width]
            vz = visn[:, 32 * t:32 * t + width].copy()
            if fault == "drop_tile_last_key" and t == ft:
                vz[:, width - 1] = False
            if fault == "v_row_plus_one" and t == ft:
                vt = np.concatenate([vt[1:], vt[-1:]])
            sc = (qf @ kt.T).astype(np.float32) * sl2
            sc = np.where(vz, sc, np.float32(-np.inf)).astype(np.float32)
            mn = np.maximum(m, sc.max(axis=1))
            safe = np.where(np.isfinite(mn), mn, np.float32(0))
            pr = np.exp2(sc - safe[:, None]).astype(np.float32)
            if fault == "double_split_first_key" and s == ft // tps and t == s * tps:
                pr[:, 0] *= 2
            resc = np.exp2(np.where(np.isfinite(m), m - safe, np.float32(-np.inf))).astype(np.float32)
            pb = torch.from_numpy(pr).to(BF16).float().numpy()
            l = (l * resc + pr.sum(axis=1, dtype=np.float32)).astype(np.float32)
            o = (o * resc[:, None] + (pb @ vt).astype(np.float32)).astype(np.float32)
            m = mn
        parts.append((m, l, o))
    mm = np.max(np.stack([p[0] for p in parts]), axis=0)
    L = np.zeros(rows, dtype=np.float32)
    O = np.zeros((rows, D), dtype=np.float32)
    for m, l, o in parts:
        w = np.exp2(np.where(np.isfinite(m), m - mm, np.float32(-np.inf))).astype(np.float32)
        L = (L + l * w).astype(np.float32)
        O = (O + o * w[:, None]).astype(np.float32)
    return torch.from_numpy((O / L[:, None]).astype(np.float32)).to(BF16)
