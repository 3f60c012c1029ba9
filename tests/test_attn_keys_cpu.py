"""The census and needle constructions of attn_keys_ref test something: a tile-wise flash emulation (fp32 scores, exp2, P
rounded to bf16, online max and sum, key splits, a bf16 output) passes them bit-exactly, every planted key-bookkeeping
fault fails at least one of them; how the same faults fare against the old whole-tensor bar on randn inputs is printed.
Behind that, the GQA group sizes: what the case tables of attn_gqa_cases hold, that the constructions stand at every new
(n_q, n_kv), and that the needle — not the census — sees a wrong kv head.  CPU only."""
import functools

import numpy as np
import pytest
import torch

import attn_gqa_cases as C
import attn_keys_ref as R

SIZES = (1040, 6016, 12800)          # keys: S cached rows + one causal block of 16
BS = 16


def _emulate(p, **kw):
    """All heads of a problem (one kv head here) through the emulation: bf16 [bs, n_q, 128]."""
    G = p.n_q // p.n_kv
    with np.errstate(invalid="ignore"):
        return torch.stack([R.flash_emulation(p.q[:, h], p.k[h // G], p.v[h // G], p.vis, **kw) for h in range(p.n_q)], dim=1)


@functools.lru_cache(maxsize=None)
def _problems(n):
    S = n - BS
    census = [R.census_problem(S, 0, BS, True, 1, 1, code, seed=n) for code in ("lane", "tile")]
    return census, R.needle_problems(S, 0, BS, True, 1, 1, seed=n)


def _fault_tile(n):
    return ((n - BS + 31) // 32) // 2     # the middle tile of the cached rows, which probe_positions covers offset by offset


def _run(n, fault):
    """(census failures, needle failures) of the emulation with `fault`, as lists of messages."""
    census, needles = _problems(n)
    kw = dict(fault=fault, fault_tile=_fault_tile(n), n_split=4)
    bad_c, bad_n = [], []
    for p in census:
        try:
            st = R.check_census(p, _emulate(p, **kw), f"{n} keys")
            assert st["worst_steps"] == 0, f"{p.kind}: {st['worst_steps']} bf16 steps"      # bit-exact, not just within one
        except AssertionError as e:
            bad_c.append(str(e))
    for p in needles:
        try:
            R.check_needle(p, _emulate(p, **kw), f"{n} keys")
        except AssertionError as e:
            bad_n.append(str(e))
    return bad_c, bad_n


@pytest.mark.parametrize("n", SIZES)
def test_clean_emulation_is_bit_exact(n):
    bad_c, bad_n = _run(n, "")
    assert not bad_c and not bad_n, (bad_c, bad_n)
    census, needles = _problems(n)
    sig = min(R.single_key_signal_steps(p) for p in census)
    print(f"[parity] census {n} keys: one key moves its column by >= {sig:.1f} bf16 steps; "
          f"{sum(len(p.probes) for p in needles)} needle rows in {len(needles)} launches")
    assert sig > 1.0      # even assertion 1 alone sees a single key; assertion 2 (the count) sees it at any size


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_planted_fault_fails(n, fault):
    bad_c, bad_n = _run(n, fault)
    print(f"[parity] {fault} at {n} keys: census {'FAILS' if bad_c else 'passes'}, needle {'FAILS' if bad_n else 'passes'}"
          + (f" — {(bad_c + bad_n)[0][:200]}" if bad_c or bad_n else ""))
    assert bad_c or bad_n, fault


def test_census_names_the_lost_key():
    """The failure message names the residue (lane code) and the tile (tile code) of a dropped key."""
    n = 1040
    ft = _fault_tile(n)
    bad_c, _ = _run(n, "drop_tile_last_key")
    assert any(f"residue key % 128 = {(32 * ft + 31) % 128}: lost 1" in m for m in bad_c), bad_c
    assert any(f"tile (key // 32) % 128 = {ft % 128}: lost 1" in m for m in bad_c), bad_c


def test_randn_bar_against_the_faults():
    """The gap these tests close: on randn keys a planted single-key fault moves the output by about the old bar itself
    (max-abs <= 2^-6 of the fp64 reference's scale) at 6016 keys and by less with every further key, while census and
    needle fail it at every size.  How many faults the old bar lets through is printed, not asserted."""
    for n in (6016, 12800):
        S = n - BS
        g = torch.Generator().manual_seed(1)
        q, k, v = (torch.randn(*s, generator=g).to(R.BF16) for s in ((BS, 1, 128), (1, n, 128), (1, n, 128)))
        vis = R.decode_visibility(S, 0, BS, True)
        ref, _ = R.attention_ref(q, k, v, vis)
        scale = float(ref.abs().max())
        passed = []
        for fault in ("",) + R.FAULTS:
            with np.errstate(invalid="ignore"):
                out = R.flash_emulation(q[:, 0], k[0], v[0], vis, fault=fault, fault_tile=_fault_tile(n))
            err = float((out.double() - ref[:, 0]).abs().max()) / scale
            print(f"[parity] randn {n} keys, fault {fault or 'none'}: max {err:.3e} of scale (bar {2 ** -6:.3e})")
            if err <= 2 ** -6:
                passed.append(fault)
        assert "" in passed
        print(f"[parity] {len(passed) - 1} of {len(R.FAULTS)} planted faults pass the 2^-6 bar on {n} randn keys: {passed[1:]}")


def test_constructions():
    """Visibility, probe positions, slot tables and the host-rule mirror say what the GPU cases rely on."""
    vis = R.decode_visibility(3, 2, 4, True)
    assert vis[:, :5].all() and vis[0, 5] and not vis[0, 6] and vis[3].all()
    assert R.decode_visibility(3, 2, 4, False).all()
    assert torch.equal(R.prefill_visibility(5), torch.tril(torch.ones(5, 5, dtype=torch.bool)))
    pos = R.probe_positions(1041, 5)
    assert {0, 1040, 1041, 1045, 31, 32, 33, 1023, 1024, 1025}.issubset(pos) and set(range(1024, 1041)).issubset(pos)
    for S, tau, bs, causal, G in ((0, 0, 16, True, 1), (1100, 16, 16, False, 4), (9001, 0, 16, True, 2), (33, 32, 17, True, 4)):
        tabs = R.needle_slot_keys(S, tau, bs, causal, G)
        assert 1 <= len(tabs) <= R.MAX_LAUNCHES
        seen = set()
        vis = R.decode_visibility(S, tau, bs, causal)
        for tab in tabs:
            for j in range(bs):
                for g in range(G):
                    if tab[j, g] >= 0:
                        assert vis[j, tab[j, g]]
                        seen.add(int(tab[j, g]))
        assert set(range(S + tau, S + tau + bs)).issubset(seen)               # every block row, the diagonal included
        assert set(R.probe_positions(S, tau)).issubset(seen) or S > 5000
    tabs = R.needle_slot_keys(0, 0, 300, True, 1, prefill=True)
    assert len(tabs) == 4 and torch.equal(tabs[0][:, 0], torch.arange(300))
    assert len(R.leak_rows(1024, True)) <= 128 and len(R.leak_rows(16, False)) == 15
    # csrc/attn_head.hip's pair rule: two heads per workgroup only where the workgroup budget, not the tile count, limits the splits
    assert R.head_form(16, 8, 5300, 16, 32)["kernel"] == "pair" and R.head_form(8, 2, 5300, 16, 32)["kernel"] == "head1"
    assert R.head_form(32, 8, 5300, 16, 32)["kernel"] == "pair"
    assert R.head_form(4, 2, 9001, 16, 8) == dict(kernel="head1", ns=7, tiles_per_wave=6)
    assert R.head_form(8, 2, 1100, 16, 16, oproj=True)["kernel"] == "oproj"


# ---------------------------------------------------------------- GQA group sizes (tests/attn_gqa_cases.py, test_hip_attn_gqa.py)
GQA_HEADS = [h for h in C.all_heads() if h != (4, 2)]          # (4, 2) is the older tests' geometry


def test_gqa_case_tables_keep_their_groups():
    """What tests/test_hip_attn_gqa.py promises, asserted without a GPU: every case has n_kv >= 2 (head = kvh * G + hh: with
    one kv head a wrong kvh * G is 0 whatever G is), and no table loses a group."""
    assert all(n_kv >= 2 and n_q % n_kv == 0 for n_q, n_kv in C.all_heads())
    assert {C.group(c[:2]) for c in C.HEAD_CASES} >= {1, 3, 5, 6, 7, 8, 16}
    for form in ("f32", "bf16"):
        for R_ in (2, 4):
            assert {C.group(v[1]) for v in C.BATCH_CASES.values() if v[0] == form and len(v[2]) == R_} >= {3, 5, 6}, (form, R_)
    assert all(0 in v[2] and max(v[2]) + 16 <= v[4] for v in C.BATCH_CASES.values())       # one request at S = 0; the rows fit
    assert {C.group(h) for h in C.CAND_HEADS} >= {3, 5, 6}
    assert {C.group(h) for h, S, _ in C.OPROJ_CASES if S < 100} >= {3, 5, 6} <= {C.group(h) for h, S, _ in C.OPROJ_CASES if S > 1000}
    assert all(n_q * 128 <= 4096 for (n_q, _), _, _ in C.OPROJ_CASES)                       # dfl_attn_head_oproj's own limit
    assert {C.group(h) for h in C.PREFILL_HEADS} >= {3, 5, 6, 7, 8, 16}
    assert {g for g, _, _ in C.BLOCK_CASES} == {1, 2, 3, 5, 7, 8} and C.group(C.BLOCK_REFUSED) == 9
    assert {C.group(h) for h in C.FUSED_HEADS} == {1, 2, 8} and {C.group(h) for h in C.FUSED_REFUSED} == {3, 5, 6, 7, 16}
    assert {C.group(h) for h in C.ROW_HEADS} == {3, 5, 8}


def test_gqa_head_cases_reach_their_forms():
    """The launch form of every chosen dfl_attn_head case, by the mirror of attn_head_launch's rule."""
    forms = {c: C.head_form(c) for c in C.HEAD_CASES}
    assert all(f["kernel"] == "head1" and f["tiles_per_wave"] == 1 for c, f in forms.items() if c in C.HEAD_SHORT)
    assert all(f["kernel"] == "head2" for c, f in forms.items() if c in C.HEAD_QT2)
    # G = 6 and G = 8 at ~5300 keys: k_attn_head_pair with hpg = G / 2 = 3 and 4 workgroups per kv head and split
    for c in C.HEAD_LONG[:3]:
        assert forms[c] == dict(kernel="pair", ns=21, tiles_per_wave=1) and C.group(c[:2]) // 2 in (3, 4), c
    assert {C.group(c[:2]) for c in C.HEAD_LONG[:3]} == {6, 8}
    # G = 5 never pairs: (40, 8) keeps the budget's 224 / 40 - 1 = 4 splits of 42 tiles, six per wave
    assert C.HEAD_LONG[3][:2] == (40, 8) and forms[C.HEAD_LONG[3]] == dict(kernel="head1", ns=4, tiles_per_wave=6)
    # ragged batch: R = 4 of the even non-power-of-two group pairs through n_cand > 2; the odd groups never do; R = 4
    # requests of 40 heads floor the budget (256 / 160 - 1 < 1) at one split
    for form in ("f32", "bf16"):
        assert C.batch_form(f"{form}-R4-G6") == dict(kernel="pair", ns=5, tiles_per_wave=1)
        assert C.batch_form(f"{form}-R2-G6")["kernel"] == "head1"
        assert all(C.batch_form(f"{form}-R{r}-G{g}")["kernel"] == "head1" for r in (2, 4) for g in (3, 5))
        assert C.batch_form(f"{form}-R4-G5-40x8") == dict(kernel="head1", ns=1, tiles_per_wave=3)
    assert [C.prefill_form(h) for h in C.PREFILL_HEADS] == [(1, 3), (1, 5), (2, 3), (1, 7), (4, 2), (4, 4)]


@functools.lru_cache(maxsize=None)
def _gqa_problems(heads, causal):
    n_q, n_kv = heads
    ps = [R.census_problem(33, 5, 16, causal, n_q, n_kv, code, seed=n_q) for code in ("lane", "tile")]
    ps += R.needle_problems(33, 5, 16, causal, n_q, n_kv, seed=n_q)
    if causal:
        ps.append(R.leak_problem(33, 5, 16, True, n_q, n_kv, seed=n_q))
        ps += R.needle_problems(0, 0, 45, True, n_q, n_kv, seed=n_q, prefill=True)
        ps.append(R.leak_problem(0, 0, 45, True, n_q, n_kv, seed=n_q, prefill=True))
    return ps


def _ref_out(p, kv_of=None):
    return R.attention_ref(p.q, p.k, p.v, p.vis, kv_of=kv_of)[0].to(R.BF16)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("heads", GQA_HEADS, ids=lambda h: f"G{h[0] // h[1]}-({h[0]},{h[1]})")
def test_gqa_constructions_hold_on_the_reference(heads, causal):
    """Every new geometry, decode and prefill shaped: on the fp64 reference the census counts are exact, every needle probe
    returns its V row (check_needle asserts its top weight >= TOP_WEIGHT_MIN), leak probes are invisible; and every needle
    launch probes every query head, those of kv groups >= 1 included."""
    n_q, n_kv = heads
    for p in _gqa_problems(heads, causal):
        out = _ref_out(p)
        if p.kind.startswith("census"):
            assert R.check_census(p, out)["worst_steps"] == 0
        elif p.kind == "needle":
            assert R.check_needle(p, out) == len(p.probes) > 0
            assert {h for _, h, _ in p.probes} == set(range(n_q))          # kv groups >= 1 included
        else:
            assert R.check_leak(p, out) <= 2.0 ** -8          # bf16 rounding of the reference itself


def gqa_mutants(n_q, n_kv):
    """Wrong maps from a query head to its kv head: head // G' for the next power of two above G and for G - 1 (clamped
    to the last kv head), and the right G with the heads of kv groups 0 and 1 swapped."""
    G = n_q // n_kv
    up = 1 << G.bit_length()
    m = {f"G'={up} (next power of two)": lambda h: min(h // up, n_kv - 1),
         "kv groups 0 and 1 swapped": lambda h: {0: 1, 1: 0}.get(h // G, h // G)}
    if G > 1:
        m[f"G'={G - 1}"] = lambda h: min(h // (G - 1), n_kv - 1)
    return m


@pytest.mark.parametrize("heads", GQA_HEADS, ids=lambda h: f"G{h[0] // h[1]}-({h[0]},{h[1]})")
def test_needle_sees_a_wrong_kv_head_and_the_census_cannot(heads):
    """Sensitivity, on the reference only: attention_ref with the kv head of a query head taken as head // G' for a wrong G'
    (or with two kv groups swapped) fails check_needle at every new geometry — V is random per kv head, so the row that
    comes back is the other group's.  The census CANNOT see this: its K is 0 and its V the same in every kv head, so the
    mutants pass check_census unchanged.  Hence every GPU case of test_hip_attn_gqa.py runs the needle family, never the
    census alone."""
    n_q, n_kv = heads
    ps = _gqa_problems(heads, True)
    census, needle = ps[0], ps[2]
    for name, kv_of in gqa_mutants(n_q, n_kv).items():
        assert any(kv_of(h) != h // (n_q // n_kv) for h in range(n_q)), name
        with pytest.raises(AssertionError, match="probe rows differ from their V row"):
            R.check_needle(needle, _ref_out(needle, kv_of), name)
        assert R.check_census(census, _ref_out(census, kv_of), name)["worst_steps"] == 0
        print(f"[parity] ({n_q},{n_kv}) mutant {name}: check_needle FAILS, check_census passes")
