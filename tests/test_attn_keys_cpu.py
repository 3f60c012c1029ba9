"""The census and needle constructions of attn_keys_ref test something: a tile-wise flash emulation (fp32 scores, exp2, P
rounded to bf16, online max and sum, key splits, a bf16 output) passes them bit-exactly, every planted key-bookkeeping
fault fails at least one of them; how the same faults fare against the old whole-tensor bar on randn inputs is printed.
CPU only."""
import functools

import numpy as np
import pytest
import torch

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
