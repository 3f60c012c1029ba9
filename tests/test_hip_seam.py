"""The seam that carries the residual stream from one layer to the next in every ragged-tile path (dflash_amd/tile_stack.py):

    dfl_gemm_f32_batch   o_proj / down_proj as fp32 K-part sums [ksplit][batch_tiles(R)*16][N]   (k_gemm_b<MT, EPI_F32>)
    dfl_norm_frag_batch  adds the parts (or the MoE expert shares) to h, one rounding, tap, RMSNorm -> frag16

each alone, the two chained on the stride contract between them (parts batch_tiles(R)*16*N floats apart, whatever the
caller's tile-slot count), and TileStack.run + finish over them, against the plain reference of tests/seam_ref.py.
Buffers are wider than the kernel is told and sentinel-filled, and compared whole; what the header calls ignored is
NaN-poisoned.  The shapes are picked with the mirrored host rules; tests/test_seam_cpu.py pins the forms they reach."""
import pytest
import torch

import helpers as H
import seam_ref as S

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
SENT = -7.0                      # exactly representable; no kernel output below is -7 by construction of the checks
NAN = float("nan")
EINVAL = -22
DYN_BS = 2


def dev():
    return torch.device("cuda", 0)


def _cuda_gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _log(what, **kw):
    import os
    H._log_parity({"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "what": what, **kw})


def _frag_check(name, got_rows, h_new_rows, nw, eps=S.EPS):
    """Normalised rows against rms_frag_ref: every element within 2 bf16 steps, at most FLIP_CAP of them different (a
    last-bit difference in rstd moves a rounding).  got_rows / h_new_rows [n, H] bf16 on the CPU."""
    if got_rows.shape[0] == 0:
        return 0.0
    assert not torch.isnan(got_rows.float()).any(), name
    d = S.bf16_steps(got_rows, S.rms_frag_ref(h_new_rows, nw, eps))
    share, mx = float((d > 0).float().mean()), int(d.max())
    print(f"[parity] {name}: {share:.2e} of {d.numel()} elements differ from rms_frag_ref (cap {S.FLIP_CAP:.0e}), max {mx} bf16 steps")
    _log(name, flip_share=share, max_steps=mx, cap=S.FLIP_CAP, elements=d.numel())
    assert mx <= 2, (name, mx)
    assert share <= S.FLIP_CAP, (name, share)
    return share


# ================================================================ a. dfl_norm_frag_batch with pending sums
class NormBuffers:
    """Everything one dfl_norm_frag_batch launch touches, wider than the kernel is told: h as a view with ldh = H + 8 and
    17 rows per request, the tap as columns j*H..(j+1)*H of a [slots, 16, 3H + 8] buffer (the view TileStack._norm builds),
    frag16 buffers 16H + 64 apart, one slot more than R of each; parts [nsplit][batch_tiles(R)*16][ldp] (+ slack)."""

    def __init__(self, Hd, R, nsplit, via, tap_j):
        self.H, self.R, self.ns, self.via, self.tap_j = Hd, R, nsplit, via, tap_j
        self.bt = S.batch_tiles(R)
        self.hbuf = torch.full((R + 1, 17, Hd + 8), SENT, dtype=BF16, device=dev())
        self.h = self.hbuf[:, :16, :Hd]
        self.tapbuf = torch.full((R + 1, 16, 3 * Hd + 8), SENT, dtype=BF16, device=dev())
        self.tap = None if tap_j is None else self.tapbuf[:, :, tap_j * Hd:(tap_j + 1) * Hd]
        self.fragbuf = torch.full((R + 1, 16 * Hd + 64), SENT, dtype=BF16, device=dev())
        # K parts: the layout dfl_gemm_f32_batch(N = H) leaves; shares: a row stride and a share stride with slack
        self.ldp = Hd if via == "K" else Hd + 4
        self.psplit = self.bt * 16 * self.ldp + (0 if via == "K" else 8)
        self.part = torch.full((max(nsplit, 1) * self.psplit,), NAN, dtype=F32, device=dev()) if nsplit else None
        self.nw = None

    def load(self, h, parts, nw, valid):
        """Fresh inputs: h [R, 16, H] bf16, parts [ns, R*16, H] fp32 (CPU).  The parts rows of invalid rows, of the slots
        >= R and the slack columns stay NaN; h rows >= valid keep their data (the kernel must leave them alone)."""
        R, Hd = self.R, self.H
        self.hbuf.fill_(SENT)
        self.h[:R] = h.to(dev())
        self.nw = nw.to(dev())
        if self.part is not None:
            self.part.fill_(NAN)
            for k in range(self.ns):
                pv = self.part[k * self.psplit:k * self.psplit + self.bt * 16 * self.ldp].view(self.bt * 16, self.ldp)
                for r in range(R):
                    nv = valid[r]
                    pv[r * 16:r * 16 + nv, :Hd] = parts[k, r * 16:r * 16 + nv].to(dev())

    def launch(self, dyn, word=DYN_BS, **over):
        from dflash_amd import ops
        a = dict(h=self.h.data_ptr(), h_stride=self.h.stride(0), ldh=self.h.stride(1), R=self.R,
                 part=None if self.part is None else self.part.data_ptr(), nsplit=self.ns, psplit=self.psplit, ldp=self.ldp,
                 tap=None if self.tap is None else self.tap.data_ptr(), ldtap=self.tapbuf.stride(1),
                 tap_stride=self.tapbuf.stride(0), nw=self.nw.data_ptr(), eps=S.EPS, frag=self.fragbuf.data_ptr(),
                 frag_stride=self.fragbuf.stride(0), H=self.H, dyn=None if dyn is None else dyn.data_ptr(), word=word)
        a.update(over)
        return ops.lib().dfl_norm_frag_batch(a["h"], a["h_stride"], a["ldh"], a["R"], a["part"], a["nsplit"], a["psplit"],
                                             a["ldp"], a["tap"], a["ldtap"], a["tap_stride"], a["nw"], a["eps"], a["frag"],
                                             a["frag_stride"], a["H"], a["dyn"], a["word"], _stream())


def _norm_expect(h, parts, ns, valid, R):
    """The new h rows [R, 16, H]: rows < valid through parts_add_ref (or unchanged without parts), the others unchanged."""
    Hd = h.shape[2]
    new = h.clone()
    if ns:
        added = S.parts_add_ref(h, parts.view(-1, R, 16, Hd), ns)
        for r in range(R):
            new[r, :valid[r]] = added[r, :valid[r]]
    return new


def _norm_check(name, B, h, parts, nw, valid):
    """All of B's buffers against the reference, whole."""
    R, Hd = B.R, B.H
    new = _norm_expect(h, parts, B.ns, valid, R)
    want_h = torch.full_like(B.hbuf, SENT).cpu()
    want_h[:R, :16, :Hd] = new
    got_h = B.hbuf.cpu()
    assert not torch.isnan(got_h.float()).any(), f"{name}: NaN leaked into h"
    assert torch.equal(got_h, want_h), f"{name}: h differs (rows < valid bit for bit, everything else untouched)"
    got_tap = B.tapbuf.cpu()
    want_tap = torch.full_like(got_tap, SENT)
    if B.tap is not None:
        for r in range(R):
            want_tap[r, :valid[r], B.tap_j * Hd:(B.tap_j + 1) * Hd] = new[r, :valid[r]]
    assert torch.equal(got_tap, want_tap), f"{name}: tap differs (rows < valid = the new h rows, everything else untouched)"
    got_f = B.fragbuf.cpu()
    assert torch.all(got_f[R:] == SENT) and torch.all(got_f[:, 16 * Hd:] == SENT), f"{name}: frag written outside its tiles"
    share = 0.0
    for r in range(R):
        rows = S.frag16_unpack(got_f[r], Hd)
        assert torch.count_nonzero(rows[valid[r]:].float()) == 0 and not torch.isnan(rows.float()).any(), \
            f"{name}: frag rows >= valid of request {r} are not zero"
        share = max(share, _frag_check(f"{name} r{r}", rows[:valid[r]], new[r, :valid[r]], nw))
    return share


def _dyn_for(valid, R):
    """[R, 8] records with the valid counts in the DYN_BS word and values that would show in every other word."""
    if valid is None:
        return None
    d = torch.full((R, 8), 13, dtype=torch.int32)
    d[:, 0], d[:, 1] = 16, 3
    for r in range(R):
        d[r, DYN_BS] = valid[r]
    return d.to(dev())


NORM_CASES, _K_OF = S.NORM_CASES, S.NORM_K_OF
NORM_IDS = [S.norm_case_id(c) for c in NORM_CASES]


@pytest.mark.parametrize("Hd,R,ns,via,valid,tap_j", NORM_CASES, ids=NORM_IDS)
def test_norm_frag_batch_pending_sums(Hd, R, ns, via, valid, tap_j):
    """dfl_norm_frag_batch adding K parts / expert shares: h and tap rows < valid equal parts_add_ref bit for bit, rows
    outside keep their sentinels, frag rows >= valid are zero, frag rows < valid within 2 bf16 steps of rms_frag_ref with at
    most 2e-3 of them different.  Launched twice into the same buffers with fresh inputs: the second result is checked in
    full as well, so nothing of the first may show in it."""
    from dflash_amd import ops
    if via == "K":
        assert ops.batch_ksplit(_K_OF[ns]) == ns == S.batch_ksplit(_K_OF[ns])
    assert ops.batch_tiles(R) == S.batch_tiles(R)
    B = NormBuffers(Hd, R, ns, via, tap_j)
    v = valid if valid is not None else [16] * R
    dyn = _dyn_for(valid, R)
    name = f"norm_frag_batch H{Hd} R{R} ns{ns}{via or ''}"
    worst = 0.0
    for launch in range(2):
        h, parts, nw = S.norm_case_data(Hd, R, ns, 100 + Hd + 17 * launch)
        B.load(h, parts, nw, v)
        assert B.launch(dyn) == 0, ops.lib().dfl_last_error()
        worst = max(worst, _norm_check(f"{name} launch {launch}", B, h, parts, nw, v))
    _log(name + " worst", flip_share=worst)


@pytest.mark.parametrize("Hd,R,ns,via", [(2560, 3, 6, "K"), (8200, 4, 8, "shares"), (16384, 2, 2, "K")])
def test_norm_frag_batch_small_ints_exact(Hd, R, ns, via):
    """Integer h, integer-valued parts, norm_w = 1: the new rows and the tap are exact integers whatever is rounded where —
    a pure index check (a wrong chunk, part or row shows as a wrong integer).  The column index is folded into the data
    (h = column mod 7 - 3 + row) so that a duplicated or shifted chunk cannot reproduce its neighbour."""
    g = torch.Generator().manual_seed(Hd + R)
    col = torch.arange(Hd)
    h = ((col * 5 + col // 8) % 7 - 3)[None, None, :] + torch.randint(-4, 5, (R, 16, 1), generator=g)
    parts = torch.randint(-3, 4, (ns, R * 16, Hd), generator=g) + ((col // 8) % 3 - 1)[None, None, :]
    valid = [16, 9, 1, 5][:R]
    B = NormBuffers(Hd, R, ns, via, 2)
    hb, pf = h.to(BF16), parts.to(F32)
    B.load(hb, pf, torch.ones(Hd, dtype=BF16), valid)
    assert B.launch(_dyn_for(valid, R)) == 0
    new = _norm_expect(hb, pf, ns, valid, R)
    exact = (h + parts.sum(0).view(R, 16, Hd)).to(BF16)       # |values| <= 7 + 8 * 4: exact in bf16
    for r in range(R):
        assert torch.equal(new[r, :valid[r]], exact[r, :valid[r]])
    _norm_check(f"norm ints H{Hd} R{R}", B, hb, pf, torch.ones(Hd, dtype=BF16), valid)


def test_norm_frag_batch_rejections():
    """DFL_EINVAL and nothing launched: every buffer still holds what it held."""
    Hd, R, ns = 64, 2, 2
    B = NormBuffers(Hd, R, ns, "shares", 0)
    h, parts, nw = S.norm_case_data(Hd, R, ns, 1)
    valid = [16, 16]
    B.load(h, parts, nw, valid)
    dyn = _dyn_for(valid, R)
    before = [t.clone() for t in (B.hbuf, B.tapbuf, B.fragbuf)]
    big = 16392   # strides that would do for it, so that only the H limit refuses
    bad = [dict(H=60), dict(H=big, ldh=big, ldp=big, ldtap=3 * big + 8, frag_stride=16 * big), dict(ldh=Hd - 8),
           dict(ldh=Hd + 4), dict(ldp=Hd - 4), dict(nsplit=0), dict(ldtap=Hd - 8), dict(R=0), dict(R=5),
           dict(frag_stride=16 * Hd - 8)]
    for over in bad:
        assert B.launch(dyn, **over) == EINVAL, over
    torch.cuda.synchronize()
    for a, b in zip(before, (B.hbuf, B.tapbuf, B.fragbuf)):
        assert torch.equal(a, b)
    assert B.launch(dyn) == 0      # and the unmodified call is accepted


# ================================================================ b. dfl_gemm_f32_batch, slab form, exact on small integers
def _ints(shape, g, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g, device=dev(), dtype=torch.int8).to(BF16)


TAIL = 1024


def _gemm_exact(N, K, Rs):
    """out NaN-filled with a sentinel tail; for slots < R the sum over the parts equals x @ W^T bit for bit (small
    integers: every product and fp32 sum is exact), each part is the GEMM over its own k-steps, every part entry was
    written; plain rows >= valid are NaN in memory and must give exact zeros."""
    from dflash_amd import ops
    g = _cuda_gen(N + K)
    w = _ints((N, K), g, -2, 2)
    wp = ops.pack_weight(w)
    wd = w.double()
    ks, pk = S.batch_ksplit(K), S.part_ksteps(K) * 32
    assert ops.batch_ksplit(K) == ks
    for R in Rs:
        MT = ops.batch_tiles(R)
        x = _ints((MT, 16, K), g, -1, 2)                 # asymmetric: a sign error cannot cancel
        n = ks * MT * 16 * N
        for mode in ("frag", "rows"):
            out = torch.full((n + TAIL,), NAN, dtype=F32, device=dev())
            out[n:] = SENT
            xe = x.clone()
            if mode == "frag":
                src = ops.brows_frag(H.frag_of(x))
                dyn = H.dyn_records([(0, 16)] * MT, MT, dev())
            else:
                valid = [([16, 5, 1, 9][r] if r < R else 0) for r in range(MT)]
                xm = x.clone()
                for r in range(MT):
                    xm[r, valid[r]:] = NAN
                    xe[r, valid[r]:] = 0
                src = ops.brows_plain(xm, ops.DYN_BS)
                dyn = H.dyn_records([(0, v) for v in valid], MT, dev())
            ops.gemm_f32_batch(wp, src, R, N, K, out, dyn)
            parts = out[:n].view(ks, MT, 16, N)[:, :R]
            assert bool(torch.isfinite(parts).all()), (mode, R, "a part entry of a slot < R was not written, or NaN leaked")
            assert bool((out[n:] == SENT).all()), (mode, R, "tail written")
            xd = xe[:R].double()
            assert torch.equal(parts.sum(0).double(), xd @ wd.T), (mode, R, "sum over the parts")
            for k in range(ks):
                c0, c1 = min(k * pk, K), min((k + 1) * pk, K)
                assert torch.equal(parts[k].double(), xd[:, :, c0:c1] @ wd[:, c0:c1].T), (mode, R, "part", k)


@pytest.mark.parametrize("N,K", S.GEMM_SMALL, ids=[f"N{N}-K{K}-{S.gemm_form_id(N, K)}" for N, K in S.GEMM_SMALL])
def test_gemm_f32_batch_slab_exact(N, K):
    _gemm_exact(N, K, (1, 2, 3, 4))


@pytest.mark.parametrize("N,K", S.GEMM_MODEL, ids=[f"N{N}-K{K}-{S.gemm_form_id(N, K)}" for N, K in S.GEMM_MODEL])
def test_gemm_f32_batch_slab_exact_model_points(N, K):
    _gemm_exact(N, K, (4,))


def test_gemm_f32_batch_rejects_17_parts():
    from dflash_amd import ops
    from dflash_amd._lib import DFlashHipError
    N, K, R = 16, S.GEMM_K_REJECTED, 4
    assert ops.batch_ksplit(K) == 17
    w = torch.zeros(N, K, dtype=BF16, device=dev())
    x = torch.zeros(4, 16 * K, dtype=BF16, device=dev())
    out = torch.full((17 * 4 * 16 * N,), SENT, dtype=F32, device=dev())
    with pytest.raises(DFlashHipError):
        ops.gemm_f32_batch(w.view(-1), ops.brows_frag(x), R, N, K, out, H.dyn_records([(0, 16)] * 4, 4, dev()))
    assert bool((out == SENT).all())


# ================================================================ c. the two chained, on random data
@pytest.mark.parametrize("Hd,K", S.CHAIN_CASES, ids=[f"H{h}-K{k}-{S.gemm_form_id(h, k)}" for h, k in S.CHAIN_CASES])
def test_gemm_f32_then_norm_frag_batch(Hd, K):
    """gemm_f32_batch(N = H, K) into a part buffer, norm_frag_batch(part, K) behind it, through the ops wrappers, with
    exactly batch_tiles(R) tile slots and with 4 slots at R <= 2 (the candidate verifier's allocation: the parts stay
    batch_tiles(R)*16*H apart).  The new h equals parts_add_ref over the kernel's own parts bit for bit; the parts' sum
    is within the worst-case fp32 accumulation bound K 2^-24 (|x| @ |W|^T) of a float64 GEMM."""
    from dflash_amd import ops
    g = _cuda_gen(Hd + K)
    w = (torch.randn(Hd, K, generator=g, device=dev()) * 0.05).to(BF16)
    wp = ops.pack_weight(w)
    ks = ops.batch_ksplit(K)
    nw = (1 + 0.1 * torch.randn(Hd, generator=g, device=dev())).to(BF16)
    for R, slots in [(1, 2), (2, 2), (3, 4), (4, 4), (1, 4), (2, 4)]:
        bt = ops.batch_tiles(R)
        name = f"chain H{Hd} K{K} R{R} slots{slots}"
        x = torch.randn(slots, 16, K, generator=g, device=dev()).to(BF16)
        h0 = (torch.randn(slots, 16, Hd, generator=g, device=dev()) * 2).to(BF16)
        valid = [16, 9, 1, 5][:R]
        dyn = H.dyn_records([(0, v) for v in valid] + [(0, 0)] * (slots - R), slots, dev())
        n = ks * bt * 16 * Hd
        part = torch.full((ks * 4 * 16 * Hd + TAIL,), NAN, dtype=F32, device=dev())   # room for a 4-slot stride too
        part[n:n + TAIL] = SENT
        ops.gemm_f32_batch(wp, ops.brows_frag(H.frag_of(x)), R, Hd, K, part, dyn)
        assert bool((part[n:n + TAIL] == SENT).all()), name
        own = part[:n].view(ks, bt, 16, Hd)[:, :R].clone()
        got = own.double().sum(0)
        ref = x[:R].double() @ w.double().T
        bound = K * 2.0 ** -24 * (x[:R].double().abs() @ w.double().abs().T)
        err = ((got - ref).abs() / bound).max()
        print(f"[parity] {name}: parts' sum vs float64 GEMM, worst |err| / bound = {float(err):.3e}")
        _log(name + " gemm", err_over_bound=float(err))
        assert bool(((got - ref).abs() <= bound).all()), name
        h = h0.clone()
        taps = torch.full((slots, 16, 3 * Hd + 8), SENT, dtype=BF16, device=dev())
        xn = torch.full((slots, 16 * Hd), SENT, dtype=BF16, device=dev())
        ops.norm_frag_batch(h, R, nw, S.EPS, xn, dyn, ops.DYN_BS, part=part, N=Hd, K=K, tap=taps[:, :, Hd:2 * Hd])
        want = h0.cpu().clone()
        added = S.parts_add_ref(h0[:R].cpu(), own.cpu(), ks)
        want_tap = torch.full_like(taps, SENT).cpu()
        for r in range(R):
            want[r, :valid[r]] = added[r, :valid[r]]
            want_tap[r, :valid[r], Hd:2 * Hd] = added[r, :valid[r]]
        assert torch.equal(h.cpu(), want), f"{name}: h is not bf16(h + bf16(part 0 + part 1 + ...)) of the kernel's own parts"
        assert torch.equal(taps.cpu(), want_tap), f"{name}: tap"
        xc = xn.cpu()
        assert bool((xc[R:] == SENT).all()), name
        for r in range(R):
            rows = S.frag16_unpack(xc[r], Hd)
            assert torch.count_nonzero(rows[valid[r]:].float()) == 0, name
            _frag_check(f"{name} r{r}", rows[:valid[r]], want[r, :valid[r]], nw.cpu())


# ================================================================ d. TileStack.run + finish against stack_ref
SH, SQ, SI, SNQKV, SLOTS = 512, 2112, 4160, 2624, 4
TAP_LAYERS = (0, 0, 1)


def _stack_weights(seed):
    """Three layers — dense, MoE-style (3 expert shares), dense — as plain [out, in] bf16 weights on the device."""
    g = _cuda_gen(seed)
    r = lambda o, i: (torch.randn(o, i, generator=g, device=dev()) / i ** 0.5).to(BF16)                      # noqa: E731
    nrm = lambda: (1 + 0.1 * torch.randn(SH, generator=g, device=dev())).to(BF16)                            # noqa: E731
    L = []
    for kind in ("dense", "moe", "dense"):
        lw = dict(ln1=nrm(), ln2=nrm(), qkv=r(SNQKV, SH), o=r(SH, SQ))
        if kind == "moe":
            lw["experts"] = [r(SH, SH) * 0.6 for _ in range(3)]
        else:
            lw.update(gate=r(SI, SH), up=r(SI, SH), down=r(SH, SI))
        L.append(lw)
    return L, nrm()


def _packed(L):
    from dflash_amd import ops
    out = []
    for lw in L:
        p = dict(ln1=lw["ln1"], ln2=lw["ln2"], qkv=ops.pack_weight(lw["qkv"]), o=ops.pack_weight(lw["o"]))
        if "experts" in lw:
            p.update(gu_e=True, experts=lw["experts"])
        else:
            p.update(gu=ops.pack_weight_gateup(lw["gate"], lw["up"]), down=ops.pack_weight(lw["down"]))
        out.append(p)
    return out


def _new_stack(qkv, adopt):
    from dflash_amd import ops, tile_stack
    gws = tile_stack.gemm_ws(SH, [SNQKV, 2 * SI], [SQ, SI], dev())
    z = lambda *s: torch.zeros(*s, dtype=BF16, device=dev())  # noqa: E731
    own = dict(h=z(SLOTS, 16, SH), attn=z(SLOTS, 16 * SQ), act=z(SLOTS, 16 * SI), xq=z(SLOTS, 16, SNQKV)) if adopt else {}
    st = tile_stack.TileStack(H=SH, q_dim=SQ, I=SI, nqkv=SNQKV, eps=S.EPS, MT=SLOTS, gws=gws, part_qkv=qkv == "parts",
                              moe_nsplit=3, **own)
    if adopt:
        assert all(getattr(st, k) is v for k, v in own.items())
    assert st.part_h.numel() == max(ops.batch_ksplit(SQ), ops.batch_ksplit(SI), 3) * SLOTS * 16 * SH
    return st


def _run_stack(st, PL, final_norm, R, bs, h_rows, qkv, tap_layers=TAP_LAYERS):
    """One run + finish with torch closures for the attention stage and the MoE MLP: only the stack's own launches and
    its protocol are under test.  Returns (h, taps, xn) as left on the device."""
    from dflash_amd import ops
    bt = ops.batch_tiles(R)
    st.h.fill_(SENT)
    for r in range(R):
        st.h[r, :bs[r]] = h_rows[r][:bs[r]]
    taps = torch.full((SLOTS, 16, len(tap_layers) * SH), SENT, dtype=BF16, device=dev())
    dyn = H.dyn_records([(0, b) for b in bs] + [(0, 0)] * (SLOTS - R), SLOTS, dev())

    def attend(i, lw):
        for r in range(R):
            if qkv == "rows":
                q = st.xq[r, :, :SQ].float()
            else:
                nk = ops.batch_ksplit(SH)
                pq = st.part_qkv[:nk * bt * 16 * SNQKV].view(nk, bt * 16, SNQKV)[:, r * 16:(r + 1) * 16, :SQ]
                q = pq.sum(0).to(BF16).float()
            a = torch.tanh(q).to(BF16)
            a[bs[r]:] = 0
            st.attn[r, :16 * SQ] = S.frag16_pack(a)

    def moe(lw, R_, MT_, dyn_, xn, part_h):
        assert R_ == R and MT_ == SLOTS and xn is st.xn and part_h is st.part_h
        pv = part_h[:3 * bt * 16 * SH].view(3, bt * 16, SH)
        for r in range(R):
            x = S.frag16_unpack(xn[r], SH).float()
            for s, we in enumerate(lw["experts"]):
                pv[s, r * 16:(r + 1) * 16] = x @ we.float().T
        return 3

    st.run(PL, R, dyn, attend, qkv=qkv, taps=taps, tap_layers=tap_layers, moe=moe)
    st.finish(final_norm)
    torch.cuda.synchronize()
    return st.h.clone(), taps, st.xn.clone()


@pytest.mark.parametrize("R,qkv,adopt", [(1, "rows", True), (3, "parts", False), (3, "rows", False), (1, "parts", True)],
                         ids=["R1-rows-adopted", "R3-parts-own", "R3-rows-own", "R1-parts-adopted"])
def test_tile_stack_against_stack_ref(R, qkv, adopt):
    """TileStack.run + finish (dense, MoE-style, dense; tap_layers (0, 0, 1); 4 tile slots) against stack_ref in float64
    with the documented bf16 roundings.  The o_proj sums are 2 K parts, the down sums 3, the expert shares 3.  Rows >= bs
    of h and of the taps are untouched; a second run on fresh inputs gives the bits a fresh stack gives (nothing stale
    may stay in part_h between a 3-part and a 2-part layer); tapping the last layer is refused."""
    from dflash_amd import ops
    assert (ops.batch_ksplit(SQ), ops.batch_ksplit(SI)) == (2, 3)
    L, fin = _stack_weights(11)
    PL = _packed(L)
    bs = [16, 7, 1][:R] if R > 1 else [7]
    g = _cuda_gen(5 + R)
    inputs = [[torch.randn(16, SH, generator=g, device=dev()).to(BF16) for _ in range(R)] for _ in range(2)]
    st = _new_stack(qkv, adopt)
    with pytest.raises(NotImplementedError):
        st.run(PL, R, None, None, qkv=qkv, taps=None, tap_layers=(2,), moe=None)
    h, taps, xn = _run_stack(st, PL, fin, R, bs, inputs[0], qkv)
    Lc = [{k: ([e.cpu() for e in v] if isinstance(v, list) else v.cpu()) for k, v in lw.items()} for lw in L]
    hc, tc, xc = h.cpu(), taps.cpu(), xn.cpu()
    assert bool((hc[R:] == SENT).all()) and bool((tc[R:] == SENT).all())
    for r in range(R):
        n = bs[r]
        rh, rt, rx = S.stack_ref(inputs[0][r][:n].cpu(), Lc, fin.cpu(), S.EPS, SQ, TAP_LAYERS)
        assert bool((hc[r, n:] == SENT).all()) and bool((tc[r, n:] == SENT).all()), "rows >= bs of h / the taps were written"
        name = f"tile stack R{R} {qkv} tile {r}"
        H.assert_close(name + " h", hc[r, :n], rh)
        for j in range(3):
            H.assert_close(name + f" tap slot {j}", tc[r, :n, j * SH:(j + 1) * SH], rt[:, j * SH:(j + 1) * SH])
        assert torch.equal(tc[r, :n, :SH], tc[r, :n, SH:2 * SH]), "the slots of a repeated tap id differ"
        rows = S.frag16_unpack(xc[r], SH)
        assert torch.count_nonzero(rows[n:].float()) == 0
        H.assert_close(name + " xn", rows[:n], rx)
    # second run of the same stack on fresh inputs == a fresh stack on them, bit for bit
    h2, taps2, xn2 = _run_stack(st, PL, fin, R, bs, inputs[1], qkv)
    h3, taps3, xn3 = _run_stack(_new_stack(qkv, adopt), PL, fin, R, bs, inputs[1], qkv)
    assert torch.equal(h2, h3) and torch.equal(taps2, taps3)
    assert torch.equal(xn2[:R], xn3[:R])
