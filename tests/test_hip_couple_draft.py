"""The coupled draft draw on the GPU, launch by launch: the draft head and the verify head draw
the same noise word for word (records set by the real helpers); dfl_grammar_draft_sample_rows against the numpy model of
couple_draft_ref.py, ids array_equal; which launches a session and a decoder enqueue with the keyword off and on."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import couple_draft_common as C
import couple_draft_ref as CD
import grammar_draft_ref as GD
import grammar_ref as GR
import helpers as H
import sampling_ref as SR

pytestmark = pytest.mark.gpu
BF16, I16, I32, I64, F32 = torch.bfloat16, torch.int16, torch.int32, torch.int64, torch.float32
SENT_BITS, SENT_ID = 0x1234, -7
T = 0.7
dev = C.dev


# ------------------------------------------------------------------------------------------------------------ the records
def _head_case(seed):
    """An lm_head [V = 2048, K = 512] and 16 activation rows for the verify; the draft's rows are the same rows one slot
    further down (draft row j = verify row j - 1: the same logits for the same position)."""
    from dflash_amd import ops
    g = torch.Generator(device=dev()).manual_seed(seed)
    W = (torch.randn(2048, 512, generator=g, device=dev()) * 0.05).to(BF16)
    xt = torch.randn(16, 512, generator=g, device=dev()).to(BF16)
    xd = torch.zeros_like(xt)
    xd[1:] = xt[:-1]
    return ops.pack_weight(W), xt, xd


@pytest.mark.parametrize("start", [40, 1039])
def test_draft_head_and_verify_head_draw_the_same_noise(start):
    """The draft head as model.draft_tokens(sample=dict(..., stream=RNG_TARGET)) launches it, positions from the draft
    record's START word as dfl_set_dyn2 writes it for a draft forward (S, tau, bs, pos0 = S: START = S + tau), and the
    verify head as NativeTarget.verify launches it (POS0 of the block-form record; the eager form with the host's start
    likewise).  Slot j of the block and verify row j - 1 return the same id for every j; on RNG_DRAFT, or with the draft
    record one position off, they do not."""
    from dflash_amd import ops
    V, K, bs, seed, tau = 2048, 512, 16, 2 ** 41 + 9, 5
    wp, xt, xd = _head_case(start)
    m = C.draft_model()
    ws = ops.argmax_ws(dev())
    dyn_d, dyn_t = (torch.zeros(16, dtype=I32, device=dev()) for _ in range(2))
    ops.set_dyn2(dyn_d, start - tau, tau, bs, start - tau)          # model.draft_block: S, tau, bs, pos0 = S
    ops.set_dyn2(dyn_t, start, 0, bs, start)                        # NativeTarget.verify: block form
    assert int(dyn_d[ops.DYN_START]) == start and int(dyn_t[ops.DYN_POS0]) == start

    def verify(replayed):
        post = torch.full((16,), -1, dtype=I64, device=dev())
        ops.gemm_sample(wp, ops.rows_plain(xt), V, K, 0, bs, ws, post, 0, seed=seed, temperature=T,
                        pos_dyn=dyn_t[:8] if replayed else None, pos_word=ops.DYN_POS0, pos_base=start, pos_add=1,
                        dyn=dyn_t[:8])
        return post.cpu().numpy()

    def draft(stream, dyn=dyn_d, host=None):
        blk = torch.full((16,), -1, dtype=I64, device=dev())
        lg = torch.zeros(16, V, dtype=BF16, device=dev())
        m.draft_tokens(ops.rows_plain(xd), wp, bs, blk, logits=lg,
                       sample=dict(seed=seed, temperature=T, dyn=dyn, start=host, stream=stream))
        return blk.cpu().numpy(), lg

    post = verify(True)
    assert np.array_equal(post, verify(False))
    blk, lg = draft(ops.RNG_TARGET)
    assert blk[0] == -1 and np.array_equal(blk[1:], post[:-1]), (blk, post)
    assert np.array_equal(draft(ops.RNG_TARGET, dyn=None, host=start)[0], blk)           # the host's start: the same words
    # and both are the mirror's coupled draw over the logits the draft head materialised
    want, gaps = CD.draw(lg.float().cpu().numpy(), T, seed, start, bs)
    safe = gaps[1:] > 1e-3
    assert safe.mean() >= 0.9 and np.array_equal(blk[1:][safe], want[1:][safe])
    own = draft(ops.RNG_DRAFT)[0]
    assert (own[1:] != post[:-1]).sum() >= 8, own                                         # independent noise
    ops.set_dyn2(dyn_d, start - tau + 1, tau, bs, start - tau + 1)
    off = draft(ops.RNG_TARGET)[0]
    assert (off[1:] != post[:-1]).sum() >= 8, off                                         # an off-by-one in p: independent too


def test_batch_heads_draw_the_same_noise_per_slot():
    """dfl_gemm_sample_batch at R = 3 with per-slot invT (slot 1 greedy: the plain argmax on both sides): the draft head
    as BatchedDecoder._draft_head launches it (row0 = 1, START word, stream TARGET) and the verify head (row0 = 0, POS0
    word + 1) agree slot by slot, row by row."""
    from dflash_amd import ops
    V, K, R = 2048, 512, 3
    g = torch.Generator(device=dev()).manual_seed(77)
    W = (torch.randn(V, K, generator=g, device=dev()) * 0.05).to(BF16)
    MT = ops.batch_tiles(R)
    xt = torch.randn(MT, 16, K, generator=g, device=dev()).to(BF16)
    xd = torch.zeros_like(xt)
    xd[:, 1:] = xt[:, :-1]
    bs, starts = [16, 16, 9], [40, 1039, 300]
    rec = torch.zeros(MT, 8, dtype=torch.int32)
    for t in range(R):
        rec[t, ops.DYN_BS], rec[t, ops.DYN_POS0], rec[t, ops.DYN_START] = bs[t], starts[t], starts[t]
    rec = rec.to(dev())
    seeds = torch.tensor([ops.seed_i64(s) for s in (3, 2 ** 63 + 5, 77, 0)][:MT], dtype=I64, device=dev())
    inv = torch.tensor([float(SR.inv_t(0.7)), 0.0, float(SR.inv_t(1.0)), 0.0][:MT], dtype=F32, device=dev())
    gws = torch.zeros(ops.lib().dfl_gemm_batch_ws_bytes(V, K), dtype=torch.uint8, device=dev())
    wp = ops.pack_weight(W)
    post = torch.full((MT, 16), -1, dtype=I64, device=dev())
    ops.gemm_sample_batch(wp, ops.brows_frag(H.frag_of(xt)), R, V, K, 0, 16, gws, post, 0, rec, seeds=seeds, inv_ts=inv,
                          pos_word=ops.DYN_POS0, pos_add=1, nrows_dyn_word=ops.DYN_BS)

    def draft(stream):
        blk = torch.full((MT, 16), -1, dtype=I64, device=dev())
        ops.gemm_sample_batch(wp, ops.brows_frag(H.frag_of(xd)), R, V, K, 1, 15, gws, blk, 1, rec, seeds=seeds, inv_ts=inv,
                              stream=stream, pos_word=ops.DYN_START, pos_add=0, nrows_dyn_word=ops.DYN_BS)
        return blk.cpu().numpy()
    blk, own, post = draft(ops.RNG_TARGET), draft(ops.RNG_DRAFT), post.cpu().numpy()
    greedy = (xt[1].float() @ W.float().T).to(BF16).float().argmax(dim=1).cpu().numpy()
    for t in range(R):
        n = bs[t]
        assert np.array_equal(blk[t, 1:n], post[t, :n - 1]), t
        assert (blk[t, n:] == -1).all() and blk[t, 0] == -1
        if t == 1:    # the greedy slot: no noise on either stream
            assert np.array_equal(own[t, 1:n], post[t, :n - 1]) and np.array_equal(post[t, :n], greedy[:n])
        else:
            assert (own[t, 1:n] != post[t, :n - 1]).sum() >= n // 2, t


# ------------------------------------------------------------------------------------------------------------ the pick kernel
def to_bf16(b: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16)).to(dev()).view(BF16)


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def pool_of(tables, V, spare=2):
    """tests/test_hip_grammar_draft.py::pool_of: the tables in one pool, `spare` all-illegal rows in front of each."""
    bases, rows, at = [], [], 0
    for t in tables:
        rows.append(np.full((spare, V), -1, np.int16))
        at += spare
        bases.append(at)
        rows.append(t)
        at += len(t)
    return np.concatenate(rows), bases


def state_of(pool, base, state):
    return SimpleNamespace(table=d(pool), base=d(np.asarray(base, np.int32)), state=d(np.asarray(state, np.int32)))


def sentinel_blocks(n):
    return SENT_ID - np.arange(n * 16, dtype=np.int64).reshape(n, 16)


def run_pick(x, st, bias, blocks, *, seeds, ld_pad=24, blk_pad=3, **kw):
    """x bits [T, 16, V] and blocks int64 [T, 16] in padded buffers through ops.grammar_draft_sample_rows; the logits,
    the state and what lies behind a slot's 16 ids must come back unchanged."""
    from dflash_amd import ops
    n, _, V = x.shape
    buf = to_bf16(np.full((n, 16, V + ld_pad), SENT_BITS, dtype=np.uint16))
    logits = buf[:, :, :V]
    logits.copy_(to_bf16(x))
    raw = buf.clone()
    bbuf = torch.full((n, 16 + blk_pad), SENT_ID, dtype=I64, device=dev())
    blk = bbuf[:, :16]
    blk.copy_(d(blocks))
    s0 = None if st is None else (st.base.clone(), st.state.clone())
    b = None if bias is None else d(np.asarray(bias, np.float32))
    sd = torch.tensor([ops.seed_i64(s) for s in seeds], dtype=I64, device=dev())
    ops.grammar_draft_sample_rows(logits, st, bias=b, block=blk, seeds=sd, **kw)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(I16), raw.view(I16)) and (bbuf[:, 16:] == SENT_ID).all()
    if st is not None:
        assert torch.equal(st.base, s0[0]) and torch.equal(st.state, s0[1])
    return blk.cpu().numpy()


def want_of(x, blocks, pool, base, state, bias, ns, seeds, invs, starts, screen=1e-4):
    out = []
    for t in range(len(x)):
        w, _, gaps = CD.pick(x[t], ns[t], blocks[t], seed=seeds[t], inv_t=np.float32(invs[t]), pos0=starts[t], pool=pool,
                             base=-1 if base is None else base[t], state=-1 if state is None else state[t],
                             bias=None if bias is None else bias[t])
        assert all(g > screen for g in gaps), (t, min(gaps))       # (the inputs: no pick rests on a logf rounding)
        out.append(w)
    return np.stack(out)


SEEDS4 = (3, 2 ** 63 + 5, 77, 1 << 40)
STARTS4 = (40, 1039, 7, 300000)


@pytest.mark.parametrize("form", ["grammar", "bias", "both"])
def test_pick_against_the_model(form):
    """V = 2048, four slots with their own seeds and position bases (one from each record's START word), two grammars at
    different pool bases; slot 1 has no grammar, slot 2 is violated; slot 3 has invT = 0 and must return the sibling's
    plain pick.  The rows hold NaN, +-inf and +-0 (grammar_ref.case_rows): a legal +inf ties in the perturbed key on
    purpose (the lowest legal column wins), a NaN key never wins."""
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(2048 + len(form))
    pool, bases = pool_of([GR.case_dfa(rng, 3, V, 0.5), GR.case_dfa(rng, 300, V, 0.5)], V)
    base, state = [bases[0], -1, bases[1], bases[1]], [1, 0, -1, 299]
    x = np.stack([GR.case_rows(rng, 16, V) for _ in range(4)])
    x[0, 3, [100, 900, 1500]] = 0x7F80                                # +inf three times in one row: a tie in the key
    bias = None
    if form != "grammar":
        bias = np.where(rng.random((4, V)) < 0.4, -np.inf, rng.standard_normal((4, V)) * 30).astype(np.float32)
        bias[:, V - 1] = 0.0
    blocks = sentinel_blocks(4)
    st = None if form == "bias" else state_of(pool, base, state)
    invs = [float(SR.inv_t(0.7)), float(SR.inv_t(1.0)), float(SR.inv_t(0.7)), 0.0]
    dyn = torch.zeros(4, 8, dtype=I32)
    dyn[:, ops.DYN_BS] = 16
    dyn[:, ops.DYN_START] = torch.tensor(STARTS4, dtype=I32)
    got = run_pick(x, st, bias, blocks, seeds=SEEDS4, inv_ts=d(np.asarray(invs, np.float32)), dyn=dyn.to(dev()),
                   nrows_dyn_word=ops.DYN_BS, pos_dyn_word=ops.DYN_START)
    args = (pool if st else None, base if st else None, state if st else None, bias, [16] * 4)
    want = want_of(x, blocks, *args, SEEDS4, invs, STARTS4)
    assert np.array_equal(got, want), np.nonzero(got != want)
    assert np.array_equal(got[:, 0], blocks[:, 0])
    assert np.array_equal(got[2], blocks[2]) == (form != "bias") and np.array_equal(got[1], blocks[1]) == (form == "grammar")
    # slot 3 (invT = 0) is the sibling's output, bit for bit; a noisy slot is not
    sib = blocks.copy()
    sibt = d(sib)
    ops.grammar_draft_rows(to_bf16(x), st, bias=None if bias is None else d(bias), block=sibt)
    sib = sibt.cpu().numpy()
    assert np.array_equal(got[3], sib[3]) and (got[0, 1:] != sib[0, 1:]).any()
    # another position base moves the picks: the noise is keyed by START + m
    dyn[:, ops.DYN_START] += 1
    moved = run_pick(x, st, bias, blocks, seeds=SEEDS4, inv_ts=d(np.asarray(invs, np.float32)), dyn=dyn.to(dev()),
                     nrows_dyn_word=ops.DYN_BS, pos_dyn_word=ops.DYN_START)
    assert (moved[0, 1:] != got[0, 1:]).any() and np.array_equal(moved[3], got[3])


def test_block_size_from_the_record_and_a_host_position():
    """n = dyn[t][DYN_BS]: 16, 5, 1 (a block without a draft token) and 0 (an idle slot); the position base from the host
    (one value for the launch) and a scalar temperature."""
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(5)
    pool, bases = pool_of([GR.case_dfa(rng, 7, V, 0.5)], V)
    ns = [16, 5, 1, 0]
    x = np.stack([GR.case_rows(rng, 16, V) for _ in range(4)])
    blocks = sentinel_blocks(4)
    dyn = torch.zeros(4, 8, dtype=I32)
    dyn[:, ops.DYN_BS] = torch.tensor(ns, dtype=I32)
    got = run_pick(x, state_of(pool, [bases[0]] * 4, [0, 1, 2, 3]), None, blocks, seeds=SEEDS4, temperature=0.7,
                   dyn=dyn.to(dev()), nrows_dyn_word=ops.DYN_BS, pos_base=1039)
    want = want_of(x, blocks, pool, [bases[0]] * 4, [0, 1, 2, 3], None, ns, SEEDS4, [SR.inv_t(0.7)] * 4, [1039] * 4)
    assert np.array_equal(got, want)
    assert np.array_equal(got[2], blocks[2]) and np.array_equal(got[3], blocks[3])
    assert (got[1, 1:5] >= 0).all() and np.array_equal(got[1, 5:], blocks[1, 5:])


def test_stops_a_row_without_a_legal_column_and_ties():
    """A hand-written grammar over V = 2048: the only legal column is V - 1; a legal set that is all -inf ties in the key
    (-inf + g = -inf: the lowest legal column); a legal set that is all +inf likewise; a legal set that is all NaN stops:
    the rows behind keep their ids.  Then a state without any legal column stops at once."""
    V = 2048
    t = np.full((6, V), -1, np.int16)
    t[0, V - 1] = 1
    t[1, [5, 1030]] = 2                   # all -inf
    t[2, [70, 600, 2047]] = 3             # all +inf
    t[3, [3, 77]] = 4                     # all NaN: stop
    pool, bases = pool_of([t], V)
    rng = np.random.default_rng(3)
    x = GR.f32_to_bf16_bits((rng.standard_normal((16, V)) * 4).astype(np.float32)).reshape(16, V)
    x[2, [5, 1030]] = 0xFF80
    x[3, [70, 600, 2047]] = 0x7F80
    x[4, [3, 77]] = 0x7FC0
    blocks = sentinel_blocks(1)
    got = run_pick(x[None], state_of(pool, bases, [0]), None, blocks, seeds=[9], temperature=0.7, pos_base=40)
    want, states, _ = CD.pick(x, 16, blocks[0], seed=9, inv_t=SR.inv_t(0.7), pos0=40, pool=pool, base=bases[0], state=0)
    assert np.array_equal(got[0], want)
    assert got[0, 1:4].tolist() == [V - 1, 5, 70] and states == [0, 1, 2, 3]
    assert np.array_equal(got[0, 4:], blocks[0, 4:])
    got = run_pick(x[None], state_of(pool, bases, [5]), None, blocks, seeds=[9], temperature=0.7, pos_base=40)
    assert np.array_equal(got, blocks)


@pytest.mark.parametrize("n", [2, 16])
def test_full_vocabulary(n):
    """V = 151936 on a single tile, S = 300 at a non-zero base, with a bias table: every thread makes several trips."""
    V = 151936
    rng = np.random.default_rng(7 + n)
    pool, bases = pool_of([GR.case_dfa(rng, 2, V, 0.5), GR.case_dfa(rng, 300, V, 0.5)], V)
    x = GR.case_rows(rng, 16, V)[None]
    bias = np.where(rng.random((1, V)) < 0.3, -np.inf, 0).astype(np.float32)
    blocks = sentinel_blocks(1)
    got = run_pick(x, state_of(pool, [bases[1]], [299]), bias, blocks, seeds=[2 ** 63 + 5], temperature=0.7, nrows=n,
                   pos_base=1039)
    want = want_of(x, blocks, pool, [bases[1]], [299], bias, [n], [2 ** 63 + 5], [SR.inv_t(0.7)], [1039])
    assert np.array_equal(got, want)
    assert np.array_equal(got[0, n:], blocks[0, n:]) and got[0, 0] == blocks[0, 0] and (got[0, 1:n] >= 0).all()


def test_eager_and_replayed_launches_give_the_same_ids():
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(13)
    pool, bases = pool_of([GR.case_dfa(rng, 5, V, 0.5), GR.case_dfa(rng, 9, V, 0.5)], V)
    st = state_of(pool, bases, [4, 8])
    x = np.stack([GR.case_rows(rng, 16, V) for _ in range(2)])
    logits = to_bf16(x)
    blocks = sentinel_blocks(2)
    eager, replayed = d(blocks), d(blocks)
    sd = torch.tensor([5, 6], dtype=I64, device=dev())
    kw = dict(seeds=sd, temperature=0.7, pos_base=123)
    ops.grammar_draft_sample_rows(logits, st, block=eager, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        ops.grammar_draft_sample_rows(logits, st, block=replayed, **kw)
    replayed.copy_(d(blocks))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager, replayed) and (eager[:, 1:] >= 0).all()


def test_refusals():
    from dflash_amd import ops
    V = 64
    rng = np.random.default_rng(1)
    pool, bases = pool_of([GR.case_dfa(rng, 2, V)], V)
    x = to_bf16(GR.case_rows(rng, 32, V).reshape(2, 16, V))
    blk = d(np.zeros((2, 16), np.int64))
    st = state_of(pool, bases * 2, [0, 0])
    sd = torch.zeros(2, dtype=I64, device=dev())
    with pytest.raises(ValueError):
        ops.grammar_draft_sample_rows(x, st, block=blk, seeds=sd)                                  # neither temperature nor inv_ts
    with pytest.raises(ValueError):
        ops.grammar_draft_sample_rows(x, st, block=blk, seeds=sd, temperature=0.7, inv_ts=torch.ones(2, device=dev()))
    with pytest.raises(TypeError):
        ops.grammar_draft_sample_rows(x, st, block=blk, seeds=sd.to(I32), temperature=0.7)
    with pytest.raises(NotImplementedError):
        ops.grammar_draft_sample_rows(x, st, block=blk, seeds=sd, temperature=0.7, tiles_per_req=2)


# ------------------------------------------------------------------------------------------------------------ routing
def _spy(monkeypatch, names):
    """Every call of ops.<name> logged as (name, args, kwargs) in front of the real launch."""
    from dflash_amd import ops
    log = []
    for n in names:
        real = getattr(ops, n)
        monkeypatch.setattr(ops, n, (lambda real, n: lambda *a, **k: (log.append((n, a, k)), real(*a, **k))[1])(real, n))
    return log


HEADS = ("gemm_argmax", "gemm_sample", "grammar_draft_rows", "grammar_draft_sample_rows", "gemm_argmax_batch",
         "gemm_sample_batch")


def _session(couple, **kw):
    from dflash_amd.generate import DecodeSession
    cfg = H.tiny_cfg()
    s = DecodeSession(C.draft_model(cfg), C.native(), C.prompt(), mask_token_id=cfg.mask_token_id, max_new_tokens=40,
                      max_block_size=16, stop_token_ids=None, temperature=T, sampler="device", seed=5, couple_draft=couple,
                      **kw)
    s.prefill()
    return s


def test_session_routing(monkeypatch):
    """Off at T = 0.7: the draft head is gemm_argmax into the block, no gemm_sample writes the block and the new op is
    never called.  On: the draft head is gemm_sample with stream == RNG_TARGET, the request's seed, the target's
    temperature and the draft cache's record (START word); no gemm_argmax writes the block.  With constrain_draft the pick
    behind it is grammar_draft_sample_rows, off: grammar_draft_rows.  At T = 0 the keyword changes nothing."""
    from dflash_amd import ops
    from dflash_amd.generate import DecodeSession
    log = _spy(monkeypatch, HEADS)

    def heads(s):
        del log[:]
        for _ in range(2):
            s.cycle(16, ahead_ok=True)
        torch.cuda.synchronize()
        blk = s.block.data_ptr()
        return [(n, a, k) for n, a, k in log if n.startswith("gemm_") and a[7].data_ptr() == blk], [e[0] for e in log]

    draft, names = heads(_session(False))
    assert draft and {e[0] for e in draft} == {"gemm_argmax"} and "grammar_draft_sample_rows" not in names
    s = _session(True)
    draft, names = heads(s)
    assert len(draft) >= 2 and {e[0] for e in draft} == {"gemm_sample"}       # cycle 0's own draft and the run-ahead ones
    for _, a, k in draft:
        assert k["stream"] == ops.RNG_TARGET and k["seed"] == 5 and k["temperature"] == T and a[4] == 1
        assert k["pos_word"] == ops.DYN_START and k["pos_dyn"].data_ptr() == s.dcache.dyn.data_ptr()
    assert not {"grammar_draft_rows", "grammar_draft_sample_rows"} & set(names)
    ban = dict(banned_token_ids=[7, 8, 9])
    s = _session(True, constrain_draft=True, **ban)
    draft, names = heads(s)
    assert {e[0] for e in draft} == {"gemm_sample"} and "grammar_draft_sample_rows" in names
    assert "grammar_draft_rows" not in names
    picks = [(a, k) for n, a, k in log if n == "grammar_draft_sample_rows"]
    assert all(k["pos_dyn_word"] == ops.DYN_START and k["dyn"].data_ptr() == s.dcache.dyn.data_ptr() for _, k in picks)
    _, names = heads(_session(False, constrain_draft=True, **ban))
    assert "grammar_draft_rows" in names and "grammar_draft_sample_rows" not in names
    # T = 0: the launches of before
    cfg = H.tiny_cfg()
    s0 = DecodeSession(C.draft_model(cfg), C.native(), C.prompt(), mask_token_id=cfg.mask_token_id, max_new_tokens=40,
                       max_block_size=16, stop_token_ids=None, temperature=0.0, couple_draft=True)
    s0.prefill()
    draft, names = heads(s0)
    assert {e[0] for e in draft} == {"gemm_argmax"} and "gemm_sample" not in names


def test_decoder_routing(monkeypatch):
    """BatchedDecoder: off, the draft head is gemm_argmax_batch; on, gemm_sample_batch with stream == RNG_TARGET, the
    START word, the decoder's seeds and — with request_temperature — its per-slot invT array; with constrain_draft the new
    op behind it, reading the same seeds and invT."""
    from dflash_amd import ops
    from dflash_amd.batch import BatchedDecoder
    cfg = H.tiny_cfg()
    m, nt = C.draft_model(cfg), C.native()
    prompts = [C.prompt(3, 41), C.prompt(4, 37)]
    log = _spy(monkeypatch, HEADS)

    def draft_calls(**kw):
        dec = BatchedDecoder(m, nt, 2, max_rows=160, out_len=160, mask_token_id=cfg.mask_token_id, temperature=T,
                             sampler="device", **kw)
        for r in range(2):
            dec.admit(r, prompts[r], T if r == 0 else (0.0 if kw.get("request_temperature") else T), seed=5 + r,
                      **(dict(banned_token_ids=[7, 8]) if kw.get("logit_bias") else {}))
        del log[:]
        dec.draft()
        calls = list(log)
        dec.verify()
        dec.accept()
        torch.cuda.synchronize()
        return dec, calls

    _, calls = draft_calls()
    assert [c[0] for c in calls] == ["gemm_argmax_batch"]
    dec, calls = draft_calls(couple_draft=True)
    assert [c[0] for c in calls] == ["gemm_sample_batch"]
    k = calls[0][2]
    assert k["stream"] == ops.RNG_TARGET and k["pos_word"] == ops.DYN_START and k["temperature"] == T
    assert k["seeds"].data_ptr() == dec.seeds.data_ptr() and calls[0][1][5] == 1
    dec, calls = draft_calls(couple_draft=True, request_temperature=True, logit_bias=True, constrain_draft=True)
    assert [c[0] for c in calls] == ["gemm_sample_batch", "grammar_draft_sample_rows"]
    for _, _, k in calls:
        assert k["inv_ts"].data_ptr() == dec.inv_ts.data_ptr() and k["seeds"].data_ptr() == dec.seeds.data_ptr()
    assert calls[1][2]["pos_dyn_word"] == ops.DYN_START
