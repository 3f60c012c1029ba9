"""The coupled draft draw without a GPU: the mirror's match rate against the closed form, the
keyword and its refusals, and the refusals of dfl_grammar_draft_sample_rows."""
import inspect
import math

import numpy as np
import pytest

import couple_draft_ref as CD
import grammar_draft_ref as GD
import grammar_ref as GR
import sampling_ref as S

V, N, SEED = 48, 6000, 20260117


def _pair(kind: str):
    """Target and draft logits (bf16-valued fp32 [V]): q = p, a mild and a strong perturbation."""
    rng = np.random.default_rng(5)
    x = S.bf16_round((rng.standard_normal(V) * 2).astype(np.float32))
    sigma = dict(same=0.0, mild=0.5, strong=3.0)[kind]
    y = S.bf16_round((x + sigma * rng.standard_normal(V)).astype(np.float32))
    return x, y


def _ids(x, seed, positions, stream=S.TARGET, extra=0):
    z = S.perturbed(np.broadcast_to(x, (len(positions), V)), 0.7, seed, stream, positions, extra)
    return z.argmax(axis=1)



@pytest.mark.parametrize("kind", ["same", "mild", "strong"])
def test_match_rate_meets_the_closed_form(kind):
    """N positions of one request: the target's draw of position p and the coupled draft's pick for it share g(seed,
    TARGET, p, v, 0); their match rate lies within 4 sigma of sum_i 1 / sum_j max(p_j / p_i, q_j / q_i)."""
    x, y = _pair(kind)
    P = CD.match_probability(CD.softmax(x, 0.7), CD.softmax(y, 0.7))
    pos = np.arange(100, 100 + N)
    rate = float((_ids(x, SEED, pos) == _ids(y, SEED, pos)).mean())
    bound = 4 * math.sqrt(P * (1 - P) / N)
    print(f"{kind}: closed form {P:.4f}, measured {rate:.4f}, bound {bound:.4f}")
    assert abs(rate - P) <= bound, (kind, P, rate, bound)
    if kind == "same":
        assert P == pytest.approx(1.0, abs=1e-12) and rate == 1.0
    else:
        assert P >= (1 - _tv(x, y)) / (1 + _tv(x, y)) - 1e-12          # the lower bound of the coupling
        greedy = float(CD.softmax(x, 0.7)[int(np.argmax(y))])        # what a greedy draft is accepted with
        own = float((CD.softmax(x, 0.7) * CD.softmax(y, 0.7)).sum())   # a draft drawn on its own stream
        assert own < P
        print(f"{kind}: greedy draft {greedy:.4f}, own-noise draft {own:.4f}")


def _tv(x, y):
    return 0.5 * float(np.abs(CD.softmax(x, 0.7) - CD.softmax(y, 0.7)).sum())


def test_same_logits_pick_the_targets_draw_and_the_draft_stream_does_not():
    """q = p: slot j of the block at `start` and verify row j - 1 agree for every j; the DRAFT-stream draw of the policy
    loop (extra = start) does not; neither does a pick one position off."""
    rng = np.random.default_rng(9)
    for start in (40, 1039):
        lg = S.bf16_round((rng.standard_normal((16, V)) * 2).astype(np.float32))
        tgt, _ = CD.target_draw(lg[1:], 0.7, SEED, start, 15)         # row r holds the logits of position start + r + 1
        cpl, _ = CD.draw(lg, 0.7, SEED, start, 16)
        own, _ = CD.draw(lg, 0.7, SEED, start, 16, stream=S.DRAFT)
        off, _ = CD.draw(lg, 0.7, SEED, start + 1, 16)
        assert np.array_equal(cpl[1:], tgt)
        assert (own[1:] != tgt).sum() >= 5 and (off[1:] != tgt).sum() >= 5


def test_noise_pick_mirror_is_the_sibling_at_inv_t_zero_and_walks_the_automaton():
    rng = np.random.default_rng(2)
    Vg = 256
    pool = GR.case_dfa(rng, 6, Vg, 0.4)
    x = GR.case_rows(rng, 16, Vg)
    blk = np.full(16, -7, np.int64)
    plain = GD.pick(x, 16, blk, pool, 0, 2)
    for inv in (0.0, -1.0, float("nan")):
        got = CD.pick(x, 16, blk, seed=3, inv_t=inv, pos0=50, pool=pool, base=0, state=2)
        assert np.array_equal(got[0], plain[0]) and got[1] == plain[1]
    out, states, gaps = CD.pick(x, 16, blk, seed=3, inv_t=S.inv_t(0.7), pos0=50, pool=pool, base=0, state=2)
    assert len(states) == 16 and GR.walk(pool, 0, 2, out[1:]) == states[-1] >= 0
    assert (out != plain[0]).any()                                     # the noise moves some pick
    # the unconstrained slot of the same position, where its pick is legal, is that pick
    free, _ = CD.draw(GR.bits_to_f32(x), 0.7, 3, 50, 2)
    if pool[2, free[1]] >= 0 and not np.isnan(GR.bits_to_f32(x)[1]).all():
        assert out[1] == free[1]


# ------------------------------------------------------------------------------------------------------ the public keyword
def _entries():
    from dflash_amd import batch, engine, generate, model
    return [generate.DecodeSession.__init__, generate.run_decode, generate.dflash_generate, generate.dflash_generate_policy,
            model.DFlashDraftModel.spec_generate, batch.BatchedDecoder.__init__, batch.dflash_generate_batch,
            engine.BatchEngine.__init__, engine.dflash_generate_stream]


def test_couple_draft_is_a_keyword_of_every_entry_and_off_by_default():
    from dflash_amd import batch, candidates
    for fn in _entries():
        p = inspect.signature(fn).parameters
        assert "couple_draft" in p and p["couple_draft"].default is False, fn
    assert "couple_draft" not in inspect.signature(batch.dflash_generate_policy_batch).parameters
    for name, fn in inspect.getmembers(candidates, inspect.isfunction):
        assert "couple_draft" not in inspect.signature(fn).parameters, name


def test_refusals_need_no_gpu():
    from dflash_amd import batch, generate
    chk = generate.check_couple_draft
    assert chk(False, 0.7, None, "torch") == 0.0 and chk(False, 0.7, 0.7, "torch") == 0.7     # off: nothing is asked
    assert chk(True, 0.0, None, "torch") == 0.0                                               # T = 0: nothing to share
    assert chk(True, 0.7, None, "device") == 0.0 and chk(True, 0.7, 0.7, "device") == 0.7
    with pytest.raises(ValueError, match="sampler='device'"):
        chk(True, 0.7, None, "torch")
    with pytest.raises(ValueError, match="draft_temperature"):
        chk(True, 0.7, 0.5, "device")
    with pytest.raises(ValueError, match="draft_temperature"):
        chk(True, 0.7, 0.0, "device")
    # the constructors ask before they touch the model, the target or the GPU
    kw = dict(mask_token_id=0, max_new_tokens=4, max_block_size=16, stop_token_ids=None)
    with pytest.raises(ValueError, match="sampler='device'"):
        generate.DecodeSession(None, None, None, temperature=0.7, sampler="torch", couple_draft=True, **kw)
    with pytest.raises(ValueError, match="draft_temperature"):
        generate.DecodeSession(None, None, None, temperature=0.7, draft_temperature=0.3, sampler="device",
                               couple_draft=True, **kw)
    with pytest.raises(ValueError, match="sampler='device'"):
        batch.BatchedDecoder(None, None, 2, 64, 64, 0, temperature=0.7, sampler="torch", couple_draft=True)
    with pytest.raises(ValueError, match="draft_temperature"):
        batch.BatchedDecoder(None, None, 2, 64, 64, 0, temperature=0.7, sampler="device", draft_temperature=0.3,
                             couple_draft=True)


# ------------------------------------------------------------------------------------------------------- the C entry point
def test_entry_point_refusals_need_no_gpu():
    from dflash_amd import _lib
    h = _lib.lib()

    def refused(word, *args):
        assert h.dfl_grammar_draft_sample_rows(*args) == -22
        msg = h.dfl_last_error()
        assert b"dfl_grammar_draft_sample_rows:" in msg and word in msg, msg

    ok = dict(logits=256, ld=64, tile_stride=1024, tiles=2, V=64, nrows=16, dyn=512, word=-1, table=256, tstride=64,
              pool=4, base=16, state=16, bias=256, bstride=64, block=16, blkstride=16, seeds=32, inv_t=1.0, inv_ts=None,
              pos_word=-1, pos_base=0, stream=None)

    def call(**kw):
        return tuple({**ok, **kw}.values())

    refused(b"null", *call(logits=None))
    refused(b"null", *call(block=None))
    refused(b"null", *call(table=None, bias=None))
    refused(b"null", *call(state=None))
    refused(b"seeds", *call(seeds=None))
    refused(b"V=60", *call(V=60))
    refused(b"bad shape", *call(ld=60))
    refused(b"bad shape", *call(logits=264))
    refused(b"bad shape", *call(tile_stride=512))
    refused(b"table_stride", *call(tstride=60))
    refused(b"bias_stride", *call(bstride=32))
    refused(b"nrows=17", *call(nrows=17))
    refused(b"nrows_dyn_word", *call(word=2, dyn=None))
    refused(b"block_stride", *call(blkstride=8))
    refused(b"pos_dyn_word=9", *call(pos_word=9))
    refused(b"pos_dyn_word=3", *call(pos_word=3, dyn=None))
    refused(b"pos_base=-1", *call(pos_base=-1))
    # nothing to launch: no tile, or a block without a draft token
    assert h.dfl_grammar_draft_sample_rows(*call(tiles=0)) == 0
    assert h.dfl_grammar_draft_sample_rows(*call(nrows=1)) == 0
    # the sibling keeps its own name in its refusals
    assert h.dfl_grammar_draft_rows(*call(V=60)[:17], None) == -22 and b"dfl_grammar_draft_rows:" in h.dfl_last_error()
