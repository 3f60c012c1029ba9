"""NativeTarget(expert_format="mxfp4") on the GPU ("The experts"), on a tiny Qwen3MoeForCausalLM (hidden
512, 16 experts of 256, top-4, 4 layers), once with a dense layer in between."""
import pytest
import torch

import helpers as H
from test_hip_fp8_experts import KINDS, NAMES, _draft, _gen, _hook_for, _moe_hf, _verify, dev

pytestmark = pytest.mark.gpu
_S = {}


def _case(name):
    """The greedy walk is imposed BEFORE the target is constructed; the target then overwrites hf's expert tensors."""
    if name not in _S:
        from dflash_amd import NativeTarget
        from dflash_amd.synthetic import impose_greedy_walk
        hf = _moe_hf(**KINDS[name])
        perm = impose_greedy_walk(hf, seed=5)
        before = {k: v.clone() for k, v in hf.state_dict().items() if "mlp.experts" in k}
        _S[name] = dict(hf=hf, perm=perm, before=before, nt4=NativeTarget(hf, expert_format="mxfp4"))
    return _S[name]


def _spy(monkeypatch, log):
    from dflash_amd import ops
    for name in ("moe_gate_up", "moe_down"):
        real = getattr(ops, name)

        def wrapped(w, *a, _real=real, _name=name, **kw):
            log.append((_name, isinstance(w, ops.Mxfp4Experts)))
            return _real(w, *a, **kw)
        monkeypatch.setattr(ops, name, wrapped)


@pytest.mark.parametrize("name", ["tiny", "dense1"])
def test_mxfp4_expert_verify(name, monkeypatch):
    """The caller's experts hold dequantize(quantize(original)); expert_stream off is bit-equal to a bf16 NativeTarget of that
    overwritten model; stream on against off is torch.equal on ids, logits, taps and K/V rows at 16 and 11 rows; the spy shows
    both expert launches of every MoE layer taking the codes."""
    from dflash_amd import NativeTarget, ops
    c = _case(name)
    t, hf = c["nt4"], c["hf"]
    n_moe = t.L - len(KINDS[name].get("mlp_only", ()))
    assert t.expert_format == "mxfp4" and t.experts8 is None and [x is not None for x in t.experts4].count(True) == n_moe
    assert len(t.fp8_tensors()) == 4 * n_moe and not any("gu_e13" in lw for lw in t.layers)   # (no 13-bit expert twin)
    sd = hf.state_dict()
    for k, v in c["before"].items():
        q, sc = ops.quantize_mxfp4_rows(v.view(-1, v.shape[2]))
        assert torch.equal(sd[k], ops.dequantize_mxfp4_rows(q, sc).view_as(v)) and not torch.equal(sd[k], v), k
    ntb = NativeTarget(hf)
    log = []
    _spy(monkeypatch, log)
    prompt = torch.randint(0, 2000, (1, 37), generator=_gen(4)).to(dev())
    try:
        for bs in (16, 11):
            block = torch.randint(0, 2000, (bs,), generator=_gen(100 + bs)).to(dev())
            runs = {}
            for stream in (True, False):
                t.expert_stream = stream
                del log[:]
                runs[stream] = _verify(t, prompt, block, [0, 2])
                assert log == [("moe_gate_up", stream), ("moe_down", stream)] * n_moe, (stream, log)
            (a, ra), (b, rb), (p, _) = runs[True], runs[False], _verify(ntb, prompt, block, [0, 2])
            for x, y, z, what in zip(a, b, p, NAMES):
                assert torch.equal(y, z), (bs, what, "the copy against a bf16 target")
                assert torch.equal(x, y), (bs, what, "stream on against off")
            assert len(ra) == n_moe and all(i == j and torch.equal(x, y) for (i, x), (j, y) in zip(ra, rb))
    finally:
        t.expert_stream = True


def test_mxfp4_expert_loops_commit_the_walk_in_both_arms(monkeypatch):
    """dflash_generate eager and replayed at 16 rows and a 20-row block (the shared pass, on the bf16 copy), codes and copy."""
    from dflash_amd import dflash_generate
    from dflash_amd.synthetic import greedy_walk
    c = _case("tiny")
    t = c["nt4"]
    cfg, m = _draft()
    prompt = torch.randint(0, 2000, (1, 30), generator=_gen(60)).to(dev())
    n_new, P = 60, 30
    G = greedy_walk(c["perm"], prompt, 120).to(dev())
    want = G[:P + n_new].tolist()
    acc = {}
    try:
        for stream in (True, False):
            t.expert_stream = stream
            for mode, bs in (("0", 16), ("1", 16), ("1", 20)):
                monkeypatch.setenv("DFL_GRAPH", mode)
                r = dflash_generate(m, t, prompt, cfg.mask_token_id, n_new, bs, None, 0.0,
                                    draft_token_hook=_hook_for(G, H.make_plan(64, bs, 17)))
                assert r.output_ids[0].tolist() == want, (stream, mode, bs)
                if bs == 16:
                    assert (r.replayed_cycles > 0) == (mode == "1"), (stream, mode)
                acc[stream, mode, bs] = r.acceptance_lengths
    finally:
        t.expert_stream = True
    assert all(acc[True, m_, b] == acc[False, m_, b] for _, m_, b in acc)
    assert max(acc[True, "1", 16]) > 8 and max(acc[True, "1", 20]) > 16
