"""MXFP4 expert weights in the shared MoE pass over 2..4 tiles ("The shared pass"): with expert codes
and expert_stream set, NativeTarget._moe_mlp_shared hands its two grouped launches the layer's ops.Mxfp4Experts instead of
the dequantised bf16 copy.  Every bar is bit-equality: the 4-bit grouped kernels give the bits of the bf16 launch on the
dequantised weights (tests/test_hip_mxfp4_experts_shared_kernels.py), every other launch is the same kernel on the same
bytes.  Models: those of tests/test_hip_fp8_experts_shared.py — hidden 512, 16 experts of 256, top-4, 4 layers (the 64-row
item form) and two layers at hidden 2560, 8 experts of 128, top-6 (hidden > 2048; the 128-row item form)."""
import pytest
import torch

import helpers as H
from test_hip_fp8_experts_shared import GROUPED, KINDS, NAMES, _draft, _gen, _hook_for, _moe_hf, _verify, dev

pytestmark = pytest.mark.gpu
_S = {}


def _case(name):
    if name not in _S:
        from dflash_amd import NativeTarget
        from dflash_amd.synthetic import impose_greedy_walk
        hf = _moe_hf(**KINDS[name])
        perm = impose_greedy_walk(hf, seed=5)          # before the target overwrites hf's experts with the dequantised values
        t = NativeTarget(hf, expert_format="mxfp4")
        assert t.moe_shared_pass and t.expert_stream
        _S[name] = dict(perm=perm, t=t, mlp_only=tuple(KINDS[name].get("mlp_only", ())))
    return _S[name]


def _spy(monkeypatch, log):
    from dflash_amd import ops
    for name in GROUPED + ("moe_gate_up", "moe_down"):
        real = getattr(ops, name)

        def wrapped(w, *a, _real=real, _name=name, **kw):
            log.append((_name, w))
            return _real(w, *a, **kw)
        monkeypatch.setattr(ops, name, wrapped)


def _logged(log, t, mlp_only, stream, passes=1):
    """`passes` shared passes over every MoE layer: both grouped launches, on the layer's own codes or its own copy."""
    from dflash_amd import ops
    want = [(n, lw[k + "4" if stream else k]) for _ in range(passes) for i, lw in enumerate(t.layers) if i not in mlp_only
            for n, k in zip(GROUPED, ("gu_e", "down_e"))]
    assert all(isinstance(w, ops.Mxfp4Experts) == stream for _, w in want)
    return len(log) == len(want) and all(a[0] == b[0] and a[1] is b[1] for a, b in zip(log, want))


@pytest.mark.parametrize("name", ["tiny", "dense1", "h2560"])
def test_wide_verify_streams_the_codes_and_equals_the_copy(name, monkeypatch):
    """A 20- and a 32-row verify, expert_stream on against off: ids, logits, taps and K/V rows are torch.equal; the spy sees
    the layer's Mxfp4Experts in BOTH grouped launches under expert_stream (gate/up too at hidden 2560), the bf16 tensors
    without, and no per-tile expert launch."""
    c = _case(name)
    t = c["t"]
    log = []
    _spy(monkeypatch, log)
    prompt = torch.randint(0, 2000, (1, 29), generator=_gen(5)).to(dev())
    taps = [0] if name == "h2560" else [0, 2]
    try:
        for bs in (20, 32):
            block = torch.randint(0, 2000, (bs,), generator=_gen(100 + bs)).to(dev())
            runs = {}
            for stream in (True, False):
                t.expert_stream = stream
                del log[:]
                runs[stream] = _verify(t, prompt, block, taps)
                assert _logged(log, t, c["mlp_only"], stream), (bs, stream, [a for a, _ in log])
            same = dict(zip(NAMES, (torch.equal(x, y) for x, y in zip(runs[True], runs[False]))))
            assert all(same.values()), (bs, same)
    finally:
        t.expert_stream = True
    assert t._moe_sh["sc"]["rows_per_item"] == (128 if name == "h2560" else 64)


def test_batch_of_three_streams_the_codes_eager_and_replayed(monkeypatch):
    """BatchedDecoder with 3 requests, eight cycles eager and eight replayed, expert_stream on against off: the same
    acceptance lengths and committed ids (the walk), and rows bit for bit between the arms of one launch form.  The
    captured verify holds the code launches: the spy sees them during the capture, replays launch nothing from the host."""
    from dflash_amd.batch import BatchedDecoder
    from dflash_amd.synthetic import greedy_walk
    c = _case("tiny")
    t, R = c["t"], 3
    prompts = [torch.randint(0, 2000, (1, P), generator=_gen(60 + i)).to(dev()) for i, P in enumerate((30, 47, 12))]
    Gs = [greedy_walk(c["perm"], p, 240).to(dev()) for p in prompts]
    cfg, m = _draft()
    hooks = [_hook_for(Gs[i], H.make_plan(64, 16, 17 + i)) for i in range(R)]
    hook = lambda r, b, s, k: hooks[r](b, s, k)  # noqa: E731
    log = []
    _spy(monkeypatch, log)
    runs = {}
    try:
        for stream in (True, False):
            t.expert_stream = stream
            for use_graph in (False, True):
                dec = BatchedDecoder(m, t, R, max_rows=320, out_len=320, mask_token_id=cfg.mask_token_id)
                for r in range(R):
                    dec.admit(r, prompts[r])
                del log[:]
                taus = [dec.cycle(hook)]
                assert _logged(log, t, (), stream), (stream, [a for a, _ in log])
                if use_graph:
                    del log[:]
                    dec.capture()
                    assert _logged(log, t, (), stream), (stream, "capture")
                    del log[:]
                taus += [(dec.cycle_graph if use_graph else dec.cycle)(hook) for _ in range(8)]
                assert not use_graph or log == []
                torch.cuda.synchronize()
                for r in range(R):
                    assert torch.equal(dec.output_ids[r, :dec.start[r] + 1], Gs[r][:dec.start[r] + 1]), (stream, use_graph, r)
                runs[stream, use_graph] = (taus, list(dec.start), dec.output_ids.clone(), dec.post.clone(), dec.d["taps"].clone(),
                                           dec.tk.clone(), dec.tv.clone())
                del dec
    finally:
        t.expert_stream = True
    ref = runs[False, False]
    assert max(x[0] for cyc in ref[0] for x in cyc if x is not None) > 8
    for key, run in runs.items():
        assert run[0] == ref[0] and run[1] == ref[1] and torch.equal(run[2], ref[2]), key
    for use_graph in (False, True):     # (a replayed attention launch splits its keys elsewhere than an eager one)
        for x, y, what in zip(runs[True, use_graph][2:], runs[False, use_graph][2:], ("ids", "posterior", "taps", "K", "V")):
            assert torch.equal(x, y), (use_graph, what)
