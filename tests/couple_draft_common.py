"""What the two GPU test files of the coupled draft share: the soft walk target, prompts and teacher-forced audit of
tests/test_hip_sampling.py (copied, with the temperature a parameter), and a recorded single-request run — every hook
call with the block as the hook saw it, a clone of the session's materialised draft logits, and how the draft was
launched."""
import numpy as np
import torch

import helpers as H
import sampling_ref as SR

BF16 = torch.bfloat16
V = 2048
T = 0.7
_STATE = {}


def dev():
    return torch.device("cuda", 0)


def walk_target(scale=0.62):
    """tests/test_hip_sampling.py::_walk_target: the walk's next token keeps probability ~0.75 - 0.8 at T = 0.7."""
    if "hf" not in _STATE:
        from dflash_amd.synthetic import impose_greedy_walk, make_hf_qwen3
        torch.manual_seed(11)
        hf = make_hf_qwen3({**H.TINY_TARGET, "num_layers": 6}, dev(), dtype=BF16)
        perm = impose_greedy_walk(hf, seed=8)
        with torch.no_grad():
            hf.lm_head.weight.mul_(scale)
        _STATE["hf"], _STATE["perm"] = hf, perm.cpu().tolist()
    return _STATE["hf"], _STATE["perm"]


def native():
    from dflash_amd import NativeTarget
    return NativeTarget(walk_target()[0])


def draft_model(cfg=None):
    from dflash_amd import DFlashDraftModel
    cfg = cfg or H.tiny_cfg()
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
    return m


def prompt(seed=3, n=41):
    return torch.randint(0, 2000, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev())


def script(sizes=(8, 12, 16)):
    """tests/test_hip_sampling.py::_script: the policy loop with a scripted choice of block size."""
    from dflash_amd.generate import _Fixed
    a, b, c = sizes

    class Script(_Fixed):
        def select(self, cyc):
            return (c, a, b, c, b, a)[cyc % 6]

    s = Script(c)
    s.candidates = tuple(sizes)
    return s


def audit(ids, n_in, seed, temperature=T, gap=0.1, keep=0.90):
    """Teacher-forced: every emitted token is the target's seeded draw (mirror noise at its position) wherever the
    perturbed top-2 gap exceeds `gap`; at least `keep` of the positions pass the screen.  Returns (emitted, screen)."""
    hf, _ = walk_target()
    with torch.inference_mode():
        logits = hf(torch.tensor([ids], device=dev())).logits[0].float().cpu().numpy()
    pos = np.arange(n_in, len(ids))
    exp, gaps = SR.draw(SR.bf16_round(logits[pos - 1]), temperature, seed, SR.TARGET, pos)
    safe = gaps > gap
    got = np.asarray(ids)[pos]
    print(f"[couple draft] audit: T {temperature} seed {seed} positions {len(pos)} kept {safe.mean():.3f}")
    assert safe.mean() >= keep, safe.mean()
    assert np.array_equal(got[safe], exp[safe]), np.nonzero(got[safe] != exp[safe])
    return got, safe


def same_until_a_near_tie(a, b, what=""):
    """Two audited runs of one request: a divergence may only start at a position either screen left out."""
    (ga, sa), (gb, sb) = a, b
    n = min(len(ga), len(gb))
    diff = np.nonzero(ga[:n] != gb[:n])[0]
    if diff.size:
        assert not (sa[diff[0]] and sb[diff[0]]), (what, diff[0])
    return diff.size == 0


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


class Rec:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def recorded_run(monkeypatch, *, graph=True, run_ahead=True, kind="fixed", bs=16, seed=5, n_new=100, temperature=T,
                 prompt_ids=None, **kw):
    """dflash_generate / dflash_generate_policy at T > 0 with sampler="device" and a logging-only hook.  The session gets
    a draft-logits buffer (where constrain_draft has not made one) before its first cycle.  Returns (result, one Rec per
    hook call: start, bs, seen = the block, x = the draft logits' bits [16 or 32, V], ahead = the draft was taken from a
    run-ahead launch, state = the grammar state at that moment or -1; replayed flag per cycle with a draft)."""
    from dflash_amd import dflash_generate, dflash_generate_policy, generate
    monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
    monkeypatch.setenv("DFL_RUN_AHEAD", "1" if run_ahead else "0")
    sessions, ahead, recs, flags = [], [False], [], []
    if "reals" not in _STATE:
        _STATE["reals"] = (generate.DecodeSession.__init__, generate.DecodeSession._take_ahead, generate.DecodeSession._commit)
    real_init, real_take, real_commit = _STATE["reals"]

    def init(self, *a, **k):
        real_init(self, *a, **k)
        if self.draft_logits is None:
            self.draft_logits = torch.zeros(32, V, dtype=BF16, device=dev())
        sessions.append(self)

    def take(self, blk):
        ahead[0] = True
        return real_take(self, blk)

    def commit(self, res, b, start, rows, replayed):
        if b > 1:
            flags.append(bool(replayed))
        return real_commit(self, res, b, start, rows, replayed)

    monkeypatch.setattr(generate.DecodeSession, "__init__", init)
    monkeypatch.setattr(generate.DecodeSession, "_take_ahead", take)
    monkeypatch.setattr(generate.DecodeSession, "_commit", commit)

    def hook(blk, start, call):
        s = sessions[-1]
        torch.cuda.synchronize()
        rows = 16 * ((blk.shape[1] + 15) // 16)
        recs.append(Rec(start=int(start), bs=int(blk.shape[1]), seen=blk[0].cpu().numpy().copy(),
                        x=bits(s.draft_logits[:rows].clone()), ahead=ahead[0],
                        state=int(s.gr.state.item()) if s.gr is not None else -1))
        ahead[0] = False

    cfg = H.tiny_cfg()
    p = prompt() if prompt_ids is None else prompt_ids
    try:
        if kind == "fixed":
            r = dflash_generate(draft_model(cfg), native(), p, cfg.mask_token_id, n_new, bs, None, temperature,
                                draft_token_hook=hook, sampler="device", seed=seed, **kw)
        else:
            r = dflash_generate_policy(model=draft_model(cfg), target=native(), input_ids=p, mask_token_id=cfg.mask_token_id,
                                       max_new_tokens=n_new, stop_token_ids=None, temperature=temperature,
                                       scheduler=script(), draft_token_hook=hook, sampler="device", seed=seed, **kw)
    finally:
        for name, fn in zip(("__init__", "_take_ahead", "_commit"), _STATE["reals"]):
            monkeypatch.setattr(generate.DecodeSession, name, fn)
        # (monkeypatch keeps the patched methods, and with them this list, until the test's teardown: let go of the
        # session and its hipGraphs here, so that the `graphs` fixture of the calling test can collect them)
        sessions.clear()
    return r, recs, flags
