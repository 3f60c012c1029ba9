"""Where the hot kernels' launch arguments come from (kernarg preload, csrc/gemm_skinny.hip "the head of the launch
arguments"): the compiler keeps delivering the head in SGPRs, and a launch replayed from a hipGraph reads its own head."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dflash_amd", "csrc")
BF16 = torch.bfloat16

# (source file, kernel-name prefix in the demangled symbol, macro with the number of head dwords the source declares)
# (k_attn_head* declares no head yet: DESIGN.md 5b; its row goes here with the macro when it does)
HEADS = [("gemm_skinny.hip", "k_gemm", "GEMM_HEAD_DWORDS")]


def _preload_lengths(src, tmp_path):
    """{mangled kernel name: .amdhsa_user_sgpr_kernarg_preload_length} of one source, compiled with build.py's flags."""
    from dflash_amd.build import FLAGS, _hipcc
    hipcc = _hipcc()
    if not (os.path.isabs(hipcc) and os.path.exists(hipcc)) and shutil.which(hipcc) is None:
        pytest.skip("hipcc not found")
    out = os.path.join(str(tmp_path), src.replace(".hip", ".s"))
    subprocess.run([hipcc, *FLAGS, "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out], check=True,
                   capture_output=True)
    lengths, name = {}, None
    for line in open(out):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", line)
        if m and name:
            lengths[name] = int(m.group(1))
        if ".end_amdhsa_kernel" in line:
            lengths.setdefault(name, 0)   # (no directive at all: nothing is preloaded)
            name = None
    return lengths


@pytest.mark.parametrize("src,prefix,macro", HEADS)
def test_kernarg_preload_covers_the_declared_head(src, prefix, macro, tmp_path):
    """Every kernel of the family reports a preload length of at least the head the source declares: one more field in
    front of the head, or a struct moved to the first position, would switch the mechanism off without any other sign."""
    m = re.search(r"#define\s+%s\s+(\d+)" % macro, open(os.path.join(CSRC, src)).read())
    assert m, f"{src} declares no {macro}"
    need = int(m.group(1))
    assert 1 <= need <= 14
    lengths = _preload_lengths(src, tmp_path)
    # Itanium mangling: <length><name>, then I (template arguments) or E — "6k_gemmI", "8k_gemm_sI", "13k_attn_head32E"
    fam = {k: v for k, v in lengths.items() if re.search(r"\d+%s[a-z0-9_]*[IE]" % prefix, k)}
    assert len(fam) >= 2, sorted(lengths)
    short = {k: v for k, v in fam.items() if v < need}
    assert not short, f"kernels preloading fewer than {need} dwords: {short}"


@pytest.mark.gpu
def test_replayed_launches_keep_their_own_arguments():
    """Three back-to-back launches of ONE k_gemm instantiation with different argument blocks (one with a row count
    from the device record, one whose tile assignment depends on the grid-size argument) and one attention launch with
    lengths from the record, captured into one hipGraph and replayed twice with the record rewritten in between: after
    each replay every output equals eager launches on the same inputs, bit for bit."""
    from dflash_amd import ops
    from dflash_amd.generate import capture_graph
    from dflash_amd.model import _rope_tables
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(77)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(BF16).to(dev)

    shapes = [(32, 512, -1), (48, 512, ops.DYN_BS), (32, 256, -1)]   # (N, K, valid_word); 48 = three whole tiles
    wps = [ops.pack_weight(rnd(n, k, scale=k ** -0.5)) for n, k, _ in shapes]
    xs = [rnd(16, k) for _, k, _ in shapes]
    h0 = [rnd(16, n) for n, _, _ in shapes]
    n_q = n_kv = 1   # the smallest head counts the launcher takes
    S, bs = 40, 16
    ld = (n_q + 2 * n_kv) * 128
    xq = rnd(16, ld)
    qw, kw = (1 + 0.1 * torch.randn(128, generator=g)).to(BF16).to(dev), (1 + 0.1 * torch.randn(128, generator=g)).to(BF16).to(dev)
    cos, sin = _rope_tables(128, 1e6, 256, dev)
    k0, v0 = rnd(n_kv, S + bs + 8, 128), rnd(n_kv, S + bs + 8, 128)
    dyn = torch.zeros(8, dtype=torch.int32, device=dev)

    class Bufs:
        def __init__(self):
            self.h = [t.clone() for t in h0]
            self.ss = [torch.zeros(n, dtype=torch.float32, device=dev) for n, _, _ in shapes]
            self.k, self.v = k0.clone(), v0.clone()
            self.out = torch.zeros(16 * n_q * 128, dtype=BF16, device=dev)
            self.ws = ops.attn_head_ws(n_q, 8, 1, dev)

        def reset(self):
            for t, s in zip(self.h, h0):
                t.copy_(s)
            for t in self.ss:
                t.fill_(-1.0)
            self.k.copy_(k0)
            self.v.copy_(v0)
            self.out.fill_(float("nan"))

        def launch(self):
            for (n, k, vw), wp, x, h, ss in zip(shapes, wps, xs, self.h, self.ss):
                ops.gemm_resid(wp, ops.rows_plain(x, vw), n, k, h, add_residual=True, ss_out=ss, dyn=dyn)
            ops.attn_head(xq=xq, q_col=0, k_col=n_q * 128, v_col=(n_q + n_kv) * 128, n_q=n_q, n_kv=n_kv, q_norm_w=qw,
                          k_norm_w=kw, eps=1e-6, cos_tab=cos, sin_tab=sin, kcache=self.k, vcache=self.v, scale=128 ** -0.5,
                          causal=True, S=S, tau=0, bs=bs, pos0=S, dyn=dyn, ws=self.ws, max_splits=8, out_frag=self.out)

        def tensors(self):
            return [*self.h, *self.ss, self.k, self.v, self.out]

    eager, replayed = Bufs(), Bufs()
    ops.set_dyn(dyn, S, 0, 5, S)
    replayed.launch()                       # (first launches load the code objects: not inside a capture)
    torch.cuda.synchronize()
    graph = capture_graph(replayed.launch)
    for s_now, bs_now in ((S, 5), (33, 9)):  # the row count word is 5 in the first replay
        ops.set_dyn(dyn, s_now, 0, bs_now, s_now)
        eager.reset()
        replayed.reset()
        eager.launch()
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(eager.tensors(), replayed.tensors())):
            assert torch.equal(a.view(torch.int16) if a.dtype == BF16 else a, b.view(torch.int16) if b.dtype == BF16 else b), \
                f"tensor {i} differs after the replay with S={s_now} bs={bs_now}"
        # the launches did something: rows past the count of the dyn-counted launch add nothing, valid rows do
        assert torch.equal(eager.h[1][bs_now:], h0[1][bs_now:]) and not torch.equal(eager.h[1][:bs_now], h0[1][:bs_now])
        assert torch.isfinite(eager.out.float()).any() and not torch.equal(eager.k, k0)
