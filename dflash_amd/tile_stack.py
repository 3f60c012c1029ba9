"""`TileStack` — a decoder stack over 16-row tiles on the ragged-batch kernels, the one place THIS kernel family's layer
sequence lives.  There are two stacks, one per family: a single request's block on the skinny kernels (one tile, or two
in two passes) runs through row_stack.RowStack, whose partial-sum and norm protocol is another.

Every caller that pushes several 16-row tiles through a stack in ONE pass over the weights runs it through here: the
requests of a ragged batch (draft and target side, batch.py), the two tiles of a 17..32-row block (model.py,
target.py), the candidate blocks of one verify (candidates.py).  Per layer:

    norm_frag_batch(ln1, + the sums that wait in part_h)  ->  q/k/v GEMM  ->  the caller's attention launch  ->
    gemm_f32_batch(o)  ->  norm_frag_batch(ln2, + o's sums)  ->  gate/up + SiLU, gemm_f32_batch(down)   | the MoE MLP

o_proj and down_proj (or the experts) leave fp32 partial sums in `part_h`; the residual add happens in the norm launch
that follows, so a layer's output — and with it a tapped layer's rows — exists only after the NEXT norm launch.  What
waits between two launches (the K of the pending sums or their share count, the pending tap) is kept here and nowhere
else.  Callers differ in the attention launch they hand in and in what surrounds the stack (embedding, lm_head).
"""
from __future__ import annotations

import torch

from . import ops

BF16, F32 = torch.bfloat16, torch.float32


def gemm_ws(H: int, widths, depths, device) -> torch.Tensor:
    """Workspace of the ragged-batch GEMMs that serves every (N, K = H) with N in widths and (N = H, K) with K in depths
    (the caller lists its own: the lm_head's vocabulary and whatever else it launches with this workspace)."""
    lib = ops.lib()
    return torch.zeros(max(lib.dfl_gemm_batch_ws_bytes(max(widths), H), lib.dfl_gemm_batch_ws_bytes(H, max(depths))),
                       dtype=torch.uint8, device=device)


class TileStack:
    def __init__(self, *, H: int, q_dim: int, I: int, nqkv: int, eps: float, MT: int, gws: torch.Tensor, h=None, attn=None,
                 act=None, xq=None, part_qkv: bool = False, moe_nsplit: int = 0):
        """MT tile slots.  h [MT, 16, H], attn [MT, 16 * q_dim], act [MT, 16 * I], xq [MT, 16, nqkv]: the buffers a caller
        shares with its single-request path, adopted; allocated here when not given.  part_qkv: also the fp32 K-part
        buffer of the q/k/v GEMM (qkv="parts").  moe_nsplit: the most expert shares an MoE layer leaves in part_h."""
        self.H, self.q_dim, self.I, self.nqkv, self.eps, self.MT, self.gws = H, q_dim, I, nqkv, eps, MT, gws
        ks = ops.batch_ksplit
        z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=gws.device)  # noqa: E731
        self.h = z(MT, 16, H) if h is None else h
        self.attn = z(MT, 16 * q_dim) if attn is None else attn
        self.act = z(MT, 16 * I) if act is None else act
        self.xq = z(MT, 16, nqkv) if xq is None else xq
        self.xn = z(MT, 16 * H)
        self.part_h = z(max(ks(q_dim), ks(I), moe_nsplit) * MT * 16 * H, dt=F32)
        self.part_qkv = z(ks(H) * MT * 16 * nqkv, dt=F32) if part_qkv else None
        self.src = dict(xn=ops.brows_frag(self.xn), attn=ops.brows_frag(self.attn), act=ops.brows_frag(self.act))
        self._pend = None   # between run() and finish(): (R, dyn, K, share count, tap slots, tap rows)

    def _norm(self, norm_w) -> None:
        """The norm launch that opens a layer or closes the stack: adds the pending sums to the residual stream, writes the
        pending tap — the slots of a repeated tap id (build_target_layer_ids repeats layers for shallow targets,
        model/utils.py:16-25) get copies — and leaves the normalised rows in xn."""
        R, dyn, K, ns, sl, taps = self._pend
        H = self.H
        tap = taps[:, :, sl[0] * H:(sl[0] + 1) * H] if sl else None
        ops.norm_frag_batch(self.h, R, norm_w, self.eps, self.xn, dyn, ops.DYN_BS, part=self.part_h if K or ns else None,
                            N=H, K=K, tap=tap, nsplit=ns)
        for b in sl[1:]:
            taps[:, :, b * H:(b + 1) * H].copy_(tap)

    def run(self, layers, R: int, dyn, attend, *, qkv: str, taps=None, tap_layers=(), moe=None) -> None:
        """The layers over tiles 0..R-1 of h (embedded rows; dyn [MT, 8]: the tiles' length records).  Leaves the last
        layer's sums pending: finish() follows.
        attend(i, lw): the caller's attention launch of layer i, from the q/k/v this leaves in xq (qkv="rows": finished
        bf16 rows) or part_qkv (qkv="parts": fp32 K-part sums) to frag16 rows in attn.
        taps [tiles, 16, len(tap_layers) * H]: receives the output rows of the layers in tap_layers.
        moe(lw, R, MT, dyn, xn, part_h) -> share count: the MLP of a layer with experts (NativeTarget.moe_mlp_tiles)."""
        H, s = self.H, self.src
        tl = list(tap_layers)
        if tl and max(tl) >= len(layers) - 1:
            raise NotImplementedError("tapping the last layer (post-norm state) is not supported")
        slots = {}   # tapped layer -> its slots in the tap rows
        for j, l in enumerate(tl):
            slots.setdefault(l, []).append(j)
        self._pend = (R, dyn, 0, None, (), taps)
        for i, lw in enumerate(layers):
            self._norm(lw["ln1"])
            if qkv == "parts":
                ops.gemm_f32_batch(lw["qkv"], s["xn"], R, self.nqkv, H, self.part_qkv, dyn)
            else:
                ops.gemm_resid_batch(lw["qkv"], s["xn"], R, self.nqkv, H, self.xq, add_residual=False, ws=self.gws, dyn=dyn)
            attend(i, lw)
            ops.gemm_f32_batch(lw["o"], s["attn"], R, H, self.q_dim, self.part_h, dyn)
            ops.norm_frag_batch(self.h, R, lw["ln2"], self.eps, self.xn, dyn, ops.DYN_BS, part=self.part_h, N=H,
                                K=self.q_dim)
            if "gu_e" in lw:   # sparse-MoE layer: the tiles share attention and projections, each routes its own rows
                K, ns = 0, moe(lw, R, self.MT, dyn, self.xn, self.part_h)   # expert shares, not K parts
            else:
                ops.gemm_silu_mul_batch(lw["gu"], s["xn"], R, self.I, H, self.act, self.gws, dyn)
                ops.gemm_f32_batch(lw["down"], s["act"], R, H, self.I, self.part_h, dyn)
                K, ns = self.I, None
            self._pend = (R, dyn, K, ns, slots.get(i, ()), taps)

    def finish(self, norm_w) -> None:
        """The last layer's sums and the final norm: xn (src["xn"]) holds the rows the lm_head takes.  A call of its own
        because a caller may put it into another captured graph than run()."""
        self._norm(norm_w)
