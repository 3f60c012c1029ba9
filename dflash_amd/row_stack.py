"""`RowStack` — a decoder stack over one request's block on the single-request ("skinny") kernels: TileStack's twin for
the other kernel family, and the one place THIS family's layer sequence lives.

The draft forward (model.py, draft_block) and the target's verify (target.py, verify) of a block of <= 16 rows run
through here — the headline cycle of bench.py — and so does a 17..32-row block taken in two passes (wide_one_pass =
False: every GEMM once per 16-row tile).  Per layer:

    gemm_resid(q/k/v) per tile  ->  attn_head over all tiles  ->  gemm_resid(o, + residual) per tile  ->
    gemm_silu_mul(gate/up) per tile  ->  gemm_resid(down, + residual [+ tap]) per tile        | the caller's MoE MLP

No norm launches: o_proj and down_proj add to the residual rows in `h` and leave each row's partial sums of squares in
`ss_h`, and the GEMM that consumes a normalised activation applies the RMSNorm itself from a row source built here once
(layer 0 reads the embedding's sums in `ss_emb`).  An MoE layer normalises for its successor instead and hands back the
sources of those rows.  Callers differ in the attention's mask and key rows (the draft: not causal, plus the context
rows' K/V in `xc`; the target: causal), in taps, MoE layers and timing events (target only), in the round-1 "fused"
attention stage each keeps as a callback, and in what surrounds the stack (embedding, lm_head).  Which weight format a
launch streams is the caller's row_layers(bs) (ops.row_layers): the stack takes the layer dicts as they come.
"""
from __future__ import annotations

import torch

from . import ops

BF16, F32 = torch.bfloat16, torch.float32
NT = 2   # block rows as up to two 16-row tiles (blocks of 17..32 rows)


class RowStack:
    def __init__(self, *, H: int, q_dim: int, kv_dim: int, I: int, nqkv: int, n_q: int, n_kv: int, eps: float,
                 max_splits: int, device, ln1, ln2, norm):
        """ln1 / ln2: the layers' input and post-attention norm weights, norm: the final norm's.  The row sources point
        at them and at the buffers made here: a caller that reloads its weights builds a new stack."""
        self.H, self.q_dim, self.kv_dim, self.I, self.nqkv = H, q_dim, kv_dim, I, nqkv
        self.n_q, self.n_kv, self.eps, self.max_splits = n_q, n_kv, eps, max_splits
        z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=device)  # noqa: E731
        self.h = z(16 * NT, H)
        self.ss_emb = z(16 * NT, dt=F32)
        self.ss_h = z(NT, H, dt=F32)       # per tile [H/16 column tiles][16 rows]
        self.xq = z(16 * NT, nqkv)
        self.attn = z(NT, 16 * q_dim)
        self.act = z(NT, 16 * I)
        self.head_ws = ops.attn_head_ws(n_q, max_splits, NT, device)
        self.sync = torch.zeros(ops.ATTN_OPROJ_SYNC_WORDS, dtype=torch.int32, device=device)
        self.h_tiles = [self.h[16 * t:16 * t + 16] for t in range(NT)]
        nt = H // 16

        def normed(w, first=False):
            return [ops.rows_normed(self.h_tiles[t], self.ss_emb[16 * t:] if first else self.ss_h[t], 1 if first else nt,
                                    w, eps, ops.DYN_BS) for t in range(NT)]

        self.src = dict(ln1=[normed(w, first=i == 0) for i, w in enumerate(ln1)], ln2=[normed(w) for w in ln2],
                        final=normed(norm), attn=[ops.rows_frag(self.attn[t]) for t in range(NT)],
                        act=[ops.rows_frag(self.act[t]) for t in range(NT)])

    def raise_if_failed(self) -> None:
        """A dfl_attn_head_oproj launch (fuse_oproj) whose o_proj workgroups gave up waiting (2 ms) leaves a flag."""
        if int(self.sync[ops.ATTN_OPROJ_FAIL_WORD]) != 0:
            self.sync.zero_()
            raise RuntimeError("dfl_attn_head_oproj: an o_proj workgroup gave up waiting for the attention stage")

    def run(self, layers, tiles, *, attn: dict, bs: int, fuse_oproj: bool = False, attend=None, taps=None, tap_layers=(),
            moe=None, gu_events=None) -> list:
        """The layers over the block's `bs` rows in h (embedded, their sums of squares in ss_emb).  tiles: [(t, the
        tile's length record)].  Returns the row sources of the final-normed rows, one per tile.
        attn: what the attention launch takes per call — cos_tab, sin_tab, kcache / vcache (indexed by layer here),
        causal, S, tau, pos0, dyn (or None) and, for the draft, xc: the context rows' K/V of all layers (or None).
        fuse_oproj: attention + o_proj in one launch where its range allows (one tile, q_dim <= 4096).
        attend(i, lw, x1): the round-1 "fused" stage in place of q/k/v + attention, from the sources x1 to frag16 rows
        in attn[0].
        taps [32, len(tap_layers) * H]: receives the output rows of the layers in tap_layers.
        moe(i, lw, tiles, h_tiles, taps, slots) -> the sources of the NEXT stage's normalised rows: the MLP of a layer
        with experts (NativeTarget._moe_mlp).
        gu_events (layer, start, end): events recorded around that layer's gate/up launches (bench.py)."""
        H, I, s, hs = self.H, self.I, self.src, self.h_tiles
        tl = list(tap_layers)
        if tl and max(tl) >= len(layers) - 1:
            raise NotImplementedError("tapping the last layer (post-norm state) is not supported")
        fuse_o = fuse_oproj and attend is None and len(tiles) == 1 and self.q_dim <= 4096
        xc = attn.get("xc")
        call = dict(xq=self.xq, q_col=0, k_col=self.q_dim, v_col=self.q_dim + self.kv_dim, n_q=self.n_q, n_kv=self.n_kv,
                    eps=self.eps, cos_tab=attn["cos_tab"], sin_tab=attn["sin_tab"], scale=128 ** -0.5, causal=attn["causal"],
                    S=attn["S"], tau=attn["tau"], bs=bs, pos0=attn["pos0"], ws=self.head_ws, max_splits=self.max_splits,
                    dyn=attn["dyn"])   # the attention launch's arguments that no layer changes
        nxt = None   # an MoE layer leaves its successor's input already normalised
        for i, lw in enumerate(layers):
            x1 = s["ln1"][i] if nxt is None else nxt
            if attend is not None:
                attend(i, lw, x1)
            else:
                # q/k/v as finished bf16 Linear outputs, then one launch: q/k-norm + RoPE + append + attention + merge
                for t, dt in tiles:
                    ops.gemm_resid(lw["qkv"], x1[t], self.nqkv, H, self.xq[16 * t:], add_residual=False, dyn=dt)
                kw = dict(call, q_norm_w=lw["q_norm"], k_norm_w=lw["k_norm"], kcache=attn["kcache"][i],
                          vcache=attn["vcache"][i])
                if xc is not None:
                    kw.update(xc=xc, ck_col=i * 2 * self.kv_dim, cv_col=i * 2 * self.kv_dim + self.kv_dim)
                if fuse_o:
                    ops.attn_head_oproj(**kw, attn_frag=self.attn[0], wo=lw["o"], H=H, h_io=hs[0], ss_out=self.ss_h[0],
                                        sync=self.sync)
                else:
                    ops.attn_head(**kw, out_frag=self.attn, q_tiles=len(tiles), out_tile_stride=self.attn.stride(0))
            is_moe = "gu_e" in lw
            if not fuse_o:
                for t, dt in tiles:
                    # (an MoE block normalises its rows itself — dfl_moe_router: no partial sums of squares wanted, and
                    # without them a narrow o_proj may run in half tiles on twice the workgroups)
                    ops.gemm_resid(lw["o"], s["attn"][t], H, self.q_dim, hs[t], add_residual=True,
                                   ss_out=None if is_moe else self.ss_h[t], dyn=dt)
            # every slot j with tap_layers[j] == i: build_target_layer_ids repeats layers for shallow targets and the
            # reference concatenates the same state twice (model/utils.py:16-25)
            sl = [j for j, l in enumerate(tl) if l == i]
            if is_moe:
                nxt = moe(i, lw, tiles, hs, taps, sl)
            else:
                nxt = None
                gev = gu_events if (gu_events is not None and gu_events[0] == i) else None
                if gev is not None:
                    gev[1].record()
                for t, dt in tiles:
                    ops.gemm_silu_mul(lw["gu"], s["ln2"][i][t], I, H, self.act[t], dt)
                if gev is not None:
                    gev[2].record()
                for t, dt in tiles:
                    tap = taps[16 * t:16 * t + 16, sl[0] * H:(sl[0] + 1) * H] if sl else None
                    ops.gemm_resid(lw["down"], s["act"][t], H, I, hs[t], add_residual=True, ss_out=self.ss_h[t], tap=tap,
                                   dyn=dt)
            for j in sl[1:]:
                taps[:, j * H:(j + 1) * H].copy_(taps[:, sl[0] * H:(sl[0] + 1) * H])
        return (s["final"] if nxt is None else nxt)[:len(tiles)]
