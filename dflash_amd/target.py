"""`NativeTarget` — the caller-side neighbour of the hot path: the
target's 16-token *verify* forward (model/dflash.py:249-255) on the same gfx950
kernels as the draft, over a preallocated target KV cache.

It wraps the caller's HF-style dense causal LM (Qwen3 / Llama layout) and stays
call-compatible with it: `target(input_ids, position_ids=..., past_key_values=...,
output_hidden_states=...)`, `.model.embed_tokens`, `.lm_head`, `.device` all forward to
the wrapped model, so the reference's loop still runs unchanged on it.  The decode
loops of this package detect it and take the fast path instead:

* prefill (M = prompt length, a plain library GEMM problem) runs through the wrapped
  model once; its K/V are copied into the preallocated cache;
* every verify = 36 x {qkv GEMM, q/k-norm + RoPE + append, causal block attention,
  o_proj, residual + norm, gate/up SiLU GEMM, down GEMM, residual + norm [+ tap copy]}
  + lm_head GEMM with fused argmax over all 16 rows: the posterior ids come back
  without materialising 16 x V logits, rollback is a counter, and only the tapped
  layers' hidden rows are kept (the reference keeps all 37, model/utils.py:16-25).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional, Sequence

import torch

from . import ops
from .logits_stage import LogitsStage
from .model import TARGET_WEIGHT_FORMATS as WEIGHT_FORMATS, _rope_tables
from .row_stack import RowStack
from .tile_stack import TileStack, gemm_ws
from .utils import sample

BF16 = torch.bfloat16


class TargetKVCache:
    """Preallocated target KV: [layer][kv head][rows][128] bf16; crop = counter."""

    def __init__(self, n_layers, n_kv, max_rows, device):
        self.max_rows = int(max_rows)
        self.k = torch.zeros(n_layers, n_kv, self.max_rows, 128, dtype=BF16, device=device)
        self.v = torch.zeros_like(self.k)
        self.dyn = torch.zeros(16, dtype=torch.int32, device=device)   # one length record per 16-row block tile
        self.length = 0

    def get_seq_length(self, layer_idx: int = 0) -> int:
        return self.length

    def crop(self, max_length: int) -> None:
        if 0 < max_length < self.length:
            self.length = int(max_length)
        elif max_length < 0:
            self.length = max(0, self.length + int(max_length))


class _HiddenStates:
    """hidden_states of a native prefill: indexable like the HF tuple (index 0 = embedding output, l + 1 = output of
    decoder layer l, model/utils.py:16-25) for the states that were kept."""

    def __init__(self, kept: dict, n: int):
        self._kept, self._n = kept, n

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if i < 0:
            i += self._n
        if i not in self._kept:
            raise KeyError(f"hidden state {i} was not kept by this prefill (tap_layers = {sorted(k - 1 for k in self._kept)})")
        return self._kept[i]


class _Weight:
    """`.weight` holder standing in for the wrapped model's embed_tokens / lm_head once it is gone (keep_hf = False)."""

    def __init__(self, w):
        self.weight = w


class NativeTarget:
    def __init__(self, hf_model, max_splits: int = 32, attn_impl: str = "head", keep_hf: bool = True,
                 prefill: str = "native", weight_format: str = "bf16", expert_format: str = "bf16",
                 stream_format: str = "auto"):
        """stream_format: "auto" (default): a bf16 target's verify of <= 16 block rows streams each dense layer's gate/up
        and, at temperature 0, the lm_head from a lossless 13-bit copy (ops.pack_weight_bf16x13)
        wherever the layout covers the shape (hidden 2048 or 4096) and the packer takes the matrix: the same bits out,
        13/16 of the bytes in.  The plain packed weights stay resident for every other path (prefill, wide blocks, the
        ragged batch, sampled heads): 13/16 of gate/up and lm_head more memory.  A sparse-MoE target with bf16 experts at
        hidden 2048 streams its experts' gate/up the same way (dfl_moe_gate_up on the twin of each MoE layer's tall
        E * 2I x H matrix, lw["gu_e13"]: the verify of <= 16 rows and the per-tile expert branch of moe_mlp_tiles; the
        shared pass over 2..4 tiles, prefill and an fp8-expert target read the plain copy; a layer whose matrix the packer
        refused stays bf16).  That costs 13/16 of the gate/up expert bytes on top: at 30B-A3B about 31 GB beside 58 GB of
        weights ("The experts").  "bf16": plain packed bf16 everywhere.
        weight_format: "bf16" (default), or "fp8_e4m3": every Linear weight of the target — q/k/v, o_proj, gate, up and
        down of every layer, and the lm_head — is quantised here to OCP e4m3 codes with one power-of-two scale per output
        row (ops.quantize_fp8_rows; W8A16, weight-only).  The quantised target IS the model: THE CALLER'S hf_model IS
        MODIFIED — its Linear weights are overwritten in place with q * scale (with tied embeddings the embedding table
        then holds the dequantised head), so that `target.hf`, prefill="hf", `target.lm_head.weight`, share_lm_head and
        the native prefill all see the same model.  `self.layers` is the packed bf16 copy of q * scale (every path
        without an fp8 kernel), `self.layers8` / `self.lm_wp8` the codes, which the verify streams at one byte per
        weight ("The target").  Norm weights and the embedding gather stay bf16.  What weight-only
        e4m3 does to a real checkpoint's outputs, or to the acceptance length of a draft trained on the bf16 target, is
        NOT measured — hence off by default.
        expert_format: "bf16" (default), or "fp8_e4m3" for a sparse-MoE target (weight_format stays "bf16": at the MoE
        targets' hidden widths the dense projections are at their launch floors; the bytes are the experts'): every MoE
        layer's mlp.experts.gate_up_proj ([E, 2I, H] as E * 2I rows of H) and mlp.experts.down_proj ([E, H, I] as E * H
        rows of I) is quantised the same way, one power-of-two scale per output row.  Again the quantised target IS the
        model and THE CALLER'S hf_model IS MODIFIED: both expert tensors are overwritten in place with q * scale before
        anything is packed.  Router, norms, attention projections, dense layers (mlp_only_layers) and the lm_head stay
        bf16.  lw["gu_e"] / lw["down_e"] stay the packed bf16 copy of q * scale (the experts cost 1.5 x their bf16 bytes);
        `self.experts8[i]` holds layer i's codes and scales (ops.Fp8Experts; None for a dense layer), which the <= 16-row
        verify, the per-tile expert branch and the shared pass over 2..4 tiles stream while `self.expert_stream` is True
        ("The experts"; the native MoE prefill reads the copy).  What weight-only e4m3 does to a real MoE checkpoint's routing and outputs is NOT measured.
        attn_impl: "head" = dfl_attn_head on finished bf16 q/k/v rows (round 2, default); "fused" = the
        round-1 stage (fp32 K-split partials -> dfl_attn_fused), kept for A/B measurement and as a second
        implementation the tests compare against.
        prefill: "native" (round 3, default where the shapes allow: dense target, projection widths % 128) = the prompt
        through the MFMA GEMMs of csrc/prefill.hip on the same packed weights; "hf" = through the wrapped model.
        keep_hf = False: the wrapped model is dropped after packing (ONE copy of the layers' weights in memory; the
        caller must drop its own reference too); needs the native prefill."""
        self.x13 = ops.check_stream_format(stream_format) and weight_format == "bf16"
        self.stream_format = stream_format
        if attn_impl not in ("head", "fused"):
            raise ValueError("attn_impl must be 'head' or 'fused'")
        if prefill not in ("native", "hf"):
            raise ValueError("prefill must be 'native' or 'hf'")
        self.attn_impl = attn_impl
        # True: attention + o_proj in one launch (dfl_attn_head_oproj) where its range allows.  Measured SLOWER than the
        # two launches (23.2 vs 20.3 us per layer): off by default, kept for A/B and tests
        self.fuse_oproj = False
        # blocks of 17..32 rows: True = one pass over the weights through the ragged-batch GEMMs (R = 2), False = the
        # single-request GEMMs once per 16-row tile (two passes; kept for A/B and as a second implementation for tests)
        self.wide_one_pass = True
        self._wide = None
        self._wide_seed = None    # int64 [1]: the seed of an fp8 target's sampled wide head (dfl_gemm_sample_batch on e4m3 codes)
        self._kw_bufs = {}        # the buffers of a verify that is given the row processors as keywords, not as a stage
        self._nuc_logits = None   # the stage buffer the last verify materialised its raw rows into (what a test reads back)
        self.moe_pair_kernel = True   # MoE gate/up at K <= 2048 through dfl_moe_gate_up (False: the general kernel)
        self.moe_shared_pass = True   # three or four tiles (ragged batch, candidates): one pass over the experts they share
        self.moe_shared_min = 2       # tiles from which the shared pass is taken (30B-A3B layer: 2 tiles 291 -> 216 us, 4: 576 -> 241)
        self._moe_sh = None
        cfg = hf_model.config
        self.check_config(cfg, weight_format, expert_format)   # (before anything touches the device: a rejected architecture never launches a kernel)
        self.weight_format = weight_format
        self.expert_format = expert_format
        fp8 = weight_format == "fp8_e4m3"
        e8 = expert_format == "fp8_e4m3"
        # fp8 experts only: False = the bf16 expert kernels on the dequantised copy (the second implementation the tests compare)
        self.expert_stream = True
        self.experts8 = [] if e8 else None   # per layer: {"gu_e", "down_e"} ops.Fp8Experts twins, None for a dense layer
        # fp8_e4m3 only: False = the bf16 kernels on the dequantised copy (the second implementation the tests compare)
        self.fp8_stream = True
        self.layers8 = [] if fp8 else None   # per layer: ops.Fp8Weight twins of qkv / o / gu / down in self.layers
        self.lm_wp8 = None                   # the e4m3 lm_head (ops.Fp8Weight)
        self._tile_layers = {}               # tile_layers(): qkv_parts -> layer dicts with the e4m3 twins
        self._row_layers = {}                # row_layers(): streams e4m3 -> layer dicts with the e4m3 / 13-bit twins
        self.hf = hf_model
        self.model = hf_model.model
        self.lm_head = hf_model.lm_head
        self.config = cfg
        dev = hf_model.lm_head.weight.device
        if dev.type != "cuda":
            raise RuntimeError("NativeTarget: the wrapped model must live on the GPU")
        self._dev = dev
        self.H = cfg.hidden_size
        self.L = cfg.num_hidden_layers
        self.n_q = cfg.num_attention_heads
        self.n_kv = getattr(cfg, "num_key_value_heads", self.n_q)
        self.hd = getattr(cfg, "head_dim", None) or self.H // self.n_q
        self.I = cfg.intermediate_size
        self.V = cfg.vocab_size
        self.eps = float(cfg.rms_norm_eps)
        rope = getattr(cfg, "rope_parameters", None) or {}
        rtype = rope.get("rope_type", "default") if isinstance(rope, dict) else "default"
        theta = (rope.get("rope_theta") if isinstance(rope, dict) else None) or getattr(cfg, "rope_theta", None)
        if self.hd != 128 or self.H % 32 or (self.I % 32 and not getattr(cfg, "num_experts", 0)) or self.V % 16:
            raise NotImplementedError("NativeTarget: needs head_dim 128, hidden %32, vocab %16")
        # hidden > 4096: prefill on the prefill kernels and decode through the ragged-batch kernels (BatchedDecoder, a
        # group of one request); verify() — the single-request kernels, a whole K = hidden slice per workgroup — is not available
        self.wide_hidden = self.H // 32 > 128
        # position-only RoPE variants: the cos/sin tables are taken from the wrapped model's own
        # rotary module (Llama-3.1's "llama3" frequency scaling, BASELINE config 4; linear; yarn)
        if rtype not in ("default", "llama3", "linear", "yarn") or (rtype == "default" and theta is None):
            raise NotImplementedError(f"NativeTarget: rope_type {rtype!r} is not supported; keep the HF target")
        self.rope_type = rtype
        # sparse-MoE targets (BASELINE configs[4], Qwen3-Coder-30B-A3B): HF Qwen3-MoE layout (fused per-expert
        # gate_up_proj / down_proj tensors, softmax -> top-k -> renormalise router)
        self.E = int(getattr(cfg, "num_experts", 0) or 0)
        if getattr(cfg, "num_local_experts", 0) and not self.E:
            raise NotImplementedError("NativeTarget: only the Qwen3-MoE expert layout is supported; keep the HF target")
        if self.E:
            self.top_k = int(cfg.num_experts_per_tok)
            self.Ie = int(cfg.moe_intermediate_size)
            self.norm_topk = bool(getattr(cfg, "norm_topk_prob", False))
            if self.E > 256 or self.top_k > 8 or self.Ie % 32:
                raise NotImplementedError("NativeTarget: MoE needs <= 256 experts, top-k <= 8, moe_intermediate_size % 32 == 0")
        if getattr(cfg, "attention_bias", False) or getattr(cfg, "mlp_bias", False):
            raise NotImplementedError("NativeTarget: biased projections are not supported")
        self.theta = float(theta) if theta is not None else None
        sd = hf_model.state_dict()

        def w(name):
            return sd[name].detach().to(device=dev, dtype=BF16).contiguous()

        def mat(name, store, key):
            """A Linear weight: as loaded, or (fp8) its dequantised values q * scale — written back over the wrapped
            model's own tensor — with the codes and scales kept in `store`."""
            m = w(name)
            if fp8:
                m, store[key] = ops.quantize_keep_fp8(m)
                with torch.no_grad():
                    sd[name].copy_(m)   # (the state dict's tensors are the parameters' storage; exact in any float dtype)
            return m

        if fp8:   # the head first: with tied embeddings self.embed, read below, is then the dequantised head
            h8 = {}
            mat("lm_head.weight", h8, "lm")
            self.lm_wp8 = ops.pack_weight_fp8(*h8.pop("lm"))
        self.layers = []
        self.gu13 = []   # stream_format="auto": per layer, the 13-bit twin of a dense layer's gate/up or None
        self.down13 = []   # ... and of its down_proj (the K-chunked form: intermediate size a multiple of 2048 above 4096)
        for i in range(self.L):
            p = f"model.layers.{i}."
            l8, gu13, down13 = {}, None, None
            qkv = torch.cat([mat(p + "self_attn.q_proj.weight", l8, "q"), mat(p + "self_attn.k_proj.weight", l8, "k"),
                             mat(p + "self_attn.v_proj.weight", l8, "v")], dim=0)
            has_qk = (p + "self_attn.q_norm.weight") in sd
            lw = {"qkv": ops.pack_weight(qkv), "o": ops.pack_weight(mat(p + "self_attn.o_proj.weight", l8, "o")),
                  "q_norm": w(p + "self_attn.q_norm.weight") if has_qk else None,
                  "k_norm": w(p + "self_attn.k_norm.weight") if has_qk else None,
                  "ln1": w(p + "input_layernorm.weight"), "ln2": w(p + "post_attention_layernorm.weight")}
            if (p + "mlp.experts.0.gate_proj.weight") in sd:   # per-expert ModuleList layout (older transformers)
                raise NotImplementedError("NativeTarget: per-expert ModuleList MoE weights (mlp.experts.{e}.gate_proj) are "
                                          "not supported, only the fused gate_up_proj / down_proj tensors; keep the HF target")
            if (p + "mlp.experts.gate_up_proj") in sd:       # sparse-MoE layer
                gup, dwn = w(p + "mlp.experts.gate_up_proj"), w(p + "mlp.experts.down_proj")   # [E, 2I, H], [E, H, I]
                Ie = self.Ie
                if gup.shape != (self.E, 2 * Ie, self.H) or dwn.shape != (self.E, self.H, Ie):
                    raise ValueError(f"layer {i}: unexpected expert tensor shapes {tuple(gup.shape)} {tuple(dwn.shape)}")
                if e8:   # codes + scales per output row; the model's own tensors and what is packed below become q * scale
                    x8 = {}
                    for key, name, t in (("gu_e", "mlp.experts.gate_up_proj", gup), ("down_e", "mlp.experts.down_proj", dwn)):
                        q, sc = ops.quantize_fp8_rows(t.view(-1, t.shape[2]))
                        t.copy_(ops.dequantize_fp8_rows(q, sc).view_as(t))
                        with torch.no_grad():
                            sd[p + name].copy_(t)
                        x8[key] = ops.pack_experts_fp8(q.view(t.shape), sc.view(t.shape[:2]), gateup=key == "gu_e")
                        del q, sc
                    self.experts8.append(x8)
                    lw["gu_e8"], lw["down_e8"] = x8["gu_e"], x8["down_e"]   # (the layer dict is what moe_mlp_tiles is handed)
                lw["gu_e"] = torch.stack([ops.pack_weight_gateup(gup[e, :Ie].contiguous(), gup[e, Ie:].contiguous())
                                          for e in range(self.E)])
                lw["down_e"] = torch.stack([ops.pack_weight(dwn[e].contiguous()) for e in range(self.E)])
                if self.x13 and not e8 and self.H == 2048:   # the experts' gate/up as ONE tall matrix in 13 bits
                    g13 = ops.bf16x13_twin(lw["gu_e"], self.E * 2 * Ie, self.H, "experts_gateup")
                    if g13 is not None:   # (None: the kind is off or the packer refused the matrix — plain bf16 stays)
                        lw["gu_e13"] = g13   # (held by the layer dict: a captured verify reads it for the target's lifetime)
                ep = (self.E + 15) // 16 * 16               # router rows padded to whole column tiles (never routed to)
                rw = torch.zeros(ep, self.H, dtype=BF16, device=dev)
                rw[:self.E] = w(p + "mlp.gate.weight")
                lw["router"] = ops.pack_weight(rw)
                if ep % 128:    # the prefill's router GEMM (prefill.hip:k_pgemm) takes column blocks of 128
                    rp = torch.zeros((self.E + 127) // 128 * 128, self.H, dtype=BF16, device=dev)
                    rp[:self.E] = rw[:self.E]
                    lw["router_p"] = ops.pack_weight(rp)
                    del rp
                else:
                    lw["router_p"] = lw["router"]
                del gup, dwn, rw
            else:
                lw["gu"] = ops.pack_weight_gateup(mat(p + "mlp.gate_proj.weight", l8, "gate"),
                                                  mat(p + "mlp.up_proj.weight", l8, "up"))
                lw["down"] = ops.pack_weight(mat(p + "mlp.down_proj.weight", l8, "down"))
                if self.x13:   # the 13-bit twin, or None where plain bf16 stays (ops.bf16x13_twin)
                    gu13 = ops.bf16x13_twin(lw["gu"], 2 * self.I, self.H, "gateup")
                    down13 = ops.bf16x13_twin(lw["down"], self.H, self.I, "down")
                if e8:
                    self.experts8.append(None)
            if fp8:
                if "gate" not in l8:
                    raise NotImplementedError("NativeTarget: fp8_e4m3 needs dense MLP layers")
                self.layers8.append(ops.pack_layer_fp8(l8))
            self.layers.append(lw)
            self.gu13.append(gu13)
            self.down13.append(down13)
            del qkv, l8
        self.norm = w("model.norm.weight")
        self.embed = w("model.embed_tokens.weight")
        self.lm_wp = None  # set by share_lm_head() or packed on first use
        self.max_splits = max_splits
        self.q_dim, self.kv_dim = self.n_q * 128, self.n_kv * 128
        self.nqkv = self.q_dim + 2 * self.kv_dim
        self.ks_qkv = ops.pick_ksplit(self.nqkv, self.H, 1)
        self.ks_o = ops.pick_ksplit(self.H, self.q_dim, 1)
        self.ks_down = ops.pick_ksplit(self.H, self.I, 1)
        npart = max(self.ks_qkv * 16 * self.nqkv, self.ks_o * 16 * self.H, self.ks_down * 16 * self.H)
        z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
        NT = 2  # block rows as up to two 16-row tiles (blocks of 17..32 rows: one GEMM launch per tile)
        # the block rows' buffers and row sources, and the verify's layer sequence on the single-request kernels
        self.rows = RowStack(H=self.H, q_dim=self.q_dim, kv_dim=self.kv_dim, I=self.I, nqkv=self.nqkv, n_q=self.n_q,
                             n_kv=self.n_kv, eps=self.eps, max_splits=max_splits, device=dev,
                             ln1=[lw["ln1"] for lw in self.layers], ln2=[lw["ln2"] for lw in self.layers], norm=self.norm)
        self.ws = dict(part=z(npart, dt=torch.float32), attn_ws=ops.attn_fused_ws(self.n_q, self.n_kv, max_splits, dev),
                       argmax_ws=ops.argmax_ws(dev), sync=self.rows.sync,
                       post=torch.zeros(16 * NT, dtype=torch.int64, device=dev))
        self.is_moe = any("gu_e" in lw for lw in self.layers)
        if self.is_moe:
            ep = (self.E + 15) // 16 * 16
            # shares of the active experts (grid.y of dfl_moe_down): 4 with its two-tiles-per-workgroup form (H % 32 == 0)
            self.moe_nsplit = 2 if self.H % 32 else 4
            self.ws.update(xn=z(NT, 16 * self.H), xn1=z(NT, 16 * self.H), rlog=z(NT, 16, ep), wt=z(NT, 16, self.E),
                           act_e=z(self.E, 16 * self.Ie), moe_part=z(self.moe_nsplit, 16, self.H, dt=torch.float32),
                           active=torch.zeros(self.E, dtype=torch.int32, device=dev),
                           elist=torch.zeros(self.E, dtype=torch.int32, device=dev),
                           n_active=torch.zeros(1, dtype=torch.int32, device=dev),
                           rticket=torch.zeros(1, dtype=torch.int32, device=dev))
            # norm + gate Linear + routing as ONE launch (dfl_moe_router); the three launches otherwise
            self.moe_router_fused = self.H <= 4096 and self.E % 2 == 0
        self.src = {}
        if self.is_moe:   # MoE layers hand their successor ready-normalised rows (the residual add + norm launch after the experts)
            self.src = {k: [ops.rows_frag(self.ws[k][t]) for t in range(NT)] for k in ("xn", "xn1")}
        q_dim, kv_dim = self.n_q * 128, self.n_kv * 128
        self._pf = self._pf_moe = None
        dense_ok = all("gu_e" in lw for lw in self.layers) or self.I % 64 == 0   # (a dense MLP layer needs I % 64)
        self.native_prefill = (prefill == "native" and (q_dim + 2 * kv_dim) % 128 == 0 and self.H % 128 == 0 and dense_ok
                               and q_dim % 64 == 0 and (not self.is_moe or self.Ie % 64 == 0))
        self.prefill_attn = "native"   # "sdpa": the causal attention core of the prefill through torch (round-3 first form)
        self._rotary = getattr(hf_model.model, "rotary_emb", None)
        if not keep_hf:
            if not self.native_prefill:
                raise NotImplementedError("NativeTarget(keep_hf=False) needs the native prefill (widths % 128, FFN widths % 64)")
            if self.lm_wp is None:
                self.lm_wp = ops.pack_weight(self.lm_head.weight.detach().to(BF16).contiguous())
                self._head_twin()
            self.hf = None
            self.model = SimpleNamespace(embed_tokens=_Weight(self.embed), rotary_emb=self._rotary)
            self.lm_head = _Weight(self.lm_head.weight.detach())
        self.debug_routing = None
        self.gu_events = None   # (layer, start, end): torch.cuda.Event pair recorded around that layer's gate/up GEMM launch
        # (layer, start, end, n_active_out): the same around that MoE layer's expert gate/up launch; n_active_out (int32 [1],
        # device) receives the launch's active-expert count right behind the end event (bench.py: bytes = count x expert bytes)
        self.moe_events = None
        self._rope = None
        self._taps = {}
        torch.cuda.synchronize(dev)

    @staticmethod
    def check_config(cfg, weight_format: str = "bf16", expert_format: str = "bf16") -> None:
        """Architectures the kernels do not cover are rejected loudly, before any launch (the reference is shape-agnostic:
        model/dflash.py:36,42-56 take head_dim, attention_bias and sliding_window from the config; no BASELINE config
        needs them): head_dim != 128, biased projections, sliding-window attention layers, a sparse-MoE target (num_experts)
        whose hidden_size exceeds 4096 or is no multiple of 32.  weight_format: an unknown
        one is a ValueError; "fp8_e4m3" refuses a sparse-MoE target (its experts take expert_format instead) and hidden,
        intermediate or q widths that are not multiples of 64 (the packed e4m3 layout holds k-step pairs).
        expert_format: an unknown one is a ValueError; "fp8_e4m3" needs a sparse-MoE config (num_experts) whose hidden_size
        and moe_intermediate_size are multiples of 64."""
        if weight_format not in WEIGHT_FORMATS:
            raise ValueError(f"NativeTarget: weight_format must be one of {WEIGHT_FORMATS}, got {weight_format!r}")
        if expert_format not in WEIGHT_FORMATS:
            raise ValueError(f"NativeTarget: expert_format must be one of {WEIGHT_FORMATS}, got {expert_format!r}")
        n_q = cfg.num_attention_heads
        hd = getattr(cfg, "head_dim", None) or cfg.hidden_size // n_q
        if hd != 128:
            raise NotImplementedError(f"NativeTarget: the gfx950 kernels are built for head_dim == 128 (got {hd}); keep the HF target")
        if getattr(cfg, "attention_bias", False) or getattr(cfg, "mlp_bias", False):
            raise NotImplementedError("NativeTarget: biased projections are not supported; keep the HF target")
        lt = getattr(cfg, "layer_types", None) or ()
        if any(t == "sliding_attention" for t in lt) and getattr(cfg, "sliding_window", None):
            raise NotImplementedError("NativeTarget: sliding-window attention layers are not supported; keep the HF target")
        if getattr(cfg, "num_experts", 0) and (cfg.hidden_size > 4096 or cfg.hidden_size % 32):
            # (the experts' gate/up launch covers one K pass of 16 waves x 8 k-steps of 32: dfl_gemm_silu_mul_experts)
            raise NotImplementedError(f"NativeTarget: the sparse-MoE expert kernels cover hidden_size <= 4096 in multiples "
                                      f"of 32 (got {cfg.hidden_size}); keep the HF target")
        if weight_format == "fp8_e4m3":
            if getattr(cfg, "num_experts", 0) or getattr(cfg, "num_local_experts", 0):
                raise NotImplementedError("NativeTarget: fp8_e4m3 weights are not supported for sparse-MoE targets (the "
                                          "expert kernels have no e4m3 form); use weight_format='bf16'")
            widths = dict(hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, q_width=n_q * hd)
            bad = {k: v for k, v in widths.items() if v % 64}
            if bad:
                raise NotImplementedError(f"NativeTarget: fp8_e4m3 weights need hidden, intermediate and q widths % 64 == 0 "
                                          f"(got {bad})")
        if expert_format == "fp8_e4m3":
            if not getattr(cfg, "num_experts", 0):
                raise NotImplementedError("NativeTarget: expert_format='fp8_e4m3' needs a sparse-MoE target (Qwen3-MoE expert "
                                          "layout); a dense target takes weight_format='fp8_e4m3'")
            widths = dict(hidden_size=cfg.hidden_size, moe_intermediate_size=getattr(cfg, "moe_intermediate_size", 0))
            bad = {k: v for k, v in widths.items() if not v or v % 64}
            if bad:
                raise NotImplementedError(f"NativeTarget: fp8_e4m3 experts need hidden and moe_intermediate widths % 64 == 0 "
                                          f"(got {bad})")

    # ---- HF-compatible surface (the reference loop can still drive the wrapped model)
    @property
    def device(self):
        return self._dev

    def __call__(self, *a, **kw):
        if self.hf is None:
            raise RuntimeError("NativeTarget(keep_hf=False): the wrapped model is gone; use prefill() / verify()")
        return self.hf(*a, **kw)

    def share_lm_head(self, packed: torch.Tensor) -> None:
        self.lm_wp = packed
        self._head_twin()

    def _head_twin(self) -> None:
        """stream_format="auto": the packed head's 13-bit twin at load, not inside the first verify (one per packed
        tensor: a head shared with the draft has one twin)."""
        if self.x13 and self.lm_wp is not None:
            ops.bf16x13_twin(self.lm_wp, self.V, self.H, "lm_head")

    def streams_fp8(self, bs: int = 16) -> bool:
        """Whether verify() streams the e4m3 codes for a block of `bs` rows: an fp8 target, fp8_stream, the head
        attention stage; one 16-row tile with o_proj not fused, or 17..32 rows in one pass (_verify_wide).  Every other
        path computes the same quantised model from self.layers / self.lm_wp."""
        if self.layers8 is None or not self.fp8_stream or self.attn_impl != "head" or self.wide_hidden:
            return False
        return (not self.fuse_oproj) if bs <= 16 else self.wide_one_pass

    def streams_fp8_tiles(self) -> bool:
        """The same for the tile-stack paths — _verify_wide, the ragged batch and engine (batch.py; hidden > 4096 runs
        there as a group of one): gate/up, o_proj, down_proj and the lm_head take the codes, and q/k/v where it leaves K
        parts; q/k/v as finished rows reads self.layers.  Widths under 256 (toy models) run the
        bf16 kernels on the dequantised copy: the batch W8 forms refuse K < 256."""
        return (self.layers8 is not None and self.fp8_stream and self.attn_impl == "head"
                and min(self.H, self.I, self.q_dim) >= 256)   # (the ring and K-part W8 forms take K >= 256)

    def tile_layers(self, qkv_parts: bool) -> list:
        """The layer dicts TileStack.run takes: self.layers, with gu / o / down — and qkv, where the caller runs
        qkv="parts" — replaced by their e4m3 twins when streams_fp8_tiles()."""
        if not self.streams_fp8_tiles():
            return self.layers
        return ops.tile_layers(self.layers, self.layers8, qkv_parts, self._tile_layers)

    def row_layers(self, bs: int) -> list:
        """The layer dicts RowStack.run takes for a block of `bs` rows: self.layers, with the four matrices replaced by
        their e4m3 twins when streams_fp8(bs), else a dense layer's gate/up and down by their 13-bit twins where it has
        them (gu13, down13)."""
        return ops.row_layers(self.layers, self.layers8, self.gu13, self.streams_fp8(bs), self._row_layers, self.down13)

    def fp8_tensors(self) -> tuple:
        """Every e4m3 code tensor and scale vector of an fp8 target and of fp8 experts (empty for bf16): what a captured
        graph of the verify holds raw pointers to (DecodeSession's keep-alive tuple, the engine's capture key)."""
        ws = []
        if self.layers8 is not None:
            ws += [w8 for l8 in self.layers8 for w8 in l8.values()] + [self.lm_wp8]
        if self.experts8 is not None:
            ws += [x8 for l8 in self.experts8 if l8 is not None for x8 in l8.values()]
        return tuple(t for w8 in ws for t in (w8.wp, w8.scale))

    def expert_weights(self, lw: dict) -> tuple:
        """(gate/up, down) weights of an MoE layer (its dict in self.layers) for the two expert launches on <= 16 rows:
        the e4m3 codes (ops.Fp8Experts) of an fp8-expert target while expert_stream is set — gate/up only where the pair
        kernel runs (hidden <= 2048, moe_pair_kernel): dfl_gemm_silu_mul_experts has no W8 form — else the packed bf16
        copy; of a bf16 target under stream_format="auto", gate/up is the layer's 13-bit twin (lw["gu_e13"], hidden 2048)
        where the pair kernel runs and the packer took the matrix: the same bits from 13/16 of the bytes."""
        pair = self.H <= 2048 and self.moe_pair_kernel
        if "gu_e8" not in lw or not self.expert_stream:
            return (lw["gu_e13"] if (pair and "gu_e13" in lw) else lw["gu_e"]), lw["down_e"]
        return (lw["gu_e8"] if pair else lw["gu_e"]), lw["down_e8"]

    def tile_head(self):
        """The lm_head of the tile-stack paths: the e4m3 codes when streams_fp8_tiles(), else the packed bf16 copy."""
        return self.lm_wp8 if self.streams_fp8_tiles() else self.lm_wp

    def new_cache(self, max_rows: Optional[int] = None) -> TargetKVCache:
        if max_rows is None:
            raise ValueError("NativeTarget.new_cache needs max_rows (prompt + new tokens + block)")
        return TargetKVCache(self.L, self.n_kv, max_rows, self._dev)

    def _rope_tab(self, need: int):
        if self._rope is None or self._rope[0].shape[0] < need:
            n = 1 << (max(need, 4096) - 1).bit_length()
            if self.rope_type == "default":
                self._rope = _rope_tables(128, self.theta, n, self._dev)
            else:  # what the wrapped model itself multiplies by (scaled frequencies, attention factor), in bf16
                pos = torch.arange(n, device=self._dev).unsqueeze(0)
                cos, sin = self._rotary(torch.zeros(1, dtype=BF16, device=self._dev), pos)
                self._rope = (cos[0, :, :64].to(BF16).contiguous(), sin[0, :, :64].to(BF16).contiguous())
        return self._rope

    # ---- prefill (model/dflash.py:218-225)
    @torch.inference_mode()
    def prefill(self, input_ids: torch.Tensor, cache: TargetKVCache, output_hidden_states: bool = True,
                tap_layers: Optional[Sequence[int]] = None):
        """Returns an object with `.logits` [1, 1, V] (last prompt row, logits_to_keep = 1) and `.hidden_states`
        (indexable like HF's tuple).  tap_layers: keep only hidden_states[l + 1] for these layers (the draft's taps,
        model/utils.py:16-25) instead of all of them."""
        P = input_ids.shape[1]
        if P > cache.max_rows:
            raise ValueError("target KV cache too small for the prompt")
        if self.native_prefill:
            return self._prefill_native(input_ids, cache, output_hidden_states, tap_layers)
        return self._prefill_hf(input_ids, cache, output_hidden_states)

    def _prefill_native(self, input_ids, cache, output_hidden_states, tap_layers):
        """The prompt rows on the kernels: per layer RMSNorm -> frag16 tiles, q/k/v GEMM (bf16 rows), q/k-norm + RoPE +
        cache write, causal attention over the prompt (k_pattn: one wave per head and 16-row query tile), o_proj +
        residual, RMSNorm, gate/up + SiLU,
        down_proj + residual (+ tap).  Last row: final norm + lm_head through the decode path's skinny GEMM."""
        import torch.nn.functional as F
        P = input_ids.shape[1]
        H, I, dev = self.H, self.I, self._dev
        Pp = ops.prefill_rows_padded(P)
        q_dim, kv_dim, nqkv = self.q_dim, self.kv_dim, self.nqkv
        if self._pf is None or self._pf["h"].shape[0] < Pp:
            z = lambda *s: torch.zeros(*s, dtype=BF16, device=dev)  # noqa: E731
            dense_I = I if any("gu" in lw for lw in self.layers) else 0
            self._pf = dict(h=z(Pp, H), xf=z(Pp * max(H, q_dim)), qkv=z(Pp, nqkv), act=z(Pp * max(dense_I, 1)), attn=z(Pp, q_dim),
                            logits=z(16, self.V), ids=torch.zeros(16, dtype=torch.int64, device=dev))
        pf = self._pf
        h, xf, qkv, act, attn = pf["h"], pf["xf"], pf["qkv"], pf["act"], pf["attn"]
        h.zero_()
        torch.index_select(self.embed, 0, input_ids[0], out=h[:P])
        cos, sin = self._rope_tab(P + 64)
        want = None
        if output_hidden_states:
            want = set(range(self.L + 1)) if tap_layers is None else {int(l) + 1 for l in tap_layers}
            if max(want) >= self.L and tap_layers is not None:
                raise NotImplementedError("tapping the last layer (post-norm state) is not supported")
        kept = {}
        if want and 0 in want:
            kept[0] = h[:P].clone().unsqueeze(0)
        for i, lw in enumerate(self.layers):
            ops.prefill_norm_pack(h, P, H, lw["ln1"], self.eps, xf)
            ops.prefill_gemm_rows(lw["qkv"], xf, P, nqkv, H, qkv)
            ops.prefill_qk_rope(qkv, P, 0, q_dim, q_dim + kv_dim, self.n_q, self.n_kv, lw["q_norm"], lw["k_norm"], self.eps,
                                cos, sin, 0, cache.k[i], cache.v[i], 0)
            if self.prefill_attn == "native":   # csrc/prefill.hip:k_pattn, straight into o_proj's frag16 operand
                ops.prefill_attn(qkv, P, 0, cache.k[i], cache.v[i], self.n_q, self.n_kv, 128 ** -0.5, xf)
            else:                               # torch SDPA on the same rows (second implementation: tests, A/B)
                q = qkv[:P, :q_dim].view(P, self.n_q, 128).transpose(0, 1).unsqueeze(0)
                o = F.scaled_dot_product_attention(q, cache.k[i][:, :P].unsqueeze(0), cache.v[i][:, :P].unsqueeze(0),
                                                   is_causal=True, scale=128 ** -0.5, enable_gqa=self.n_kv != self.n_q)
                attn[:P].view(P, self.n_q, 128).copy_(o[0].transpose(0, 1))
                ops.prefill_norm_pack(attn, P, q_dim, None, self.eps, xf)      # rows -> frag16 tiles, no norm
            ops.prefill_gemm_resid(lw["o"], xf, P, H, q_dim, h)
            ops.prefill_norm_pack(h, P, H, lw["ln2"], self.eps, xf)
            tap = None
            if want and (i + 1) in want and i + 1 < self.L:   # (the last layer's output only exists final-normed in HF)
                tap = torch.empty(P, H, dtype=BF16, device=dev)
                kept[i + 1] = tap.unsqueeze(0)
            if "gu_e" in lw:   # sparse-MoE layer: rows sorted by expert, grouped MFMA GEMMs over each expert's rows
                if self._pf_moe is None or self._pf_moe["P"] < P:
                    self._pf_moe = ops.prefill_moe_scratch(P, H, self.Ie, self.E, self.top_k,
                                                           (self.E + 127) // 128 * 128, dev)
                ops.prefill_moe_mlp(lw["router_p"], lw["gu_e"], lw["down_e"], xf, P, H, self.Ie, self.E, self.top_k,
                                    self.norm_topk, h, self._pf_moe, tap=tap)
                if self.debug_routing is not None:    # tests: the experts every prompt row was routed to
                    self.debug_routing.append((i, self._pf_moe["pair_e"][:P, :self.top_k].clone()))
                continue
            ops.prefill_gemm_silu(lw["gu"], xf, P, I, H, act)
            ops.prefill_gemm_resid(lw["down"], act, P, H, I, h, tap=tap)
        # last prompt row: final norm + lm_head on its 16-row tile (the decode path's GEMM, norm applied in its prologue)
        if self.lm_wp is None:
            self.lm_wp = ops.pack_weight(self.lm_head.weight.detach().to(BF16).contiguous())
        t0 = (P - 1) // 16 * 16
        rows = h[t0:t0 + 16]
        if self.wide_hidden:   # K = hidden cut over workgroups: the ragged-batch form of norm + lm_head, one tile
            if "wxn" not in pf:
                pf["wxn"] = torch.zeros(2, 16 * H, dtype=BF16, device=dev)
                pf["wdyn"] = torch.tensor([[0, 0, 16, 0, 0, 0, 0, 0]] * 2, dtype=torch.int32, device=dev)
                pf["wgws"] = torch.zeros(ops.lib().dfl_gemm_batch_ws_bytes(self.V, H), dtype=torch.uint8, device=dev)
                pf["wh"] = torch.zeros(2, 16, H, dtype=BF16, device=dev)
                pf["wlogits"], pf["wids"] = torch.zeros(2, 16, self.V, dtype=BF16, device=dev), torch.zeros(2, 16, dtype=torch.int64, device=dev)
            pf["wh"][0].copy_(rows)
            ops.norm_frag_batch(pf["wh"], 1, self.norm, self.eps, pf["wxn"], pf["wdyn"], ops.DYN_BS)
            ops.gemm_argmax_batch(self.lm_wp, ops.brows_frag(pf["wxn"]), 1, self.V, H, 0, 16, pf["wgws"], pf["wids"], 0,
                                  pf["wdyn"], nrows_dyn_word=ops.DYN_BS, logits=pf["wlogits"])
            pf["logits"].copy_(pf["wlogits"][0])
        else:
            ss = rows.float().pow(2).sum(-1).contiguous()
            ops.gemm_argmax(self.lm_wp, ops.rows_normed(rows, ss, 1, self.norm, self.eps), self.V, H, 0, 16,
                            self.ws["argmax_ws"], pf["ids"], 0, logits=pf["logits"])
        logits = pf["logits"][P - 1 - t0].clone().view(1, 1, self.V)
        # (hidden_states[L], HF's final-normed state, is not kept: nothing on the path reads it — model/utils.py:16-25
        # taps layer OUTPUTS, and build_target_layer_ids never picks the last layer)
        cache.length = P
        return SimpleNamespace(logits=logits, hidden_states=_HiddenStates(kept, self.L + 1) if output_hidden_states else None)

    def _prefill_hf(self, input_ids, cache, output_hidden_states):
        """Through the wrapped model, K/V copied into the preallocated cache (odd widths, prefill="hf")."""
        from transformers import DynamicCache
        P = input_ids.shape[1]
        tmp = DynamicCache()
        pos = torch.arange(P, device=self._dev).unsqueeze(0)
        out = self.hf(input_ids, position_ids=pos, past_key_values=tmp, use_cache=True, logits_to_keep=1,
                      output_hidden_states=output_hidden_states)
        for i in range(self.L):
            cache.k[i, :, :P].copy_(tmp.layers[i].keys[0])
            cache.v[i, :, :P].copy_(tmp.layers[i].values[0])
        cache.length = P
        return out

    def _moe_mlp(self, i: int, lw: dict, tiles, hrow, taps, sl) -> list:
        """Qwen3MoeSparseMoeBlock of layer i on the block rows (tf:models/qwen3_moe/modeling_qwen3_moe.py): norm, router
        GEMM, softmax/top-k/renormalise, gate/up of every active expert in one launch, the routing-weighted down
        projections as fp32 K-part sums, then residual add + tap + the NEXT stage's RMSNorm in one row-wise launch.
        Returns the row sources of those normalised rows (RowStack.run's `moe`)."""
        ws, H, E = self.ws, self.H, self.E
        nxt = self.layers[i + 1]["ln1"] if i + 1 < self.L else self.norm
        gu_e, down_e = self.expert_weights(lw)   # (fp8 experts: the codes where the launch has a W8 form)
        for t, dt in tiles:
            if self.moe_router_fused:
                ops.moe_router(h=hrow[t], norm_w=lw["ln2"], eps=self.eps, xn=ws["xn"][t], wp_router=lw["router"], K=H, E=E,
                               top_k=self.top_k, norm_topk=self.norm_topk, rlog=ws["rlog"][t], wt=ws["wt"][t],
                               active=ws["active"], lst=ws["elist"], n_active=ws["n_active"], ticket=ws["rticket"], dyn=dt,
                               dyn_word=ops.DYN_BS)
            else:
                ops.norm_pack(norm_w=lw["ln2"], frag=ws["xn"][t], H=H, eps=self.eps, resid_in=hrow[t], dyn=dt,
                              dyn_word=ops.DYN_BS)
                ops.gemm_resid(lw["router"], self.src["xn"][t], ws["rlog"].shape[2], H, ws["rlog"][t], add_residual=False,
                               dyn=dt)
                ops.moe_route(ws["rlog"][t], E, self.top_k, self.norm_topk, ws["wt"][t], ws["active"], ws["elist"],
                              ws["n_active"], dyn=dt, dyn_word=ops.DYN_BS)
            if self.debug_routing is not None and t == 0:    # tests: the routing weights of every MoE layer
                self.debug_routing.append((i, ws["wt"][0].clone()))
            mev = self.moe_events if (self.moe_events is not None and self.moe_events[0] == i and t == 0) else None
            if mev is not None:
                mev[1].record()
            if H <= 2048 and self.moe_pair_kernel:   # one LDS meeting per (gate, up) tile pair: 64 KB tiles at K = 2048
                ops.moe_gate_up(gu_e, ws["xn"][t], E, self.Ie, H, ws["act_e"], ws["elist"], ws["n_active"], dyn=dt,
                                valid_word=ops.DYN_BS)
            else:
                ops.gemm_silu_mul_experts(lw["gu_e"], self.src["xn"][t], E, self.Ie, H, ws["act_e"], ws["elist"],
                                          ws["n_active"], dyn=dt)
            if mev is not None:
                mev[2].record()
                mev[3].copy_(ws["n_active"])
            ops.moe_down(down_e, ws["act_e"], ws["wt"][t], ws["elist"], ws["n_active"], E, H, self.Ie,
                         self.moe_nsplit, ws["moe_part"])
            tap = taps[16 * t:16 * t + 16, sl[0] * H:(sl[0] + 1) * H] if sl else None
            ops.norm_pack(norm_w=nxt, frag=ws["xn1"][t], H=H, eps=self.eps, part=ws["moe_part"], nsplit=self.moe_nsplit,
                          part_split=16 * H, ldp=H, resid_in=hrow[t], h_out=hrow[t], h_out2=tap,
                          ld2=taps.stride(0) if tap is not None else 0, dyn=dt, dyn_word=ops.DYN_BS)
        return self.src["xn1"]

    def moe_mlp_tiles(self, lw: dict, R: int, MT: int, dyn: torch.Tensor, xn: torch.Tensor, part: torch.Tensor) -> int:
        """Qwen3MoeSparseMoeBlock (tf:models/qwen3_moe/modeling_qwen3_moe.py) of one layer for R 16-row tiles that went
        through the layer's attention and dense projections together (requests of a ragged batch, candidate blocks of
        one verify): tile r routes ITS rows — router GEMM on its ln2-normalised fragments xn[r], fp32 softmax / top-k /
        renormalise — and streams ITS active experts (gate/up + SiLU, routing-weighted down projections); the experts a
        tile uses are its own, so there is no weight stream to share unless two tiles pick the same expert.  The
        routing-weighted sums land as fp32 shares in the batch partial-sum layout part[share][MT * 16][H], where the
        next dfl_norm_frag_batch adds them to the residual stream (one rounding).  dyn: [MT, 8] length records (valid
        rows = the DYN_BS word).  Returns the share count."""
        w, ns, H = self.ws, self.moe_nsplit, self.H
        if R >= self.moe_shared_min and self.moe_shared_pass and H % 128 == 0 and self.Ie % 64 == 0:
            return self._moe_mlp_shared(lw, R, MT, dyn, xn, part)
        # The share stride is what the consumer reads with — dfl_norm_frag_batch(nsplit=ns) strides by
        # batch_tiles(R) * 16 * H (ops.norm_frag_batch) — NOT the caller's tile-slot count: a candidate verifier
        # always allocates MT = 4 slots, and for R <= 2 (batch_tiles = 2) share 1 would otherwise land at 64 H
        # while it is read at 32 H (half of the experts' down projections dropped).
        mt = ops.batch_tiles(R)
        if mt > MT:
            raise ValueError(f"moe_mlp_tiles: {R} tiles need {mt} tile slots, the buffers have {MT}")
        pv = part[:ns * mt * 16 * H].view(ns, mt * 16, H)
        gu_e, down_e = self.expert_weights(lw)   # (fp8 experts: the codes, as the shared pass above)
        for r in range(R):
            dt, x = dyn[r], xn[r]
            if self.moe_router_fused:   # gate Linear + routing in one launch on the tile's normalised fragments
                ops.moe_router(h=None, norm_w=None, eps=self.eps, xn=x, wp_router=lw["router"], K=H, E=self.E,
                               top_k=self.top_k, norm_topk=self.norm_topk, rlog=w["rlog"][0], wt=w["wt"][0],
                               active=w["active"], lst=w["elist"], n_active=w["n_active"], ticket=w["rticket"], dyn=dt,
                               dyn_word=ops.DYN_BS)
            else:
                ops.gemm_resid(lw["router"], ops.rows_frag(x), w["rlog"].shape[2], H, w["rlog"][0], add_residual=False, dyn=dt)
                ops.moe_route(w["rlog"][0], self.E, self.top_k, self.norm_topk, w["wt"][0], w["active"], w["elist"],
                              w["n_active"], dyn=dt, dyn_word=ops.DYN_BS)
            if H <= 2048 and self.moe_pair_kernel:
                ops.moe_gate_up(gu_e, x, self.E, self.Ie, H, w["act_e"], w["elist"], w["n_active"], dyn=dt,
                                valid_word=ops.DYN_BS)
            else:
                ops.gemm_silu_mul_experts(lw["gu_e"], ops.rows_frag(x), self.E, self.Ie, H, w["act_e"], w["elist"],
                                          w["n_active"], dyn=dt)
            ops.moe_down(down_e, w["act_e"], w["wt"][0], w["elist"], w["n_active"], self.E, H, self.Ie, ns,
                         w["moe_part"])
            pv[:, r * 16:(r + 1) * 16].copy_(w["moe_part"])
        return ns

    def _moe_mlp_shared(self, lw: dict, R: int, MT: int, dyn: torch.Tensor, xn: torch.Tensor, part: torch.Tensor) -> int:
        """The same for three or four tiles in ONE pass over the experts: the R x 16 rows are routed, sorted by expert and
        gathered like prompt rows (dfl_prefill_moe_*, csrc/prefill.hip), so that an expert several tiles picked is
        streamed once (four tiles of 16 rows x top-8 touch nearly all of 128 experts: one pass over them instead of four
        over ~80 each).  Same rounding points as the per-tile kernels; the rows' fp32 sums land as ONE share in `part`.
        An fp8-expert target streams the codes here too while expert_stream is set (ops.moe_grouped_gate_up / _down).
        Rows beyond a tile's valid count are routed too (zero fragments) and ignored by the norm launch that follows."""
        H, P = self.H, R * 16
        if self._moe_sh is None:
            ep = (self.E + 127) // 128 * 128
            self._moe_sh = dict(sc=ops.prefill_moe_scratch(4 * 16, H, self.Ie, self.E, self.top_k, ep, self._dev),   # (<= 4 tiles)
                                rlog=torch.zeros(4, 16, ep, dtype=BF16, device=self._dev),
                                gws=torch.zeros(ops.lib().dfl_gemm_batch_ws_bytes(ep, H), dtype=torch.uint8, device=self._dev))
        sh = self._moe_sh
        sc, L, st = sh["sc"], ops.lib(), ops._stream()
        ops.gemm_resid_batch(lw["router_p"], ops.brows_frag(xn), R, sh["rlog"].shape[2], H, sh["rlog"], add_residual=False,
                             ws=sh["gws"], dyn=dyn)
        ops.prefill_moe_route(sh["rlog"].view(64, -1), P, sc, self.norm_topk)
        # fp8 experts: both grouped launches stream the codes (the grouped form has no K <= 2048 limit, so gate/up too at
        # any hidden width); else, or with expert_stream off, the packed bf16 copy
        e8 = "gu_e8" in lw and self.expert_stream
        ops.moe_grouped_gate_up(lw["gu_e8"] if e8 else lw["gu_e"], xn, sc, H, gather=True)
        ops.moe_grouped_down(lw["down_e8"] if e8 else lw["down_e"], sc, H)
        ops.check(L.dfl_prefill_moe_combine(sc["out32"].data_ptr(), sc["posmap"].data_ptr(), P, H, self.top_k, None, 0, None, 0,
                                            part.data_ptr(), st), "dfl_prefill_moe_combine")
        return 1

    # ---- the verify forward on the kernels
    def _verify_wide(self, block_ids, start, cache, bs, tap_layers, taps, logits_out, temperature, cos, sin, seed=None,
                     stage=None):
        """Blocks of 17..32 rows in ONE pass over the weights: the two 16-row tiles go through the ragged-batch
        GEMMs (tile_stack.TileStack, R = 2) as if they were two requests, and through ONE attention launch per layer with
        two query tiles on the request's single cache.  Same lines as verify(): model/dflash.py:249-257."""
        ws, rs, H, R = self.ws, self.rows, self.H, 2
        if self._wide is None:
            self._wide = TileStack(H=H, q_dim=self.q_dim, I=self.I, nqkv=self.nqkv, eps=self.eps, MT=2,
                                   gws=gemm_ws(H, (self.V, 2 * self.I, self.nqkv), (H, self.I, self.q_dim), self._dev),
                                   h=rs.h.view(2, 16, H), attn=rs.attn, act=rs.act,
                                   xq=rs.xq.view(2, 16, self.nqkv), moe_nsplit=self.moe_nsplit if self.is_moe else 0)
            self._wide_ids = torch.zeros(2, 16, dtype=torch.int64, device=self._dev)
        st = self._wide
        s, gws = st.src, st.gws
        dyn2 = cache.dyn[:16].view(2, 8)
        self._wide_ids.view(-1)[:bs].copy_(block_ids[:bs])
        ops.embed_rows_batch(self.embed, self._wide_ids, R, st.h, H, rs.ss_emb.view(2, 16), dyn2, ops.DYN_BS)

        def attend(i, lw):
            ops.attn_head(xq=rs.xq, q_col=0, k_col=self.q_dim, v_col=self.q_dim + self.kv_dim, n_q=self.n_q,
                          n_kv=self.n_kv, q_norm_w=lw["q_norm"], k_norm_w=lw["k_norm"], eps=self.eps, cos_tab=cos,
                          sin_tab=sin, kcache=cache.k[i], vcache=cache.v[i], scale=128 ** -0.5, causal=True, S=start,
                          tau=0, bs=bs, pos0=start, ws=rs.head_ws, max_splits=self.max_splits, out_frag=rs.attn,
                          q_tiles=2, out_tile_stride=rs.attn.stride(0))

        st.run(self.tile_layers(qkv_parts=False), R, dyn2, attend, qkv="rows",
               taps=None if taps is None else taps.view(2, 16, -1), tap_layers=tap_layers, moe=self.moe_mlp_tiles)
        st.finish(self.norm)
        post = ws["post"]
        if stage is not None and stage.materialises and logits_out is None:   # the head launch below materialises the block's logits
            logits_out = self._nuc_logits = stage.raw
        # tile j row m -> position start + 16 j + m + 1, both tiles of the one request
        where = dict(dyn=dyn2, nrows_dyn_word=ops.DYN_BS, pos=dict(pos_base=start, pos_add=1), tiles_per_req=2)

        def lp_rows(logits, ids):
            if stage is not None and stage.lp is not None:
                stage.logprobs(logits.view(2, 16, self.V), ids.view(2, 16), **where)

        process = stage is not None and stage.processes
        if not process and temperature >= 1e-5 and seed is not None and self.streams_fp8_tiles():
            # an fp8 target: the seeded draw in the e4m3 ring head's epilogue (tile j row m -> POS0 + 16 j + m + 1; the
            # record is rewritten here: verify() rewrites it only when the block size changes, and POS0 must be this
            # cycle's `start`) — the ids of sample_rows over the same launch's logits
            ops.set_dyn2(cache.dyn, start, 0, bs, start)
            if self._wide_seed is None:
                self._wide_seed = torch.zeros(1, dtype=torch.int64, device=self._dev)
            self._wide_seed.fill_(ops.seed_i64(seed))
            ops.gemm_sample_batch(self.lm_wp8, s["xn"], R, self.V, H, 0, 16, gws, post.view(2, 16), 0, dyn2,
                                  seeds=self._wide_seed, temperature=temperature, pos_word=ops.DYN_POS0, pos_add=1,
                                  tiles_per_req=2, nrows_dyn_word=ops.DYN_BS,
                                  logits=None if logits_out is None else logits_out.view(2, 16, self.V))
            lp_rows(logits_out, post)
            cache.length = start + bs
            return post[:bs].unsqueeze(0), taps
        logits = logits_out
        if not process and temperature >= 1e-5:
            logits = torch.empty(32, self.V, dtype=BF16, device=self._dev)
        lv = None if logits is None else logits.view(2, 16, self.V)
        ops.gemm_argmax_batch(self.tile_head(), s["xn"], R, self.V, H, 0, 16, gws, post.view(2, 16), 0, dyn2,
                              nrows_dyn_word=ops.DYN_BS, logits=lv)
        if process:   # (blocks of 17..32 rows: min_p and the filtered draw; the processors that read the block were refused)
            stage.rows(lv, None, post.view(2, 16), draw=dict(seed=seed, temperature=temperature), **where)
            posterior = post[:bs].unsqueeze(0)
        elif temperature >= 1e-5 and seed is not None:   # the seeded draw over the materialised rows: row j -> start + j + 1
            ops.sample_rows(logits[:bs], seed=seed, temperature=temperature, pos0=start + 1, out=post[:bs])
            posterior = post[:bs].unsqueeze(0)
        else:
            posterior = post[:bs].unsqueeze(0) if temperature < 1e-5 else sample(logits[:bs].unsqueeze(0), temperature)
        if stage is not None and stage.lp is not None:
            ids = post
            if posterior.data_ptr() != post.data_ptr():   # the host draw: its ids, padded to the two tiles
                ids = torch.zeros(32, dtype=torch.int64, device=self._dev)
                ids[:bs] = posterior[0]
            lp_rows(logits, ids)
        cache.length = start + bs
        return posterior, taps

    def raise_if_failed(self) -> None:
        """fuse_oproj only: a dfl_attn_head_oproj launch whose o_proj workgroups gave up waiting (2 ms) leaves a flag."""
        if self.fuse_oproj:
            self.rows.raise_if_failed()

    @torch.inference_mode()
    def verify(self, block_ids: torch.Tensor, start: int, cache: TargetKVCache, *, tap_layers: Sequence[int] = (),
               temperature: float = 0.0, logits_out: Optional[torch.Tensor] = None,
               taps_out: Optional[torch.Tensor] = None, dyn_lengths: bool = False, seed: Optional[int] = None,
               top_k: int = 0, top_p: float = 1.0, logprobs=None, penalties=None, logit_bias=None, grammar=None,
               min_p=None, stage=None):
        """block_ids int64 [bs] at positions start..start+bs-1 (cache rows alike), bs <= 32.
        Returns (posterior ids int64 [1, bs], taps bf16 [32, len(tap_layers)*H] or None).
        K/V of all bs rows are written; the caller crops to what it accepts.
        taps_out: the caller's own [32, len(tap_layers)*H] buffer (a decode session keeps the
        rows until its next draft; sessions interleaved on one target must not share one).
        logits_out: bf16 [16 * tiles, V].  Blocks of 17..32 rows run as two 16-row tiles: one pass over the
        weights through the ragged-batch GEMMs (`_verify_wide`; an MoE layer's expert MLP per tile), or one launch per
        tile of every single-request GEMM (wide_one_pass = False); both query tiles share the attention launch.
        dyn_lengths (bs <= 16, attention stage "head"): the launches take S / pos0 from the cache's device record alone
        (kept by dfl_accept_commit, dyn_t) — `start` is then only an upper bound that sizes the attention's key splits
        and the RoPE table, and the sequence can be captured into a hipGraph (DecodeSession.capture).
        seed (temperature > 0): the seeded Gumbel-max draw in the lm_head epilogue instead of softmax + multinomial —
        row j draws position start + j + 1, start from the record's POS0 word under dyn_lengths;
        no logits are written unless logits_out is given.
        stage: a logits_stage.LogitsStage (None: off, and nothing here changes) — the row processors between the head
        launch and the posterior, in the order its docstring gives.  The head launch then materialises the block's
        logits, into logits_out or the stage's own buffer, and the stage's launches write the posterior; row m predicts
        position start + m + 1, start from the record's POS0 word under dyn_lengths.  A stage with logprobs alone
        leaves the head launches below as they are and reads the rows they materialise.
        top_k / top_p / logprobs / penalties / logit_bias / grammar / min_p: the same asked by keyword, for a caller
        that keeps the state objects itself (LogitsStage.of_keywords); their buffers are this target's."""
        bs = block_ids.numel()
        own = stage is None
        if own:
            stage = LogitsStage.of_keywords(self.V, temperature, top_k=top_k, top_p=top_p, logprobs=logprobs,
                                            penalties=penalties, logit_bias=logit_bias, grammar=grammar, min_p=min_p)
        if stage is not None:
            stage.check_block(bs, temperature, seed, logits_out)
        if self.wide_hidden:
            raise NotImplementedError("NativeTarget.verify: hidden > 4096 runs through the ragged-batch path "
                                      "(dflash_generate / dflash_generate_batch / BatchedDecoder)")
        if bs < 1 or bs > 32:
            raise ValueError("verify takes 1..32 block rows")
        if bs > 16 and self.attn_impl != "head":
            raise ValueError("blocks of more than 16 rows need attn_impl='head'")
        if start + bs > cache.max_rows:
            raise ValueError("target KV cache too small")
        ws, H = self.ws, self.H
        if self.lm_wp is None:
            self.lm_wp = ops.pack_weight(self.lm_head.weight.detach().to(BF16).contiguous())
        cos, sin = self._rope_tab(start + bs + 64)
        # the verify's kernels read only the tiles' valid-row counts from the record (the attention takes immediates):
        # it is rewritten when the block size changes, not every cycle
        # — the round-1 fused stage (attn_impl="fused") reads S / TAU / POS0 from the record: rewritten every call there
        if dyn_lengths:
            if bs > 16 or self.attn_impl != "head" or self.fuse_oproj:
                raise ValueError("dyn_lengths needs a block of <= 16 rows and the plain 'head' attention stage")
        elif self.attn_impl != "head" or getattr(cache, "_dyn_bs", None) != bs:
            ops.set_dyn2(cache.dyn, start, 0, bs, start)
            cache._dyn_bs = bs
        dyn = cache.dyn[:8]
        tiles = [(t, cache.dyn[8 * t:8 * t + 8]) for t in range((bs + 15) // 16)]
        taps = None
        tap_layers = list(tap_layers)
        if tap_layers:
            if max(tap_layers) >= self.L - 1:
                raise NotImplementedError("tapping the last layer (post-norm state) is not supported")
            key = len(tap_layers)
            if taps_out is not None:
                if taps_out.shape != (32, key * H) or taps_out.dtype != BF16 or not taps_out.is_contiguous():
                    raise ValueError("taps_out must be a contiguous bf16 [32, len(tap_layers)*H] tensor")
                taps = taps_out
            else:
                if key not in self._taps:
                    self._taps[key] = torch.zeros(32, key * H, dtype=BF16, device=self._dev)
                taps = self._taps[key]
        w8 = self.streams_fp8(bs)
        head = self.lm_wp8 if w8 else self.lm_wp
        if own and stage is not None:
            stage.device, stage._bufs = self._dev, self._kw_bufs
        if len(tiles) == 2 and self.wide_one_pass and self.attn_impl == "head":
            return self._verify_wide(block_ids, start, cache, bs, tap_layers, taps, logits_out, temperature, cos, sin, seed,
                                     stage)
        rs = self.rows
        for t, dt in tiles:
            ops.embed_rows(self.embed, block_ids[16 * t:], rs.h_tiles[t], H, rs.ss_emb[16 * t:], dt, ops.DYN_BS)

        def attend(i, lw, x1):   # attn_impl="fused": the block rows' q/k/v as fp32 K parts (mt = 1), then the round-1 stage
            ops.gemm_f32(lw["qkv"], x1[0], None, 1, self.nqkv, H, self.ks_qkv, ws["part"], dyn)
            ops.attn_fused(qkv=ws["part"], nsplit=self.ks_qkv, split_stride=16 * self.nqkv, ld=self.nqkv, q_col=0,
                           k_col=self.q_dim, v_col=self.q_dim + self.kv_dim, ctx_row0=0, blk_row0=0, n_q=self.n_q,
                           n_kv=self.n_kv, q_norm_w=lw["q_norm"], k_norm_w=lw["k_norm"], eps=self.eps,
                           cos_tab=cos, sin_tab=sin, kcache=cache.k[i], vcache=cache.v[i], dyn=dyn,
                           scale=128 ** -0.5, kv_len_max=start + bs, ws=ws["attn_ws"],
                           max_splits=self.max_splits, out_frag=rs.attn[0], causal=True)

        # fin: the final-normed rows' sources (after an MoE layer the rows are final-normed already)
        fin = rs.run(self.row_layers(bs), tiles, bs=bs, fuse_oproj=self.fuse_oproj,
                     attend=None if self.attn_impl == "head" else attend,
                     attn=dict(cos_tab=cos, sin_tab=sin, kcache=cache.k, vcache=cache.v, causal=True, S=start, tau=0,
                               pos0=start, dyn=dyn if dyn_lengths else None),
                     taps=taps, tap_layers=tap_layers, moe=self._moe_mlp, gu_events=self.gu_events)
        post = ws["post"]
        logits = logits_out
        process = stage is not None and stage.processes
        if stage is not None and logits is None and (process or stage.lp is not None and (seed is not None or temperature < 1e-5)):
            logits = self._nuc_logits = stage.raw   # (the host draw below materialises into a buffer of its own)

        if stage is not None:
            def pos(t):   # tile t row m predicts position start + 16 t + m + 1, start from the record when replayed
                return dict(pos_word=ops.DYN_POS0 if dyn_lengths else -1, pos_base=start, pos_add=16 * t + 1)

            def lp_rows(ids):   # behind the launches that wrote the posterior
                for t, dt in tiles:
                    stage.logprobs(logits[16 * t:16 * t + 16], ids[16 * t:], pos=pos(t), nrows=min(16, bs - 16 * t), dyn=dt)

        if process:   # per tile: the head launch materialises the raw rows, the stage's launches write the posterior
            if temperature < 1e-5 and self.x13 and not w8:
                head = ops.bf16x13_twin(head, self.V, H, "lm_head") or head
            draw = dict(seed=seed, temperature=temperature) if temperature >= 1e-5 else None
            for t, dt in tiles:
                n, raw = min(16, bs - 16 * t), logits[16 * t:16 * t + 16]
                ops.gemm_argmax(head, fin[t], self.V, H, 0, n, ws["argmax_ws"], post, 16 * t, dyn=dt, logits=raw)
                stage.rows(raw, block_ids, post[16 * t:16 * t + 16], draw=draw, pos=pos(t), tile=t, nrows=n, dyn=dt)
            lp_rows(post)
            cache.length = start + bs
            return post[:bs].unsqueeze(0), taps
        if temperature >= 1e-5 and seed is not None:
            for t, dt in tiles:   # tile t row m predicts position start + 16 t + m + 1
                ops.gemm_sample(head, fin[t], self.V, H, 0, min(16, bs - 16 * t), ws["argmax_ws"], post, 16 * t,
                                seed=seed, temperature=temperature, pos_dyn=dt if dyn_lengths else None,
                                pos_word=ops.DYN_POS0, pos_base=start, pos_add=16 * t + 1, dyn=dt,
                                logits=None if logits is None else logits[16 * t:16 * t + 16])
            if stage is not None:
                lp_rows(post)
            cache.length = start + bs
            return post[:bs].unsqueeze(0), taps
        if temperature >= 1e-5:
            logits = torch.empty(16 * len(tiles), self.V, dtype=BF16, device=self._dev)
        elif self.x13 and not w8:   # the greedy posterior: the head's 13-bit twin (the draft's, where DecodeSession shares the packed head)
            head = ops.bf16x13_twin(head, self.V, H, "lm_head") or head
        for t, dt in tiles:
            ops.gemm_argmax(head, fin[t], self.V, H, 0, min(16, bs - 16 * t), ws["argmax_ws"], post, 16 * t,
                            dyn=dt, logits=None if logits is None else logits[16 * t:16 * t + 16])
        if temperature < 1e-5:
            posterior = post[:bs].unsqueeze(0)
        else:
            posterior = sample(logits[:bs].unsqueeze(0), temperature)
        if stage is not None:
            lp_rows(posterior[0].contiguous())
        cache.length = start + bs
        return posterior, taps
