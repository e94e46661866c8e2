"""The CLIP text encoder (transformers' ``CLIPTextModel`` / ``CLIPTextModelWithProjection``: CLIP-L of SD1.x / SDXL,
OpenCLIP-H of SD2.x, OpenCLIP-bigG of SDXL) on the HIP kernels: token ids -> prompt embeddings, what the reference's
``train_util.py:32-62`` (``text_encode`` / ``text_encode_xl``) gets from ``text_encoder(tokens)``.

The module tree only HOLDS weights under the transformers parameter names (``text_model.embeddings.token_embedding``,
``text_model.embeddings.position_embedding``, ``text_model.encoder.layers.N.{self_attn.{q,k,v,out}_proj, layer_norm1,
layer_norm2, mlp.fc1, mlp.fc2}``, ``text_model.final_layer_norm``, ``text_projection``), so an HF state dict -- or the
output of ``ckpt_convert.convert_ldm_clip`` / ``convert_open_clip`` -- loads with ``load_state_dict`` as is.  A call runs
a forward-only launch plan built from ``ops.*`` per (batch, sequence length): bf16 activations, fp32 accumulation;
replayed from a hipGraph when ``use_graphs`` is set.  The N layers are the stack of ``encoder.py``, shared with the image tower.

    token + position embedding                           leco_embed_rows
    N x  layer_norm1                                     leco_layernorm_fwd
         fused q|k|v Linear                              leco_gemm
         causal attention, 64-wide heads                 leco_attention_causal_fwd
         out_proj + residual                             leco_gemm
         layer_norm2                                     leco_layernorm_fwd
         fc1 + quick-GELU / GELU                         leco_gemm (LECO_ACT_QUICK_GELU / LECO_ACT_GELU)
         fc2 + residual                                  leco_gemm
    final_layer_norm                                     leco_layernorm_fwd
    EOS row per sample                                   leco_embed_rows (no position table)
    text_projection (no bias)                            leco_gemm

The tokenizer stays transformers' ``CLIPTokenizer``; there is no backward (no text-encoder LoRA / textual inversion).
"""
from __future__ import annotations

import json
from dataclasses import dataclass, fields
from typing import List, Optional

import torch
from torch import nn

from . import graphs, ops
from .encoder import ACTS, LN_EPS, EncoderEngine, EncoderPlan, f32, init_synthetic_encoder_, pack_encoder_layers, wb

HEAD_DIM = 64                    # what leco_attention_causal_fwd is built for: every CLIP tower SD uses


@dataclass
class CLIPTextConfig:
    vocab_size: int = 49408
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    max_position_embeddings: int = 77
    hidden_act: str = "quick_gelu"
    projection_dim: int = 768
    eos_token_id: int = 2
    bos_token_id: int = 0
    layer_norm_eps: float = LN_EPS

    def __post_init__(self):
        if self.hidden_act not in ACTS:
            raise ValueError(f"CLIP text encoder: hidden_act {self.hidden_act!r} is not one of {sorted(ACTS)}")
        if self.num_attention_heads <= 0 or self.hidden_size != HEAD_DIM * self.num_attention_heads:
            raise ValueError(f"CLIP text encoder: hidden_size {self.hidden_size} / num_attention_heads {self.num_attention_heads} "
                             f"must be {HEAD_DIM} (the causal attention kernel is built for {HEAD_DIM}-wide heads)")
        if self.max_position_embeddings > ops.CAUSAL_ATTN_MAX_S:
            raise ValueError(f"CLIP text encoder: max_position_embeddings {self.max_position_embeddings} exceeds the causal "
                             f"attention kernel's {ops.CAUSAL_ATTN_MAX_S} tokens")
        if self.intermediate_size % 64 or self.projection_dim % 8 or self.num_hidden_layers < 1:
            raise ValueError("CLIP text encoder: intermediate_size must be a multiple of 64, projection_dim of 8, and there "
                             "must be at least one layer")

    @classmethod
    def from_dict(cls, d: dict, **override) -> "CLIPTextConfig":
        known = {f.name for f in fields(cls)}
        kw = {k: v for k, v in d.items() if k in known and v is not None}
        kw.update(override)
        return cls(**kw)

    @classmethod
    def from_json(cls, path: str, **override) -> "CLIPTextConfig":
        """A diffusers ``text_encoder/config.json``."""
        with open(path) as f:
            return cls.from_dict(json.load(f), **override)


def clip_l_config(**kw) -> CLIPTextConfig:
    return CLIPTextConfig(**{**dict(eos_token_id=49407, bos_token_id=49406), **kw})


def open_clip_h_config(**kw) -> CLIPTextConfig:
    """SD2.x: 24 layers in the tower, 23 used (the penultimate layer's output)."""
    return CLIPTextConfig(**{**dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=23, num_attention_heads=16,
                                    hidden_act="gelu", projection_dim=1024, eos_token_id=49407, bos_token_id=49406), **kw})


def open_clip_bigg_config(**kw) -> CLIPTextConfig:
    return CLIPTextConfig(**{**dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20,
                                    hidden_act="gelu", projection_dim=1280, eos_token_id=49407, bos_token_id=49406), **kw})


# ---- weight holders (transformers names) ---------------------------------------------------------------------------------------
class CLIPTextEmbeddings(nn.Module):
    def __init__(self, cfg: CLIPTextConfig):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.position_embedding = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)


class CLIPAttention(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)


class CLIPMLP(nn.Module):
    def __init__(self, c: int, f: int):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(c, f), nn.Linear(f, c)


class CLIPEncoderLayer(nn.Module):
    def __init__(self, cfg: CLIPTextConfig):
        super().__init__()
        c = cfg.hidden_size
        self.self_attn = CLIPAttention(c)
        self.layer_norm1 = nn.LayerNorm(c, eps=cfg.layer_norm_eps)
        self.mlp = CLIPMLP(c, cfg.intermediate_size)
        self.layer_norm2 = nn.LayerNorm(c, eps=cfg.layer_norm_eps)


class CLIPEncoder(nn.Module):
    def __init__(self, cfg: CLIPTextConfig):
        super().__init__()
        self.layers = nn.ModuleList([CLIPEncoderLayer(cfg) for _ in range(cfg.num_hidden_layers)])


class CLIPTextTransformer(nn.Module):
    def __init__(self, cfg: CLIPTextConfig):
        super().__init__()
        self.embeddings = CLIPTextEmbeddings(cfg)
        self.encoder = CLIPEncoder(cfg)
        self.final_layer_norm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class CLIPTextOutput:
    """What ``train_util.text_encode`` / ``text_encode_xl`` read: ``[0]`` (``last_hidden_state``, or ``text_embeds`` for the
    projection class), ``.last_hidden_state``, ``.pooler_output``, ``.text_embeds``, ``.hidden_states``."""

    def __init__(self, first: str, last_hidden_state, pooler_output, text_embeds=None, hidden_states=None):
        self._first = first
        self.last_hidden_state, self.pooler_output = last_hidden_state, pooler_output
        self.text_embeds, self.hidden_states = text_embeds, hidden_states

    def _tuple(self):
        head = (self.text_embeds, self.last_hidden_state) if self._first == "text_embeds" else \
            (self.last_hidden_state, self.pooler_output)
        return head + ((self.hidden_states,) if self.hidden_states is not None else ())

    def __getitem__(self, i):
        return self._tuple()[i]

    def __iter__(self):
        return iter(self._tuple())


# ---- launch plan ---------------------------------------------------------------------------------------------------------------
class CLIPPlan(EncoderPlan):
    def __init__(self):
        super().__init__()
        self.ids: torch.Tensor = None            # int32 [B * S]: token ids
        self.eos_idx: torch.Tensor = None        # int32 [B]: row b * S + (EOS position of sample b) of the hidden states
        self.hidden: List[torch.Tensor] = []     # bf16 [B * S][C]: the embeddings, then every layer's output
        self.last: torch.Tensor = None           # bf16 [B * S][C]: final_layer_norm of the last layer's output
        self.pooled: torch.Tensor = None         # bf16 [B][C]
        self.text_embeds: Optional[torch.Tensor] = None     # bf16 [B][projection_dim]


class CLIPEngine(EncoderEngine):
    """Packed device operands of one text encoder and its launch plans, keyed by (batch, sequence length)."""

    def __init__(self, model: "CLIPTextModel", device: torch.device):
        tm = model.text_model
        super().__init__(model.cfg, device)
        self.tok, self.pos = wb(tm.embeddings.token_embedding.weight, device), wb(tm.embeddings.position_embedding.weight, device)
        self.gemm_w, self.norm_p = pack_encoder_layers(tm.encoder.layers, device)
        self.norm_p["final"] = (f32(tm.final_layer_norm.weight, device), f32(tm.final_layer_norm.bias, device))
        proj = getattr(model, "text_projection", None)
        self.proj_w = None if proj is None else wb(proj.weight, device)

    # -- plan construction ----------------------------------------------------------------------------------------------------
    def _build(self, B: int, S: int) -> CLIPPlan:
        cfg, dev = self.cfg, self.device
        Cw, H, M = cfg.hidden_size, cfg.num_attention_heads, B * S
        p = CLIPPlan()
        p.ids = torch.zeros(M, dtype=torch.int32, device=dev)
        p.eos_idx = torch.zeros(B, dtype=torch.int32, device=dev)
        p.hidden = [self.buf(M, Cw) for _ in range(cfg.num_hidden_layers + 1)]      # `hidden_states` wants every layer's output
        self.scratch(p, M)

        def attention(qkv, att):
            q0, ld = qkv.data_ptr(), 3 * Cw
            return ops.attention_causal_fwd(q0, ld, S * ld, q0 + 2 * Cw, ld, S * ld, q0 + 4 * Cw, ld, S * ld, att.data_ptr(),
                                            Cw, S * Cw, B, H, S, HEAD_DIM, HEAD_DIM ** -0.5, keep=(qkv, att))

        p.add("embed", ops.embed_rows(self.tok, Cw, cfg.vocab_size, p.ids, self.pos, Cw, S, p.hidden[0], Cw, M, Cw))
        for i in range(cfg.num_hidden_layers):
            self.layer(p, i, p.hidden[i], p.hidden[i + 1], M, attention)
        p.last = self.buf(M, Cw)
        self.ln(p, "final", p.hidden[-1], p.last, M)
        p.pooled = self.buf(B, Cw)
        p.add("eos_gather", ops.embed_rows(p.last, Cw, M, p.eos_idx, None, 0, 1, p.pooled, Cw, B, Cw))
        if self.proj_w is not None:
            p.text_embeds = self.buf(B, self.proj_w.shape[0])
            self.gemm(p, "projection", self.proj_w, None, p.pooled, p.text_embeds, B, Cw)
        return p

    def plan(self, B: int, S: int) -> CLIPPlan:
        return self.cached((B, S), lambda: self._build(B, S))


class CLIPTextModel(graphs.ForwardOnlyModel):
    """transformers' ``CLIPTextModel``, forward only."""
    _first = "last_hidden_state"
    engine_type = CLIPEngine
    label = "CLIP text encoder"
    bf16_only = "bfloat16 only; `train.precision: float32` does not extend to the native text encoder"

    def __init__(self, cfg: Optional[CLIPTextConfig] = None):
        super().__init__(use_graphs=True)
        self.cfg = cfg or CLIPTextConfig()
        self.text_model = CLIPTextTransformer(self.cfg)
        self.requires_grad_(False)

    load_state_dict = graphs.ForwardOnlyModel.load_strict      # an HF state dict as is; a wrong key is a KeyError

    @property
    def device(self):
        return self.text_model.final_layer_norm.weight.device

    @property
    def dtype(self):
        return self.text_model.final_layer_norm.weight.dtype

    def eos_positions(self, ids: torch.Tensor) -> torch.Tensor:
        """transformers' pooling rule: the first position equal to ``eos_token_id``, or argmax of the ids for the legacy
        configs that say ``eos_token_id == 2``."""
        if self.cfg.eos_token_id == 2:
            return ids.argmax(dim=-1)
        return (ids == self.cfg.eos_token_id).int().argmax(dim=-1)

    def _encode(self, input_ids) -> CLIPPlan:
        ids = torch.as_tensor(input_ids)
        if ids.ndim != 2 or ids.dtype.is_floating_point or ids.dtype == torch.bool:
            raise ValueError(f"CLIP text encoder: input_ids must be an integer [batch][tokens] tensor, got {tuple(ids.shape)} {ids.dtype}")
        B, S = ids.shape
        if not 1 <= S <= self.cfg.max_position_embeddings or B < 1:
            raise ValueError(f"CLIP text encoder: {S} tokens per prompt, max_position_embeddings is {self.cfg.max_position_embeddings}")
        host = ops.check_row_ids(ids, self.cfg.vocab_size, "input_ids")          # IndexError before any launch
        eos = self.eos_positions(host.view(B, S).long()) + torch.arange(B) * S
        plan = self.engine().plan(B, S)
        plan.ids.copy_(host)
        plan.eos_idx.copy_(eos.to(torch.int32))
        self._run(plan)
        return plan

    @torch.no_grad()
    def forward(self, input_ids, output_hidden_states: bool = False, **kw) -> CLIPTextOutput:
        plan = self._encode(input_ids)
        B, S = torch.as_tensor(input_ids).shape
        out = self.copy_out
        hs = tuple(out(h, B, S, -1) for h in plan.hidden) if output_hidden_states else None
        te = None if plan.text_embeds is None else out(plan.text_embeds, B, -1)
        return CLIPTextOutput(self._first, out(plan.last, B, S, -1), out(plan.pooled, B, -1), te, hs)


class CLIPTextModelWithProjection(CLIPTextModel):
    """transformers' ``CLIPTextModelWithProjection``: ``[0]`` / ``.text_embeds`` = text_projection(pooled output), no bias."""
    _first = "text_embeds"

    def __init__(self, cfg: Optional[CLIPTextConfig] = None):
        super().__init__(cfg)
        self.text_projection = nn.Linear(self.cfg.hidden_size, self.cfg.projection_dim, bias=False)
        self.requires_grad_(False)


def init_synthetic_clip_(model: CLIPTextModel, seed: int = 2468) -> CLIPTextModel:
    """Seeded stand-in weights (`encoder.init_synthetic_encoder_`)."""
    return init_synthetic_encoder_(model, seed)
