"""The pre-LayerNorm transformer encoder stack that both CLIP towers run (`clip.py`: causal, every layer's output kept;
`clip_vision.py`: full attention, two ping-pong buffers): weight packing, the plan base class, the launches of one layer
and the seeded stand-in weights.  What differs between the towers -- the attention launch, where the residual stream
lives, everything before and after the layers -- stays with them.

    layer_norm1                                          leco_layernorm_fwd
    fused q|k|v Linear                                   leco_gemm
    attention (the tower's own launch)                   leco_attention_causal_fwd / leco_attention_fwd
    out_proj + residual                                  leco_gemm
    layer_norm2                                          leco_layernorm_fwd
    fc1 + quick-GELU / GELU                              leco_gemm (LECO_ACT_QUICK_GELU / LECO_ACT_GELU)
    fc2 + residual                                       leco_gemm
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import graphs, ops
from .hip import ACT_GELU, ACT_NONE, ACT_QUICK_GELU, gemm_args

bf16 = torch.bfloat16
LN_EPS = 1e-5
ACTS = {"quick_gelu": ACT_QUICK_GELU, "gelu": ACT_GELU}


def f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().float().to(device).contiguous()


def wb(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device, bf16).contiguous()


def pack_encoder_layers(layers, device):
    """``(gemm_w, norm_p)`` of transformers' ``CLIPEncoderLayer``s: bf16 weight and fp32 bias under ``"{i}.qkv"`` (q, k, v
    stacked in that order), ``"{i}.out"``, ``"{i}.fc1"``, ``"{i}.fc2"``; fp32 gamma and beta under ``"{i}.ln1"``, ``"{i}.ln2"``."""
    gemm_w: Dict[str, Tuple[torch.Tensor, Optional[torch.Tensor]]] = {}
    norm_p: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
    for i, l in enumerate(layers):
        a = l.self_attn
        gemm_w[f"{i}.qkv"] = (wb(torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0), device),
                              f32(torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0), device))
        for key, m in (("out", a.out_proj), ("fc1", l.mlp.fc1), ("fc2", l.mlp.fc2)):
            gemm_w[f"{i}.{key}"] = (wb(m.weight, device), f32(m.bias, device))
        for key, m in (("ln1", l.layer_norm1), ("ln2", l.layer_norm2)):
            norm_p[f"{i}.{key}"] = (f32(m.weight, device), f32(m.bias, device))
    return gemm_w, norm_p


class EncoderPlan:
    def __init__(self):
        self.ops: List[ops.Op] = []
        self.names: List[str] = []               # one label per launch (tools/bench_clip*.py --per-op)
        self.graph = None
        self.keep: list = []                     # buffers of the tower's own launches that no other field holds
        # `EncoderEngine.scratch`: shared by every layer.  bf16 [M][C] LayerNorm output, [M][3 C] fused q|k|v, [M][C] attention
        # output, [M][C] stream after attention, [M][F] MLP hidden rows; fp32 [M] LayerNorm statistics
        self.n = self.qkv = self.att = self.h1 = self.u = self.mean = self.rstd = None

    def add(self, name: str, op: ops.Op) -> None:
        self.ops.append(op)
        self.names.append(name)


class EncoderEngine(graphs.PlanEngine):
    """The split-K workspace of one tower and the launches every plan of it is made of.  The tower packs its operands:
    ``gemm_w`` / ``norm_p`` from `pack_encoder_layers`, beside its embeddings, outer LayerNorms and projection."""

    def __init__(self, cfg, device: torch.device):
        super().__init__(device)
        self.cfg = cfg
        self.workspace = torch.empty(2 * 1024 * 1024, dtype=torch.float32, device=device)      # split-K partial slabs

    def buf(self, rows: int, cols: int) -> torch.Tensor:
        return torch.zeros(rows, cols, dtype=bf16, device=self.device)

    def scratch(self, p: EncoderPlan, M: int) -> None:
        """Allocate what the layers of plan ``p`` share (``M`` rows; the launches are ordered, so one set serves all)."""
        Cw, Fw = self.cfg.hidden_size, self.cfg.intermediate_size
        p.n, p.qkv, p.att, p.h1, p.u = self.buf(M, Cw), self.buf(M, 3 * Cw), self.buf(M, Cw), self.buf(M, Cw), self.buf(M, Fw)
        p.mean, p.rstd = torch.zeros(M, device=self.device), torch.zeros(M, device=self.device)

    def ln(self, p: EncoderPlan, name: str, x, y, rows: int) -> None:
        g, b = self.norm_p[name]
        Cw = self.cfg.hidden_size
        p.add("layernorm", ops.layernorm_fwd(x, Cw, g, b, self.cfg.layer_norm_eps, rows, Cw, y, Cw, p.mean, p.rstd))

    def gemm(self, p: EncoderPlan, label: str, w, bias, x, y, m: int, k: int, act: int = ACT_NONE, residual=None) -> None:
        g = gemm_args(x, w, y, m=m, n=w.shape[0], k=k, bias=bias, residual=residual, act=act)
        p.add(label, ops.gemm(g, keep=(w, bias, x, y, residual), ws=self.workspace))

    def layer(self, p: EncoderPlan, i: int, x, y, M: int, attention: Callable[[torch.Tensor, torch.Tensor], ops.Op]) -> None:
        """Layer ``i`` from the residual stream ``x`` into ``y`` (``M`` rows each); ``attention(qkv, att)`` is the tower's
        attention launch from the fused ``[M][3 C]`` q|k|v rows into ``[M][C]``."""
        Cw, Fw = self.cfg.hidden_size, self.cfg.intermediate_size
        self.ln(p, f"{i}.ln1", x, p.n, M)
        self.gemm(p, "qkv", *self.gemm_w[f"{i}.qkv"], p.n, p.qkv, M, Cw)
        p.add("attention", attention(p.qkv, p.att))
        self.gemm(p, "out_proj", *self.gemm_w[f"{i}.out"], p.att, p.h1, M, Cw, residual=x)
        self.ln(p, f"{i}.ln2", p.h1, p.n, M)
        self.gemm(p, "fc1", *self.gemm_w[f"{i}.fc1"], p.n, p.u, M, Cw, act=ACTS[self.cfg.hidden_act])
        self.gemm(p, "fc2", *self.gemm_w[f"{i}.fc2"], p.u, y, M, Fw, residual=p.h1)


def init_synthetic_encoder_(model, seed: int):
    """Seeded random weights of the scale of a trained tower, drawn in ``named_parameters`` order: token / position / class
    embeddings ~ N(0, 0.02), Linear and patch-convolution weights U(+-1/sqrt(fan_in)), LayerNorm gamma near 1, the rest
    0.02 N(0, 1).  Measurement tools and tests: no checkpoint exists on the build boxes."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "embedding" in name and "patch_embedding" not in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            elif p.ndim >= 2:
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) / p[0].numel() ** 0.5)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    model.release()
    return model
