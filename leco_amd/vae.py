"""The Stable Diffusion VAE (diffusers 0.20 ``AutoencoderKL``: ``Decoder``, and -- opt-in, ``encoder=True`` -- ``Encoder`` +
``quant_conv``) on the HIP kernels: latents -> image, what the reference's ``test/infer_xl.py:136-154`` does with
``vae.decode`` + ``save_image``, and image -> latents (``encode`` / ``encode_to_latents``) for img2img sampling.

The module tree only HOLDS weights under the diffusers parameter names (``post_quant_conv``, ``decoder.conv_in``,
``decoder.mid_block.resnets.N``, ``decoder.mid_block.attentions.0.{group_norm,to_q,to_k,to_v,to_out.0}``,
``decoder.up_blocks.N.resnets.M``, ``decoder.up_blocks.N.upsamplers.0.conv``, ``decoder.conv_norm_out``,
``decoder.conv_out``), so a diffusers state dict loads as is.  ``decode`` runs a forward-only launch plan built from
``ops.*`` per (batch, h, w): bf16 activations, fp32 accumulation, channels-last; replayed from a hipGraph when
``use_graphs`` is set.

    post_quant_conv (1 / scaling_factor folded in)      leco_latent_affine
    conv_in                                             leco_conv_in
    resnet: GN+SiLU -> conv3x3 -> GN+SiLU -> conv3x3 (+ shortcut as the GEMM's residual operand)
    mid attention: GN -> fused q|k|v Linear -> one head of width C (leco_attention_fwd, d = C) -> out Linear + residual
    upsample: nearest 2x folded into the conv's operand gather (LECO_A_CONV3_UP2)
    conv_norm_out + SiLU -> conv_out -> fp32 NCHW and / or 8-bit NHWC pixels (leco_conv_out_rgb)

The encoder (``encoder.conv_in``, ``encoder.down_blocks.N.resnets.M``, ``encoder.down_blocks.N.downsamplers.0.conv``,
``encoder.mid_block.*``, ``encoder.conv_norm_out``, ``encoder.conv_out``, ``quant_conv``) is the mirror image, one plan per
(batch, H, W, input kind, output kind):

    conv_in from the fp32 NCHW image in [-1, 1] or the 8-bit NHWC image         leco_conv_in_rgb
    resnets as above; downsample: F.pad(x, (0,1,0,1)) + 3x3 / stride 2 / pad 0 folded into the gather (LECO_A_CONV3_S2_PAD01)
    mid block as above
    conv_norm_out + SiLU -> conv_out -> quant_conv -> moments and / or scaled sampled latents   leco_conv_out_moments
"""
from __future__ import annotations

import json
import struct
import zlib
from dataclasses import dataclass, fields
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import graphs, hip, ops
from .hip import ACT_NONE, ACT_SILU, A_CONV3_S1, A_CONV3_S2_PAD01, A_CONV3_UP2, A_PLAIN, gemm_args

bf16 = torch.bfloat16
GN_EPS = 1e-6
WIDE_HEAD_DIMS = (128, 512)      # head widths leco_attention_fwd has a single-head kernel for


@dataclass
class VAEConfig:
    latent_channels: int = 4
    out_channels: int = 3
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    scaling_factor: float = 0.18215

    @classmethod
    def from_dict(cls, d: dict) -> "VAEConfig":
        known = {f.name for f in fields(cls)}
        kw = {k: v for k, v in d.items() if k in known}
        if "block_out_channels" in kw:
            kw["block_out_channels"] = tuple(kw["block_out_channels"])
        return cls(**kw)

    @classmethod
    def from_json(cls, path: str) -> "VAEConfig":
        with open(path) as f:
            return cls.from_dict(json.load(f))


def sd_vae_config() -> VAEConfig:
    return VAEConfig()


def sdxl_vae_config() -> VAEConfig:
    return VAEConfig(scaling_factor=0.13025)


def tiny_vae_config(scaling_factor: float = 0.18215) -> VAEConfig:
    """Four levels (the 8x factor holds), small enough for the host emulator."""
    return VAEConfig(block_out_channels=(64, 64, 128, 128), layers_per_block=1, scaling_factor=scaling_factor)


# ---- weight holders (diffusers names) ------------------------------------------------------------------------------------------
class ResnetBlock2D(nn.Module):
    def __init__(self, cin: int, cout: int, groups: int):
        super().__init__()
        self.in_channels, self.out_channels = cin, cout
        self.norm1 = nn.GroupNorm(groups, cin, eps=GN_EPS)
        self.conv1 = nn.Conv2d(cin, cout, 3, 1, 1)
        self.norm2 = nn.GroupNorm(groups, cout, eps=GN_EPS)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1)
        self.conv_shortcut = nn.Conv2d(cin, cout, 1) if cin != cout else None


class Attention(nn.Module):
    def __init__(self, c: int, groups: int):
        super().__init__()
        self.group_norm = nn.GroupNorm(groups, c, eps=GN_EPS)
        self.to_q, self.to_k, self.to_v = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.to_out = nn.ModuleList([nn.Linear(c, c)])


class UNetMidBlock2D(nn.Module):
    def __init__(self, c: int, groups: int):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(c, c, groups), ResnetBlock2D(c, c, groups)])
        self.attentions = nn.ModuleList([Attention(c, groups)])


class Upsample2D(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 1, 1)


class UpDecoderBlock2D(nn.Module):
    def __init__(self, cin: int, cout: int, layers: int, groups: int, upsample: bool):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if i == 0 else cout, cout, groups) for i in range(layers)])
        if upsample:
            self.upsamplers = nn.ModuleList([Upsample2D(cout)])
        else:
            self.upsamplers = None


class Decoder(nn.Module):
    def __init__(self, cfg: VAEConfig):
        super().__init__()
        ch, g = cfg.block_out_channels, cfg.norm_num_groups
        self.conv_in = nn.Conv2d(cfg.latent_channels, ch[-1], 3, 1, 1)
        self.mid_block = UNetMidBlock2D(ch[-1], g)
        rev = list(reversed(ch))
        self.up_blocks = nn.ModuleList()
        cout = rev[0]
        for i, c in enumerate(rev):
            cin, cout = cout, c
            self.up_blocks.append(UpDecoderBlock2D(cin, cout, cfg.layers_per_block + 1, g, i != len(rev) - 1))
        self.conv_norm_out = nn.GroupNorm(g, ch[0], eps=GN_EPS)
        self.conv_out = nn.Conv2d(ch[0], cfg.out_channels, 3, 1, 1)


class Downsample2D(nn.Module):
    """diffusers ``Downsample2D(padding=0)``: the forward pads bottom / right by one, the conv itself has no padding."""

    def __init__(self, c: int):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 2, 0)


class DownEncoderBlock2D(nn.Module):
    def __init__(self, cin: int, cout: int, layers: int, groups: int, downsample: bool):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if i == 0 else cout, cout, groups) for i in range(layers)])
        if downsample:
            self.downsamplers = nn.ModuleList([Downsample2D(cout)])
        else:
            self.downsamplers = None


class Encoder(nn.Module):
    def __init__(self, cfg: VAEConfig):
        super().__init__()
        ch, g = cfg.block_out_channels, cfg.norm_num_groups
        self.conv_in = nn.Conv2d(3, ch[0], 3, 1, 1)
        self.down_blocks = nn.ModuleList()
        cout = ch[0]
        for i, c in enumerate(ch):
            cin, cout = cout, c
            self.down_blocks.append(DownEncoderBlock2D(cin, cout, cfg.layers_per_block, g, i != len(ch) - 1))
        self.mid_block = UNetMidBlock2D(ch[-1], g)
        self.conv_norm_out = nn.GroupNorm(g, ch[-1], eps=GN_EPS)
        self.conv_out = nn.Conv2d(ch[-1], 2 * cfg.latent_channels, 3, 1, 1)


class DecoderOutput:
    def __init__(self, sample: torch.Tensor):
        self.sample = sample


class DiagonalGaussianDistribution:
    """diffusers' posterior object: ``parameters`` = the moments (B, 2 * latent_channels, h, w) = [mean | logvar]."""

    def __init__(self, parameters: torch.Tensor):
        self.parameters = parameters
        self.mean, logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def sample(self, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        noise = torch.randn(self.mean.shape, generator=generator, device=self.parameters.device, dtype=self.parameters.dtype)
        return self.mean + self.std * noise

    def mode(self) -> torch.Tensor:
        return self.mean


class AutoencoderKLOutput:
    def __init__(self, latent_dist: DiagonalGaussianDistribution):
        self.latent_dist = latent_dist


# ---- launch plan ---------------------------------------------------------------------------------------------------------------
class _Pool:
    """Activation buffers of one plan.  The launches of a plan are stream-ordered, so a buffer whose last reader has been
    appended can be handed to the next producer: `take` returns the smallest free block that fits (else a new one),
    `give` returns a block.  Together with the build order of `_Builder` the tensors ping-pong between a few blocks."""

    def __init__(self, device):
        self.device = device
        self.free: List[torch.Tensor] = []
        self.all: List[torch.Tensor] = []

    def take(self, nbytes: int) -> torch.Tensor:
        fit = [b for b in self.free if b.numel() >= nbytes]
        if fit:
            b = min(fit, key=lambda t: t.numel())
            self.free = [t for t in self.free if t is not b]
            return b
        b = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.all.append(b)
        return b

    def give(self, b: torch.Tensor) -> None:
        self.free.append(b)

    def nbytes(self) -> int:
        return sum(b.numel() for b in self.all)


class _Act:
    """A channels-last bf16 activation [rows][cols] living in a pool block."""
    __slots__ = ("blk", "rows", "cols")

    def __init__(self, blk, rows, cols):
        self.blk, self.rows, self.cols = blk, rows, cols

    @property
    def ptr(self) -> int:
        return self.blk.data_ptr()


class VAEPlan:
    def __init__(self):
        self.ops: List[ops.Op] = []
        self.graph = None
        self.x_in: torch.Tensor = None       # fp32 (B, latent_channels, h, w): unscaled latents
        self.sample: torch.Tensor = None     # fp32 (B, 3, 8h, 8w)
        self.image: torch.Tensor = None      # uint8 (B, 8h, 8w, 3)
        self.pool: _Pool = None
        self.stats: torch.Tensor = None
        # encoder plans: the image (one of the two), the caller's noise, and the outputs (one of the two)
        self.image_f32: torch.Tensor = None  # fp32 (B, 3, H, W) in [-1, 1]
        self.image_u8: torch.Tensor = None   # uint8 (B, H, W, 3)
        self.noise: torch.Tensor = None      # fp32 (B, 4, H / 8, W / 8)
        self.moments: torch.Tensor = None    # fp32 (B, 8, H / 8, W / 8)
        self.latents: torch.Tensor = None    # fp32 (B, 4, H / 8, W / 8), scaled


class _Builder:
    """Forward-only plan of one (batch, h, w): its own small builder (no LoRA, no time embedding, no backward tape)."""

    def __init__(self, eng: "VAEEngine", B: int, h: int, w: int):
        self.eng, self.B, self.h, self.w = eng, B, h, w
        self.plan = VAEPlan()
        self.pool = self.plan.pool = _Pool(eng.device)
        self.out = self.plan.ops
        G = eng.cfg.norm_num_groups
        # GroupNorm statistics scratch, shared by every norm of the plan (the launches are ordered); the plan owns it
        self.stats = self.plan.stats = torch.zeros(B * G * 2 * 257, dtype=torch.float32, device=eng.device)

    def act(self, rows: int, cols: int) -> _Act:
        return _Act(self.pool.take(rows * cols * 2), rows, cols)

    def drop(self, a: _Act) -> None:
        self.pool.give(a.blk)

    def groupnorm(self, name: str, x: _Act, hw: int, act: int) -> _Act:
        gamma, beta = self.eng.norm_p[name]
        y = self.act(x.rows, x.cols)
        self.out.append(ops.groupnorm_fwd(x.ptr, x.cols, None, 0, 0, gamma, beta, self.B, hw, x.cols, self.eng.cfg.norm_num_groups,
                                          GN_EPS, act, self.stats, y.ptr, y.cols))
        return y

    def gemm(self, name: str, x: _Act, rows: int, *, conv=None, amode=A_PLAIN, residual: Optional[_Act] = None) -> _Act:
        w, bias = self.eng.gemm_w[name]
        n, k = w.shape
        y = self.act(rows, n)
        g = gemm_args(x.ptr, w, y.ptr, m=rows, n=n, k=k, lda=x.cols, a_mode=amode, conv=conv, bias=bias,
                      residual=None if residual is None else residual.ptr, ldr=0 if residual is None else residual.cols, ldc=n)
        self.out.append(ops.gemm(g, keep=(w, bias, x.blk, y.blk, None if residual is None else residual.blk), ws=self.eng.workspace))
        return y

    def resnet(self, name: str, x: _Act, hs: int, ws: int) -> _Act:
        hw, rows, conv = hs * ws, self.B * hs * ws, (self.B, hs, ws, hs, ws)
        n1 = self.groupnorm(name + ".norm1", x, hw, ACT_SILU)
        h1 = self.gemm(name + ".conv1", n1, rows, conv=conv, amode=A_CONV3_S1)
        self.drop(n1)
        n2 = self.groupnorm(name + ".norm2", h1, hw, ACT_SILU)
        self.drop(h1)
        if name + ".conv_shortcut" in self.eng.gemm_w:
            sc = self.gemm(name + ".conv_shortcut", x, rows)
            self.drop(x)
        else:
            sc = x
        y = self.gemm(name + ".conv2", n2, rows, conv=conv, amode=A_CONV3_S1, residual=sc)
        self.drop(n2)
        self.drop(sc)
        return y

    def attention(self, name: str, x: _Act, hw: int) -> _Act:
        Cc, rows = x.cols, x.rows
        n = self.groupnorm(name + ".group_norm", x, hw, ACT_NONE)
        qkv = self.gemm(name + ".qkv", n, rows)
        self.drop(n)
        o = self.act(rows, Cc)
        ld, p0 = 3 * Cc, qkv.ptr
        self.out.append(ops.Op("leco_attention_fwd", (p0, ld, hw * ld, p0 + 2 * Cc, ld, hw * ld, p0 + 4 * Cc, ld, hw * ld,
                                                      o.ptr, Cc, hw * Cc, None, self.B, 1, hw, hw, Cc, Cc ** -0.5),
                               keep=(qkv.blk, o.blk)))
        self.drop(qkv)
        y = self.gemm(name + ".to_out.0", o, rows, residual=x)
        self.drop(o)
        self.drop(x)
        return y

    def build(self) -> VAEPlan:
        eng, cfg, B, h, w = self.eng, self.eng.cfg, self.B, self.h, self.w
        dev, plan = eng.device, self.plan
        lc = cfg.latent_channels
        plan.x_in = torch.zeros(B, lc, h, w, dtype=torch.float32, device=dev)
        z = torch.zeros(B, lc, h, w, dtype=bf16, device=dev)
        self.out.append(ops.latent_affine(plan.x_in, eng.pq_w, eng.pq_b, z, B, h * w, lc, lc, 1.0 / cfg.scaling_factor))
        ctop = cfg.block_out_channels[-1]
        x = self.act(B * h * w, ctop)
        self.out.append(ops.Op("leco_conv_in", (z.data_ptr(), eng.conv_in_w.data_ptr(), eng.conv_in_b.data_ptr(), x.ptr, B, h, w, lc,
                                                ctop), keep=(z, x.blk)))
        x = self.resnet("decoder.mid_block.resnets.0", x, h, w)
        x = self.attention("decoder.mid_block.attentions.0", x, h * w)
        x = self.resnet("decoder.mid_block.resnets.1", x, h, w)
        hs, ws = h, w
        for i, blk in enumerate(eng.vae.decoder.up_blocks):
            for j in range(len(blk.resnets)):
                x = self.resnet(f"decoder.up_blocks.{i}.resnets.{j}", x, hs, ws)
            if blk.upsamplers is not None:
                y = self.gemm(f"decoder.up_blocks.{i}.upsamplers.0.conv", x, B * 4 * hs * ws, conv=(B, 2 * hs, 2 * ws, hs, ws),
                              amode=A_CONV3_UP2)
                self.drop(x)
                x, hs, ws = y, 2 * hs, 2 * ws
        n = self.groupnorm("decoder.conv_norm_out", x, hs * ws, ACT_SILU)
        self.drop(x)
        plan.sample = torch.zeros(B, cfg.out_channels, hs, ws, dtype=torch.float32, device=dev)
        plan.image = torch.zeros(B, hs, ws, cfg.out_channels, dtype=torch.uint8, device=dev)
        self.out.append(ops.Op("leco_conv_out_rgb", (n.ptr, eng.conv_out_w.data_ptr(), eng.conv_out_b.data_ptr(),
                                                     plan.sample.data_ptr(), plan.image.data_ptr(), B, hs, ws, n.cols), keep=(n.blk,)))
        return plan

    def build_encoder(self, u8: bool, out: str) -> VAEPlan:
        """(h, w) is the IMAGE size here.  `u8`: the 8-bit NHWC image instead of the fp32 NCHW one; `out`: "moments", "sample"
        (scaled latents from the caller's noise) or "mode" (scaled mean)."""
        eng, cfg, B, H, W = self.eng, self.eng.cfg, self.B, self.h, self.w
        dev, plan = eng.device, self.plan
        c0 = cfg.block_out_channels[0]
        if u8:
            plan.image_u8 = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=dev)
        else:
            plan.image_f32 = torch.zeros(B, 3, H, W, dtype=torch.float32, device=dev)
        x = self.act(B * H * W, c0)
        self.out.append(ops.Op("leco_conv_in_rgb", (hip.ptr(plan.image_f32), hip.ptr(plan.image_u8), eng.enc_in_w.data_ptr(),
                                                    eng.enc_in_b.data_ptr(), x.ptr, B, H, W, c0), keep=(x.blk,)))
        hs, ws = H, W
        for i, blk in enumerate(eng.vae.encoder.down_blocks):
            for j in range(len(blk.resnets)):
                x = self.resnet(f"encoder.down_blocks.{i}.resnets.{j}", x, hs, ws)
            if blk.downsamplers is not None:
                y = self.gemm(f"encoder.down_blocks.{i}.downsamplers.0.conv", x, B * (hs // 2) * (ws // 2),
                              conv=(B, hs // 2, ws // 2, hs, ws), amode=A_CONV3_S2_PAD01)
                self.drop(x)
                x, hs, ws = y, hs // 2, ws // 2
        x = self.resnet("encoder.mid_block.resnets.0", x, hs, ws)
        x = self.attention("encoder.mid_block.attentions.0", x, hs * ws)
        x = self.resnet("encoder.mid_block.resnets.1", x, hs, ws)
        n = self.groupnorm("encoder.conv_norm_out", x, hs * ws, ACT_SILU)
        self.drop(x)
        lc = cfg.latent_channels
        if out == "moments":
            plan.moments = torch.zeros(B, 2 * lc, hs, ws, dtype=torch.float32, device=dev)
        else:
            plan.latents = torch.zeros(B, lc, hs, ws, dtype=torch.float32, device=dev)
            if out == "sample":
                plan.noise = torch.zeros(B, lc, hs, ws, dtype=torch.float32, device=dev)
        self.out.append(ops.Op("leco_conv_out_moments", (n.ptr, eng.enc_out_w.data_ptr(), eng.enc_out_b.data_ptr(), eng.q_w.data_ptr(),
                                                         eng.q_b.data_ptr(), hip.ptr(plan.noise), hip.ptr(plan.moments),
                                                         hip.ptr(plan.latents), float(cfg.scaling_factor), B, hs, ws, n.cols),
                               keep=(n.blk,)))
        return plan


class VAEEngine(graphs.PlanEngine):
    """Packed device operands of one AutoencoderKL and its launch plans, keyed by (batch, h, w)."""

    def __init__(self, vae: "AutoencoderKL", device: torch.device):
        super().__init__(device)
        self.vae, self.cfg = vae, vae.cfg
        cfg = self.cfg
        if cfg.out_channels != 3:
            raise ValueError(f"VAE decoder: out_channels = {cfg.out_channels}, the image epilogue writes RGB")
        ctop = cfg.block_out_channels[-1]
        if ctop not in WIDE_HEAD_DIMS:
            raise ValueError(f"VAE decoder: the mid-block attention is one head of width {ctop}; the attention kernel is built for "
                             f"{WIDE_HEAD_DIMS}")
        if any(c % 32 for c in cfg.block_out_channels):
            raise ValueError("VAE decoder: block_out_channels must be multiples of 32")
        self.workspace = torch.empty(8 * 1024 * 1024, dtype=torch.float32, device=device)    # split-K partial slabs
        f32 = lambda t: t.detach().float().to(device).contiguous()      # noqa: E731
        self.gemm_w: Dict[str, Tuple[torch.Tensor, Optional[torch.Tensor]]] = {}
        self.norm_p: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        for name, m in vae.named_modules():
            if isinstance(m, nn.GroupNorm):
                self.norm_p[name] = (f32(m.weight), f32(m.bias))
            elif isinstance(m, Attention):
                w = torch.cat([m.to_q.weight, m.to_k.weight, m.to_v.weight], 0).detach()
                b = torch.cat([m.to_q.bias, m.to_k.bias, m.to_v.bias], 0)
                self.gemm_w[name + ".qkv"] = (w.to(device, bf16).contiguous(), f32(b))
                self.gemm_w[name + ".to_out.0"] = (m.to_out[0].weight.detach().to(device, bf16).contiguous(), f32(m.to_out[0].bias))
            elif isinstance(m, nn.Conv2d) and name not in ("post_quant_conv", "decoder.conv_in", "decoder.conv_out", "quant_conv",
                                                            "encoder.conv_in", "encoder.conv_out"):
                w = m.weight.detach()
                w = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)           # [N][kh][kw][Cin]
                self.gemm_w[name] = (w.to(device, bf16).contiguous(), f32(m.bias))
        d = vae.decoder
        lc = cfg.latent_channels
        self.pq_w, self.pq_b = f32(vae.post_quant_conv.weight.reshape(lc, lc)), f32(vae.post_quant_conv.bias)
        self.conv_in_w, self.conv_in_b = f32(d.conv_in.weight.detach().permute(1, 2, 3, 0)), f32(d.conv_in.bias)     # [Cin][3][3][Cout]
        self.conv_out_w = d.conv_out.weight.detach().permute(0, 2, 3, 1).contiguous().to(device, bf16)                # [3][3][3][C]
        self.conv_out_b = f32(d.conv_out.bias)
        if vae.encoder is not None:
            e = vae.encoder
            self.enc_in_w, self.enc_in_b = f32(e.conv_in.weight), f32(e.conv_in.bias)                                  # [Cout][3][3][3]
            self.enc_out_w = e.conv_out.weight.detach().permute(0, 2, 3, 1).contiguous().to(device, bf16)              # [8][3][3][C]
            self.enc_out_b = f32(e.conv_out.bias)
            self.q_w, self.q_b = f32(vae.quant_conv.weight.reshape(2 * lc, 2 * lc)), f32(vae.quant_conv.bias)          # fp32, never folded

    def encoder_plan(self, B: int, H: int, W: int, u8: bool, out: str) -> VAEPlan:
        """Keyed beside the decoder's plans; (H, W) is the image size."""
        if H % 8 or W % 8 or H <= 0 or W <= 0:
            raise ValueError(f"VAE encode: image height and width must be multiples of 8, got {H} x {W}")
        return self.cached(("encode", B, H, W, bool(u8), out), lambda: _Builder(self, B, H, W).build_encoder(bool(u8), out))

    def plan(self, B: int, h: int, w: int) -> VAEPlan:
        return self.cached((B, h, w), lambda: _Builder(self, B, h, w).build())


class AutoencoderKL(graphs.ForwardOnlyModel):
    """diffusers' ``AutoencoderKL``.  The decoder half is always built; ``encoder=True`` adds ``encoder`` and ``quant_conv``
    (after the decoder, so the decoder-only module tree and ``state_dict()`` are a prefix of the full one).  `decode` takes
    the sampler's latents as they are and divides by ``config.scaling_factor`` itself; `encode` follows diffusers (no
    scaling factor), `encode_to_latents` returns scaled latents."""
    engine_type = VAEEngine
    label = "VAE decoder"
    bf16_only = "bfloat16 only; `train.precision: float32` does not extend to the decoder"

    def __init__(self, cfg: Optional[VAEConfig] = None, encoder: bool = False):
        super().__init__(use_graphs=False)
        self.cfg = cfg or VAEConfig()
        self.post_quant_conv = nn.Conv2d(self.cfg.latent_channels, self.cfg.latent_channels, 1)
        self.decoder = Decoder(self.cfg)
        self.encoder: Optional[Encoder] = None
        self.quant_conv: Optional[nn.Conv2d] = None
        if encoder:
            if self.cfg.latent_channels != 4:
                raise ValueError(f"VAE encoder: latent_channels = {self.cfg.latent_channels}; the moments kernel is built for 4 "
                                 "(8 moment channels)")
            self.encoder = Encoder(self.cfg)
            self.quant_conv = nn.Conv2d(2 * self.cfg.latent_channels, 2 * self.cfg.latent_channels, 1)
        self.requires_grad_(False)

    @property
    def device(self):
        return self.post_quant_conv.weight.device

    def _decode(self, latents: torch.Tensor) -> VAEPlan:
        if latents.ndim != 4 or latents.shape[1] != self.cfg.latent_channels:
            raise ValueError(f"VAE decode: latents must be (B, {self.cfg.latent_channels}, h, w), got {tuple(latents.shape)}")
        B, _, h, w = latents.shape
        plan = self.engine().plan(B, h, w)
        plan.x_in.copy_(latents)
        self._run(plan)
        return plan

    @torch.no_grad()
    def decode(self, latents: torch.Tensor, return_dict: bool = True):
        """``latents``: the sampler's output (B, 4, h, w), NOT divided by the scaling factor (the division is folded into the
        first launch).  Returns an object with ``.sample``: fp32 (B, 3, 8h, 8w), nominally in [-1, 1]."""
        sample = self._decode(latents).sample.clone()
        return DecoderOutput(sample) if return_dict else (sample,)

    @torch.no_grad()
    def decode_to_uint8(self, latents: torch.Tensor) -> torch.Tensor:
        """(B, 8h, 8w, 3) uint8 pixels: floor(clamp(sample / 2 + 0.5, 0, 1) * 255 + 0.5), from the output convolution's epilogue."""
        return self._decode(latents).image.clone()

    # ---- encoder ----
    def _encode(self, image: torch.Tensor, out: str, generator: Optional[torch.Generator] = None) -> VAEPlan:
        """`out` = "sample": the noise is drawn here, once the image's shape has been validated and its plan found."""
        if self.encoder is None:
            raise RuntimeError("VAE encode: this model was built without its encoder; load it with encoder=True "
                               "(AutoencoderKL(cfg, encoder=True) / model_util.load_vae(path, encoder=True))")
        u8 = image.dtype == torch.uint8
        if u8:
            if image.ndim != 4 or image.shape[3] != 3:
                raise ValueError(f"VAE encode: an 8-bit image must be (B, H, W, 3), got {tuple(image.shape)}")
            B, H, W, _ = image.shape
        else:
            if image.ndim != 4 or image.shape[1] != 3 or not image.is_floating_point():
                raise ValueError(f"VAE encode: the image must be float (B, 3, H, W) in [-1, 1], got {tuple(image.shape)} {image.dtype}")
            B, _, H, W = image.shape
        plan = self.engine().encoder_plan(B, H, W, u8, out)
        (plan.image_u8 if u8 else plan.image_f32).copy_(image)
        if out == "sample":
            plan.noise.copy_(torch.randn(plan.noise.shape, generator=generator, device=plan.noise.device, dtype=torch.float32))
        self._run(plan)
        return plan

    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """``x``: float (B, 3, H, W) in [-1, 1], H and W multiples of 8.  Returns an object with ``.latent_dist`` (diffusers'
        ``DiagonalGaussianDistribution``: ``parameters`` fp32 (B, 8, H/8, W/8), ``mean``, ``logvar``, ``std``, ``var``, ``mode()``,
        ``sample(generator)``).  No scaling factor is applied, as in diffusers."""
        if x.dtype == torch.uint8:
            raise ValueError("VAE encode: takes the float image in [-1, 1]; encode_to_latents takes 8-bit images")
        dist = DiagonalGaussianDistribution(self._encode(x, "moments").moments.clone())
        return AutoencoderKLOutput(dist) if return_dict else (dist,)

    @torch.no_grad()
    def encode_to_latents(self, image: torch.Tensor, generator: Optional[torch.Generator] = None, sample: bool = True) -> torch.Tensor:
        """``image``: float (B, 3, H, W) in [-1, 1] or uint8 (B, H, W, 3).  fp32 (B, 4, H/8, W/8) latents times
        ``config.scaling_factor`` -- what a sampler starts from -- drawn from the posterior with torch's RNG (``sample=False``:
        its mode), from the output convolution's epilogue."""
        return self._encode(image, "sample" if sample else "mode", generator).latents.clone()


def init_synthetic_vae_(vae: AutoencoderKL, seed: int = 4321, encoder_seed: int = 8765) -> AutoencoderKL:
    """The decoder half is drawn exactly as for a decoder-only model; the encoder half from a generator of its own."""
    from .model_util import init_synthetic_
    if vae.encoder is None:
        init_synthetic_(vae, seed)
        return vae
    dec, enc = nn.Module(), nn.Module()
    dec.post_quant_conv, dec.decoder = vae.post_quant_conv, vae.decoder
    enc.encoder, enc.quant_conv = vae.encoder, vae.quant_conv
    init_synthetic_(dec, seed)
    init_synthetic_(enc, encoder_seed)
    return vae


# ---- PNG -----------------------------------------------------------------------------------------------------------------------
def _png_bytes(img) -> bytes:
    h, w, _ = img.shape
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))      # filter type 0 on every scanline

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def save_png(uint8_hwc, path: str) -> None:
    """Write one (H, W, 3) uint8 image as an 8-bit RGB PNG: PIL when importable, else a zlib writer of its own."""
    t = torch.as_tensor(uint8_hwc)
    if t.ndim != 3 or t.shape[2] != 3 or t.dtype != torch.uint8:
        raise ValueError(f"save_png: expected (H, W, 3) uint8, got {tuple(t.shape)} {t.dtype}")
    arr = t.detach().cpu().contiguous().numpy()
    try:
        from PIL import Image
    except ImportError:
        with open(path, "wb") as f:
            f.write(_png_bytes(arr))
        return
    Image.fromarray(arr, "RGB").save(path, format="PNG")


def _paeth(a: int, b: int, c: int) -> int:
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def load_png(path: str) -> torch.Tensor:
    """Read an 8-bit, non-interlaced PNG of colour type 0 (grey, replicated), 2 (RGB) or 6 (RGBA, alpha dropped) as a
    (H, W, 3) uint8 tensor; all five scanline filters; zlib only.  Anything else is a ValueError saying what was found."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"load_png: {path} is not a PNG file (signature {raw[:8]!r})")
    pos, ihdr, idat = 8, None, []
    while pos + 8 <= len(raw):
        n, tag = struct.unpack(">I", raw[pos:pos + 4])[0], raw[pos + 4:pos + 8]
        data = raw[pos + 8:pos + 8 + n]
        if len(data) != n:
            raise ValueError(f"load_png: {path}: chunk {tag!r} is truncated")
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", data)
        elif tag == b"IDAT":
            idat.append(data)
        elif tag == b"IEND":
            break
        pos += 12 + n
    if ihdr is None:
        raise ValueError(f"load_png: {path}: no IHDR chunk")
    w, h, depth, colour, _, _, interlace = ihdr
    if depth != 8:
        raise ValueError(f"load_png: {path}: bit depth {depth}; only 8-bit files are read")
    if colour not in (0, 2, 6):
        raise ValueError(f"load_png: {path}: colour type {colour}; only 0 (grey), 2 (RGB) and 6 (RGBA) are read")
    if interlace != 0:
        raise ValueError(f"load_png: {path}: interlace method {interlace}; only non-interlaced files are read")
    bpp = {0: 1, 2: 3, 6: 4}[colour]
    stride = w * bpp
    data = zlib.decompress(b"".join(idat))
    if len(data) != h * (stride + 1):
        raise ValueError(f"load_png: {path}: {len(data)} bytes of image data, expected {h * (stride + 1)}")
    out = bytearray(h * stride)
    prev = bytearray(stride)
    for y in range(h):
        ft = data[y * (stride + 1)]
        line = bytearray(data[y * (stride + 1) + 1:(y + 1) * (stride + 1)])
        if ft == 1:
            for i in range(bpp, stride):
                line[i] = (line[i] + line[i - bpp]) & 255
        elif ft == 2:
            for i in range(stride):
                line[i] = (line[i] + prev[i]) & 255
        elif ft == 3:
            for i in range(stride):
                line[i] = (line[i] + (((line[i - bpp] if i >= bpp else 0) + prev[i]) >> 1)) & 255
        elif ft == 4:
            for i in range(stride):
                line[i] = (line[i] + _paeth(line[i - bpp] if i >= bpp else 0, prev[i], prev[i - bpp] if i >= bpp else 0)) & 255
        elif ft != 0:
            raise ValueError(f"load_png: {path}: scanline {y} has filter type {ft}")
        out[y * stride:(y + 1) * stride] = line
        prev = line
    img = torch.frombuffer(out, dtype=torch.uint8).reshape(h, w, bpp)
    if colour == 0:
        return img.expand(h, w, 3).contiguous()
    return img[:, :, :3].contiguous()
