"""The CLIP image tower (transformers' ``CLIPVisionModelWithProjection``: ViT-L/14 of OpenAI CLIP, ViT-H/14 of OpenCLIP) on
the HIP kernels, its image preprocessing on the device, and the CLIP score: the cosine between the image embedding of a
picture and the text embedding of a prompt -- the number that says how much of a concept a LoRA left in a sample.

The module tree only HOLDS weights under the transformers parameter names (``vision_model.embeddings.{class_embedding,
patch_embedding.weight, position_embedding.weight}``, ``vision_model.pre_layrnorm`` (sic), ``vision_model.encoder.layers.N.*``,
``vision_model.post_layernorm``, ``visual_projection.weight``), so an HF state dict -- or that part of a full ``CLIPModel``
file, `vision_state_dict` -- loads with ``load_state_dict`` as is.  A call runs a forward-only launch plan per batch size
(and, for raw pixels, per picture size): bf16 activations, fp32 accumulation; replayed from a hipGraph when ``use_graphs``
is set.  The N layers are the stack of ``encoder.py``, shared with the text encoder.  T = (image_size / patch_size)^2 patches,
T + 1 tokens:

    [raw pixels only] resize + crop + normalise + patchify   leco_clip_preprocess
    patch embedding (no bias), K = 3 p p padded to 64        leco_gemm
    class token + patches + position embedding               leco_vit_embed
    pre_layrnorm                                             leco_layernorm_fwd
    N x  layer_norm1                                         leco_layernorm_fwd
         fused q|k|v Linear                                  leco_gemm
         attention, 64- / 80-wide heads, T + 1 keys          leco_attention_fwd
         out_proj + residual                                 leco_gemm
         layer_norm2                                         leco_layernorm_fwd
         fc1 + quick-GELU / GELU                             leco_gemm (LECO_ACT_QUICK_GELU / LECO_ACT_GELU)
         fc2 + residual                                      leco_gemm
    class-token row per sample                               leco_embed_rows (no position table)
    post_layernorm                                           leco_layernorm_fwd
    visual_projection (no bias)                              leco_gemm
    [ClipScorer] cosines against the text embeddings         leco_cosine_scores

The preprocessing filter is PIL's ``Image.resize(..., BICUBIC)`` as transformers' ``CLIPImageProcessor`` calls it: separable,
Keys' cubic with a = -0.5, its support (2 pixels) scaled by the downscale factor (antialiasing), window clamped to the
picture and renormalised at the borders, columns first, then rows, both intermediate and final values saturating at
[0, 255].  `resize_taps` states PIL's ``precompute_coeffs`` in floating point; the kernel keeps fp32 where PIL rounds to whole
8-bit levels twice, so a value differs from PIL's by at most 0.5 * sum |row taps| + 0.5 levels (+ PIL's fixed-point taps).

bf16 only, heads of 64 or 80 (ViT-bigG's 104 is refused), no backward; the tokenizer of the scorer stays transformers'.
"""
from __future__ import annotations

import hashlib
import json
import math
from dataclasses import dataclass, fields
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import nn

from . import graphs, ops
from .clip import CLIPEncoder
from .encoder import ACTS, LN_EPS, EncoderEngine, EncoderPlan, bf16, f32, init_synthetic_encoder_, pack_encoder_layers, wb

HEAD_DIMS = (64, 80)             # the widths of leco_attention_fwd a CLIP image tower uses
OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


@dataclass
class CLIPVisionConfig:
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    image_size: int = 224
    patch_size: int = 14
    hidden_act: str = "quick_gelu"
    projection_dim: int = 768
    layer_norm_eps: float = LN_EPS
    image_mean: Tuple[float, float, float] = OPENAI_CLIP_MEAN
    image_std: Tuple[float, float, float] = OPENAI_CLIP_STD

    def __post_init__(self):
        self.image_mean, self.image_std = tuple(float(v) for v in self.image_mean), tuple(float(v) for v in self.image_std)
        if self.hidden_act not in ACTS:
            raise ValueError(f"CLIP image tower: hidden_act {self.hidden_act!r} is not one of {sorted(ACTS)}")
        if self.num_attention_heads <= 0 or self.hidden_size % self.num_attention_heads \
                or self.hidden_size // self.num_attention_heads not in HEAD_DIMS:
            raise ValueError(f"CLIP image tower: hidden_size {self.hidden_size} / num_attention_heads {self.num_attention_heads} "
                             f"must be one of {HEAD_DIMS}: the attention kernel has no "
                             f"{self.hidden_size / max(1, self.num_attention_heads):g}-wide heads (ViT-bigG's 104 is not supported)")
        if self.hidden_size % 64 or self.intermediate_size % 64 or self.projection_dim % 8 or self.num_hidden_layers < 1:
            raise ValueError("CLIP image tower: hidden_size and intermediate_size must be multiples of 64, projection_dim of 8, "
                             "and there must be at least one layer")
        if self.patch_size < 1 or self.image_size < self.patch_size or self.image_size % self.patch_size:
            raise ValueError(f"CLIP image tower: image_size {self.image_size} must be a multiple of patch_size {self.patch_size}")
        if len(self.image_mean) != 3 or len(self.image_std) != 3 or min(self.image_std) <= 0:
            raise ValueError("CLIP image tower: image_mean / image_std must be three values each, the std positive")

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads

    @property
    def num_patches(self) -> int:
        return (self.image_size // self.patch_size) ** 2

    @property
    def patch_k(self) -> int:
        """Row length of the patch operand: 3 p p rounded up to a multiple of 64 (588 -> 640)."""
        return -(-3 * self.patch_size ** 2 // 64) * 64

    @classmethod
    def from_dict(cls, d: dict, **override) -> "CLIPVisionConfig":
        known = {f.name for f in fields(cls)}
        kw = {k: v for k, v in d.items() if k in known and v is not None}
        kw.update(override)
        return cls(**kw)

    @classmethod
    def from_json(cls, path: str, **override) -> "CLIPVisionConfig":
        """A ``CLIPVisionModelWithProjection`` ``config.json``, or a ``CLIPModel`` one (its ``vision_config``; the projection
        width is the model's ``projection_dim``)."""
        with open(path) as f:
            d = json.load(f)
        if "vision_config" in d:
            d = {**d["vision_config"], **({"projection_dim": d["projection_dim"]} if d.get("projection_dim") else {})}
        return cls.from_dict(d, **override)


def vit_l_14_config(**kw) -> CLIPVisionConfig:
    return CLIPVisionConfig(**kw)


def vit_h_14_config(**kw) -> CLIPVisionConfig:
    return CLIPVisionConfig(**{**dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16,
                                      hidden_act="gelu", projection_dim=1024), **kw})


def vit_tiny_config(**kw) -> CLIPVisionConfig:
    """``synthetic:vit_tiny``: 128 wide, 2 heads of 64, 2 layers, 56 / 14 (17 tokens)."""
    return CLIPVisionConfig(**{**dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                      image_size=56, patch_size=14, projection_dim=64), **kw})


# ---- the preprocessing filter (host side) ----------------------------------------------------------------------------------------
def _bicubic(x: float) -> float:
    """Keys' cubic, a = -0.5 (PIL's ``bicubic_filter``)."""
    a, x = -0.5, abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_taps(in_size: int, out_size: int, first: int = 0, count: Optional[int] = None):
    """PIL's ``precompute_coeffs`` for the bicubic filter, one axis, in floating point: for each of the output positions
    ``first .. first + count`` of a resize ``in_size -> out_size`` the first source index, the tap count and the normalised
    weights.  Returns ``(tab int32 [count][2], weights float64 [count][taps], taps)``."""
    count = out_size - first if count is None else count
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    taps = int(math.ceil(support)) * 2 + 1
    tab = torch.zeros(count, 2, dtype=torch.int32)
    w = torch.zeros(count, taps, dtype=torch.float64)
    for i in range(count):
        center = (first + i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        k = [_bicubic((x + lo - center + 0.5) / fscale) for x in range(hi - lo)]
        total = sum(k)
        if total != 0.0:
            k = [v / total for v in k]
        tab[i, 0], tab[i, 1] = lo, hi - lo
        w[i, :hi - lo] = torch.tensor(k, dtype=torch.float64)
    return tab, w, taps


def preprocess_geometry(h: int, w: int, size: int):
    """``CLIPImageProcessor``'s geometry: the resized (height, width) -- shortest edge ``size``, the other
    ``int(size * long / short)`` -- and the (top, left) of the centre crop."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    nh, nw = (new_long, size) if w <= h else (size, new_long)
    return nh, nw, (nh - size) // 2, (nw - size) // 2


def preprocess_tables(h: int, w: int, size: int):
    """Row and column tap tables of an ``h x w`` picture for `leco_clip_preprocess`: only what survives the crop."""
    nh, nw, top, left = preprocess_geometry(h, w, size)
    return resize_taps(h, nh, top, size), resize_taps(w, nw, left, size)


def patchify(pixel_values: torch.Tensor, patch: int, kp: int) -> torch.Tensor:
    """Float [B,3,S,S] -> [B * P][kp]: column c p p + i p + j of row (b, py, px) = pixel_values[b, c, py p + i, px p + j]."""
    B, _, S, _ = pixel_values.shape
    g = S // patch
    rows = pixel_values.reshape(B, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * patch * patch)
    return torch.nn.functional.pad(rows, (0, kp - rows.shape[1]))


# ---- weight holders (transformers names) ---------------------------------------------------------------------------------------
class CLIPVisionEmbeddings(nn.Module):
    def __init__(self, cfg: CLIPVisionConfig):
        super().__init__()
        self.class_embedding = nn.Parameter(torch.zeros(cfg.hidden_size))
        self.patch_embedding = nn.Conv2d(3, cfg.hidden_size, cfg.patch_size, cfg.patch_size, bias=False)
        self.position_embedding = nn.Embedding(cfg.num_patches + 1, cfg.hidden_size)


class CLIPVisionTransformer(nn.Module):
    def __init__(self, cfg: CLIPVisionConfig):
        super().__init__()
        self.embeddings = CLIPVisionEmbeddings(cfg)
        self.pre_layrnorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.encoder = CLIPEncoder(cfg)
        self.post_layernorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class CLIPVisionOutput:
    """``[0]`` / ``.image_embeds``, ``.last_hidden_state`` (the encoder's output, before ``post_layernorm``),
    ``.pooler_output`` (``post_layernorm`` of the class token)."""

    def __init__(self, image_embeds, last_hidden_state, pooler_output):
        self.image_embeds, self.last_hidden_state, self.pooler_output = image_embeds, last_hidden_state, pooler_output

    def __getitem__(self, i):
        return (self.image_embeds, self.last_hidden_state)[i]

    def __iter__(self):
        return iter((self.image_embeds, self.last_hidden_state))


# ---- launch plan ---------------------------------------------------------------------------------------------------------------
class VisionPlan(EncoderPlan):
    def __init__(self):
        super().__init__()
        self.img: Optional[torch.Tensor] = None  # uint8 [B][H][W][3]: raw pixels (plans of `encode_images` only)
        self.patches: torch.Tensor = None        # bf16 [B * T][Kp]: the patch GEMM's operand
        self.last: torch.Tensor = None           # bf16 [B * (T + 1)][C]: the encoder's output
        self.pooled: torch.Tensor = None         # bf16 [B][C]
        self.image_embeds: torch.Tensor = None   # bf16 [B][projection_dim]


class VisionEngine(EncoderEngine):
    """Packed device operands of one image tower and its launch plans, keyed by (batch,) for preprocessed pixels and by
    (batch, height, width) for raw ones."""

    def __init__(self, model: "CLIPVisionModelWithProjection", device: torch.device):
        cfg, vm = model.cfg, model.vision_model
        super().__init__(cfg, device)
        pw = vm.embeddings.patch_embedding.weight.detach().reshape(cfg.hidden_size, -1)
        self.patch_w = wb(torch.nn.functional.pad(pw, (0, cfg.patch_k - pw.shape[1])), device)
        self.cls, self.pos = wb(vm.embeddings.class_embedding, device), wb(vm.embeddings.position_embedding.weight, device)
        self.gemm_w, self.norm_p = pack_encoder_layers(vm.encoder.layers, device)
        self.norm_p["pre"] = (f32(vm.pre_layrnorm.weight, device), f32(vm.pre_layrnorm.bias, device))
        self.norm_p["post"] = (f32(vm.post_layernorm.weight, device), f32(vm.post_layernorm.bias, device))
        self.proj_w = wb(model.visual_projection.weight, device)
        self.mean_std = torch.tensor(cfg.image_mean + cfg.image_std, dtype=torch.float32, device=device)
        self.tables: Dict[Tuple[int, int], tuple] = {}

    def _tables(self, h: int, w: int):
        """The tap tables of an h x w picture on the device (computed once per picture size)."""
        t = self.tables.get((h, w))
        if t is None:
            (rt, rw, rk), (ct, cw, ck) = preprocess_tables(h, w, self.cfg.image_size)
            for tab, size in ((rt, h), (ct, w)):         # what the kernel would otherwise clamp: a wrong table is an error here
                if int(tab[:, 0].min()) < 0 or int((tab[:, 0] + tab[:, 1]).max()) > size or int(tab[:, 1].min()) < 1:
                    raise ValueError(f"CLIP preprocessing: tap table outside a {h}x{w} picture")
            dev = self.device
            t = self.tables[(h, w)] = (rt.to(dev), rw.float().to(dev), rk, ct.to(dev), cw.float().to(dev), ck)
        return t

    # -- plan construction ----------------------------------------------------------------------------------------------------
    def _build(self, B: int, hw: Optional[Tuple[int, int]]) -> VisionPlan:
        cfg, dev = self.cfg, self.device
        Cw, H, D = cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim
        T, Kp = cfg.num_patches, cfg.patch_k
        S, M = T + 1, B * (T + 1)
        p, buf = VisionPlan(), self.buf
        p.patches = buf(B * T, Kp)
        pe, x0 = buf(B * T, Cw), buf(M, Cw)
        xa, xb = buf(M, Cw), buf(M, Cw)              # the residual stream ping-pongs between two buffers
        self.scratch(p, M)
        lse = torch.zeros(B * H * S, device=dev)
        cls_idx = (torch.arange(B, dtype=torch.int32) * S).to(dev)
        cls_row = buf(B, Cw)
        p.keep = [pe, x0, xa, xb, lse, cls_idx, cls_row]

        def attention(qkv, att):
            q0, ld = qkv.data_ptr(), 3 * Cw
            return ops.attention_fwd(q0, ld, S * ld, q0 + 2 * Cw, ld, S * ld, q0 + 4 * Cw, ld, S * ld, att.data_ptr(),
                                     Cw, S * Cw, lse, B, H, S, S, D, D ** -0.5)

        if hw is not None:
            h, w = hw
            p.img = torch.zeros(B, h, w, 3, dtype=torch.uint8, device=dev)
            rt, rw, rk, ct, cw, ck = self._tables(h, w)
            p.add("preprocess", ops.clip_preprocess(p.img, B, h, w, rt, rw, rk, ct, cw, ck, self.mean_std, cfg.image_size,
                                                    cfg.patch_size, p.patches, Kp))
        self.gemm(p, "patch_embed", self.patch_w, None, p.patches, pe, B * T, Kp)
        p.add("embed", ops.vit_embed(pe, Cw, self.cls, self.pos, Cw, x0, Cw, B, T, Cw))
        self.ln(p, "pre", x0, xa, M)
        x, y = xa, xb
        for i in range(cfg.num_hidden_layers):
            self.layer(p, i, x, y, M, attention)
            x, y = y, x
        p.last = x
        p.add("cls_gather", ops.embed_rows(p.last, Cw, M, cls_idx, None, 0, 1, cls_row, Cw, B, Cw))
        p.pooled = buf(B, Cw)
        self.ln(p, "post", cls_row, p.pooled, B)
        p.image_embeds = buf(B, cfg.projection_dim)
        self.gemm(p, "projection", self.proj_w, None, p.pooled, p.image_embeds, B, Cw)
        return p

    def plan(self, B: int, hw: Optional[Tuple[int, int]] = None) -> VisionPlan:
        return self.cached((B,) if hw is None else (B, *hw), lambda: self._build(B, hw))


class CLIPVisionModelWithProjection(graphs.ForwardOnlyModel):
    """transformers' ``CLIPVisionModelWithProjection``, forward only."""
    engine_type = VisionEngine
    label = "CLIP image tower"

    def __init__(self, cfg: Optional[CLIPVisionConfig] = None):
        super().__init__(use_graphs=True)
        self.cfg = cfg or CLIPVisionConfig()
        self.vision_model = CLIPVisionTransformer(self.cfg)
        self.visual_projection = nn.Linear(self.cfg.hidden_size, self.cfg.projection_dim, bias=False)
        self.requires_grad_(False)

    @property
    def device(self):
        return self.visual_projection.weight.device

    @property
    def dtype(self):
        return self.visual_projection.weight.dtype

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """An HF state dict as is; a wrong key is a KeyError."""
        sd = state_dict
        if sd and not any(k.startswith("vision_model.") for k in sd):      # a transformers that saves without the prefix
            sd = {(k if k.startswith("visual_projection.") else "vision_model." + k): v for k, v in sd.items()}
        return self.load_strict(sd, strict, **kw)

    def _output(self, plan: VisionPlan, B: int) -> CLIPVisionOutput:
        out = self.copy_out
        return CLIPVisionOutput(out(plan.image_embeds, B, -1), out(plan.last, B, self.cfg.num_patches + 1, -1),
                                out(plan.pooled, B, -1))

    @torch.no_grad()
    def forward(self, pixel_values, **kw) -> CLIPVisionOutput:
        """``pixel_values``: float [B,3,S,S], already resized, cropped and normalised (what ``CLIPImageProcessor`` returns)."""
        px = torch.as_tensor(pixel_values)
        S = self.cfg.image_size
        if px.ndim != 4 or px.shape[0] < 1 or tuple(px.shape[1:]) != (3, S, S) or not px.dtype.is_floating_point:
            raise ValueError(f"CLIP image tower: pixel_values must be a float [batch][3][{S}][{S}] tensor, got "
                             f"{tuple(px.shape)} {px.dtype}")
        B = px.shape[0]
        plan = self.engine().plan(B)
        plan.patches.copy_(patchify(px.to(self.device).float(), self.cfg.patch_size, self.cfg.patch_k))
        self._run(plan)
        return self._output(plan, B)

    @torch.no_grad()
    def encode_images_output(self, img_u8) -> CLIPVisionOutput:
        img = torch.as_tensor(img_u8)
        if img.ndim != 4 or img.shape[-1] != 3 or img.dtype != torch.uint8 or min(img.shape) < 1:
            raise ValueError(f"CLIP image tower: images must be a uint8 [batch][height][width][3] tensor, got "
                             f"{tuple(img.shape)} {img.dtype}")
        B, h, w, _ = img.shape
        plan = self.engine().plan(B, (h, w))
        plan.img.copy_(img)
        self._run(plan)
        return self._output(plan, B)

    def encode_images(self, img_u8) -> torch.Tensor:
        """uint8 [B,H,W,3] pictures (device or CPU, any H, W >= 1) -> ``image_embeds`` [B][projection_dim]; resized, cropped
        and normalised on the device as ``CLIPImageProcessor`` does (`leco_clip_preprocess`)."""
        return self.encode_images_output(img_u8).image_embeds


def init_synthetic_clip_vision_(model: CLIPVisionModelWithProjection, seed: int = 1357) -> CLIPVisionModelWithProjection:
    """Seeded stand-in weights (`encoder.init_synthetic_encoder_`)."""
    return init_synthetic_encoder_(model, seed)


def vision_state_dict(sd: dict) -> dict:
    """The image tower's part of a full ``CLIPModel`` state dict: ``vision_model.*`` and ``visual_projection.weight``."""
    return {k: v for k, v in sd.items() if k.startswith("vision_model.") or k.startswith("visual_projection.")}


def text_state_dict(sd: dict) -> dict:
    """The text tower's part of a full ``CLIPModel`` state dict: ``text_model.*`` and ``text_projection.weight``."""
    return {k: v for k, v in sd.items() if k.startswith("text_model.") or k.startswith("text_projection.")}


# ---- the score -----------------------------------------------------------------------------------------------------------------
class SyntheticTokenizer:
    """Stand-in of ``synthetic:*`` scorers: the "token ids" are the prompt strings."""
    model_max_length = 77

    def __call__(self, prompts, **kw):
        return list(prompts)


class SyntheticTextEmbedder(nn.Module):
    """Stand-in text side of ``synthetic:*`` scorers: a prompt's embedding is N(0, 1) noise of ``projection_dim`` seeded by
    the hash of the string (as `model_util.SyntheticTextEncoder` does for the UNet's context)."""

    def __init__(self, dim: int):
        super().__init__()
        self.dim = dim

    def embed(self, prompt: str) -> torch.Tensor:
        seed = int.from_bytes(hashlib.sha256(prompt.encode()).digest()[:4], "little")
        return torch.randn(1, self.dim, generator=torch.Generator().manual_seed(8642 + seed))

    def forward(self, prompts, **kw):
        return torch.cat([self.embed(p) for p in prompts])


class ClipScorer:
    """CLIP score of pictures against prompts: ``score(img_u8, prompts)`` -> fp32 [B][len(prompts)] cosines between
    ``vision.encode_images(img_u8)`` and the text embeddings (``logits=True``: times ``exp(logit_scale)``, transformers'
    ``logits_per_image``).  ``text_encoder``: the native `clip.CLIPTextModelWithProjection`, transformers' one, or the
    synthetic stand-in; ``tokenizer``: transformers' ``CLIPTokenizer`` (or the stand-in's)."""

    def __init__(self, vision: CLIPVisionModelWithProjection, text_encoder, tokenizer, logit_scale: float = math.log(1 / 0.07)):
        self.vision, self.text_encoder, self.tokenizer, self.logit_scale = vision, text_encoder, tokenizer, float(logit_scale)

    @property
    def device(self):
        return self.vision.device

    def to(self, device) -> "ClipScorer":
        self.vision.to(device)
        if isinstance(self.text_encoder, nn.Module):
            self.text_encoder.to(device)
        return self

    def release(self) -> None:
        self.vision.release()
        if hasattr(self.text_encoder, "release"):
            self.text_encoder.release()

    @torch.no_grad()
    def encode_text(self, prompts: Sequence[str]) -> torch.Tensor:
        """``text_embeds`` [len(prompts)][projection_dim] of the scorer's text side."""
        prompts = list(prompts)
        if isinstance(self.text_encoder, SyntheticTextEmbedder):
            return self.text_encoder(prompts)
        from . import train_util
        ids = train_util.text_tokenize(self.tokenizer, prompts)
        out = self.text_encoder(ids.to(self.text_encoder.device))
        return out.text_embeds

    @torch.no_grad()
    def score(self, img_u8, prompts: Optional[Sequence[str]] = None, *, text_embeds: Optional[torch.Tensor] = None,
              logits: bool = False) -> torch.Tensor:
        if (prompts is None) == (text_embeds is None):
            raise ValueError("ClipScorer.score: give either prompts or text_embeds")
        dev = self.device
        te = self.encode_text(prompts) if text_embeds is None else torch.as_tensor(text_embeds)
        image_embeds = self.vision.encode_images(img_u8)
        return self.cosines(image_embeds, te.to(dev), logits=logits)

    def cosines(self, image_embeds: torch.Tensor, text_embeds: torch.Tensor, logits: bool = False) -> torch.Tensor:
        """fp32 [B][T] from embeddings [B][D] and [T][D] (rounded to bf16, the kernels' operand type)."""
        x, y = image_embeds.to(self.device, bf16).contiguous(), text_embeds.to(self.device, bf16).contiguous()
        if x.ndim != 2 or y.ndim != 2 or x.shape[1] != y.shape[1]:
            raise ValueError(f"ClipScorer: embeddings of shapes {tuple(x.shape)} and {tuple(y.shape)} cannot be compared")
        out = torch.zeros(x.shape[0], y.shape[0], dtype=torch.float32, device=self.device)
        ops.cosine_scores(x, x.stride(0), y, y.stride(0), out, out.stride(0), x.shape[0], y.shape[0], x.shape[1],
                          math.exp(self.logit_scale) if logits else 1.0).run()
        return out
