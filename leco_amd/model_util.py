"""Model loading -- interface of the reference's ``model_util.py`` (``load_models`` :104-129,
``load_models_xl`` :205-227, ``create_noise_scheduler`` :230-278) without diffusers:

* a diffusers-format folder (``unet/config.json`` + ``unet/diffusion_pytorch_model.safetensors``,
  ``tokenizer/``, ``text_encoder/``) is read directly: the UNet module tree here uses the diffusers
  state-dict key names, so ``load_state_dict`` applies as is; CLIP comes from ``transformers``;
* ``synthetic:<sd15|sd21|sdxl|tiny>`` builds a seeded random-init UNet of that architecture and a
  deterministic stand-in text encoder (there are no checkpoints and no network on the build /
  benchmark boxes);
* single-file ``.ckpt`` / ``.safetensors`` checkpoints (LDM key layout) go through
  ``leco_amd/ckpt_convert.py`` (architecture detected from tensor shapes, key map derived from the block
  structure; CLIP-L / OpenCLIP-H text towers rebuilt as ``transformers`` models);
* ``native_text_encoder=True`` (opt-in) returns ``leco_amd.clip`` text encoders -- the same towers on the HIP kernels,
  bf16 only -- instead of the ``transformers`` models; the tokenizers stay ``transformers``';
* ``load_clip_scorer`` (opt-in, the CLIP score of samples) reads a local transformers ``CLIPModel`` folder or builds
  ``synthetic:vit_tiny`` / ``synthetic:vit_l`` into a `leco_amd.clip_vision.ClipScorer`.
"""
from __future__ import annotations

import hashlib
import json
import math
import os
from typing import Optional

import torch

from .scheduler import create_noise_scheduler  # noqa: F401  (re-exported, model_util.py:230)
from .unet import UNet2DConditionModel, UNetConfig, sd15_config, sd21_config, sdxl_config

TOKENIZER_V1_MODEL_NAME = "CompVis/stable-diffusion-v1-4"
TOKENIZER_V2_MODEL_NAME = "stabilityai/stable-diffusion-2-1"


def tiny_config(linear_proj: bool = False) -> UNetConfig:
    return UNetConfig(block_out_channels=(64, 128, 128, 128), layers_per_block=1, attention_head_dim=2,
                      cross_attention_dim=64, use_linear_projection=linear_proj, sample_size=16)


SYNTHETIC = {"sd15": sd15_config, "sd21": sd21_config, "sdxl": sdxl_config, "tiny": tiny_config}


def init_synthetic_(unet: torch.nn.Module, seed: int = 1234) -> torch.nn.Module:
    """Seeded PyTorch-default-style init (U(+-1/sqrt(fan_in)) for conv/linear weights, norm
    gamma=1 / beta=0); keeps activations O(1) through every block."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in unet.named_parameters():
            if p.ndim >= 2:
                bound = 1.0 / math.sqrt(p[0].numel())
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * bound)
            elif "norm" in name:
                p.fill_(1.0 if name.endswith("weight") else 0.0)
            else:
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * 0.02)
    return unet


class _PromptIds(list):
    """Stand-in for the token-id tensor: the prompt strings themselves."""

    def to(self, *a, **k):
        return self


class SyntheticTokenizer:
    model_max_length = 77

    def __call__(self, prompts, **kw):
        class _Out:
            pass
        o = _Out()
        o.input_ids = _PromptIds(prompts)
        return o


class SyntheticTextEncoder(torch.nn.Module):
    """Deterministic stand-in for CLIP: embeds a prompt string as N(0,1) noise seeded by its hash
    (``randn(1,77,C)``).  ``[0]`` of the output is the (1,77,C) embedding."""

    def __init__(self, dim: int, pooled_dim: Optional[int] = None):
        super().__init__()
        self.dim, self.pooled_dim = dim, pooled_dim
        self._p = torch.nn.Parameter(torch.zeros(1))

    @property
    def device(self):
        return self._p.device

    def embed(self, prompt: str) -> torch.Tensor:
        seed = int.from_bytes(hashlib.sha256(prompt.encode()).digest()[:4], "little")
        g = torch.Generator().manual_seed(4321 + seed)
        return torch.randn(1, 77, self.dim, generator=g)

    def forward(self, tokens, **kw):
        emb = torch.cat([self.embed(p) for p in tokens]).to(self._p.device, self._p.dtype)
        return (emb,)


class _XLOut:
    def __init__(self, pooled, hidden):
        self.pooled, self.hidden_states = pooled, [hidden, hidden, hidden]

    def __getitem__(self, i):
        return (self.pooled, self.hidden_states[-1])[i]


class SyntheticTextEncoderXL(SyntheticTextEncoder):
    """Stand-in for the two SDXL text encoders: ``hidden_states[-2]`` is (1,77,dim), ``[0]`` the pooled vector."""

    def forward(self, tokens, output_hidden_states=False, **kw):
        hid = torch.cat([self.embed(p) for p in tokens]).to(self._p.device, self._p.dtype)
        g = torch.Generator().manual_seed(991)
        proj = torch.randn(self.dim, self.pooled_dim or self.dim, generator=g) / self.dim ** 0.5
        pooled = (hid.float().mean(1).cpu() @ proj).to(self._p.device, self._p.dtype)
        return _XLOut(pooled, hid)


def tiny_xl_config() -> UNetConfig:
    return UNetConfig(block_out_channels=(64, 128, 128),
                      down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
                      up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"), layers_per_block=1,
                      transformer_layers_per_block=(1, 1, 2), attention_head_dim=(2, 2, 2), cross_attention_dim=64,
                      use_linear_projection=True, sample_size=16, addition_embed_type="text_time",
                      addition_time_embed_dim=32, projection_class_embeddings_input_dim=6 * 32 + 64)


def _load_unet_folder(path: str) -> UNet2DConditionModel:
    with open(os.path.join(path, "config.json")) as f:
        cfg = UNetConfig.from_dict(json.load(f))
    unet = UNet2DConditionModel(cfg)
    st = os.path.join(path, "diffusion_pytorch_model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file
        sd = load_file(st)
    else:
        sd = torch.load(os.path.join(path, "diffusion_pytorch_model.bin"), map_location="cpu")
    missing, unexpected = unet.load_state_dict(sd, strict=False)
    if missing:
        raise KeyError(f"UNet checkpoint {path} lacks keys, e.g. {missing[:5]}")
    return unet


NATIVE_SYNTHETIC_ERROR = ("native_text_encoder: synthetic:* models keep their hash-noise stand-in text encoders (their "
                          "cross-attention widths are not multiples of 64, the native encoder's head width)")


def _read_state_folder(d: str, stem: str = "model") -> dict:
    for name in (stem + ".safetensors", "diffusion_pytorch_model.safetensors"):
        if os.path.exists(os.path.join(d, name)):
            from safetensors.torch import load_file
            return load_file(os.path.join(d, name))
    for name in ("pytorch_model.bin", "diffusion_pytorch_model.bin"):
        if os.path.exists(os.path.join(d, name)):
            return torch.load(os.path.join(d, name), map_location="cpu")
    raise FileNotFoundError(f"{d}: no {stem}.safetensors / pytorch_model.bin")


def load_native_text_encoder(folder: str, num_hidden_layers: Optional[int] = None, projection: bool = False,
                             weight_dtype: torch.dtype = torch.bfloat16):
    """A diffusers ``text_encoder`` folder (``config.json`` + ``model.safetensors`` / ``pytorch_model.bin``) as a
    `leco_amd.clip` model; ``num_hidden_layers`` trims the tower (clip_skip / the v2 penultimate layer): the tensors of
    the dropped layers are left out, every other missing or unexpected key is a KeyError naming it.  ``weight_dtype`` is
    only the dtype the parameters are held (and the outputs returned) in: the encoder computes in bf16."""
    from . import clip as CL
    over = {} if num_hidden_layers is None else {"num_hidden_layers": num_hidden_layers}
    cfg = CL.CLIPTextConfig.from_json(os.path.join(folder, "config.json"), **over)
    sd = _native_clip_state(_read_state_folder(folder), cfg.num_hidden_layers, projection)
    model = (CL.CLIPTextModelWithProjection if projection else CL.CLIPTextModel)(cfg)
    model.load_state_dict(sd)
    return model.to(weight_dtype)


def _native_clip_state(sd: dict, layers: int, projection: bool) -> dict:
    """HF text-encoder state dict -> what the trimmed native tower holds: the ``text_model.`` prefix restored where a
    newer ``transformers`` saved without it, layers >= `layers` and (without a projection head) ``text_projection`` dropped."""
    if not any(k.startswith("text_model.") for k in sd):
        sd = {(k if k.startswith("text_projection.") else "text_model." + k): v for k, v in sd.items()}
    out = {}
    for k, v in sd.items():
        if k.startswith("text_model.encoder.layers.") and int(k.split(".")[3]) >= layers:
            continue
        if k.startswith("text_projection.") and not projection:
            continue
        out[k] = v
    return out


def load_diffusers_model(path: str, v2: bool = False, clip_skip: Optional[int] = None,
                         weight_dtype: torch.dtype = torch.float32, native_text_encoder: bool = False):
    from transformers import CLIPTokenizer
    tokenizer = CLIPTokenizer.from_pretrained(path, subfolder="tokenizer")
    full = 24 if v2 else 12             # the released checkpoints (model_util.py:43-49, 58-61) ...
    try:                                # ... or whatever the folder's own config says (reduced test models)
        with open(os.path.join(path, "text_encoder", "config.json")) as f:
            full = int(json.load(f).get("num_hidden_layers", full))
    except OSError:
        pass
    default_layers = full - 1 if v2 else full   # v2: penultimate layer (model_util.py:43-49)
    nl = full - (clip_skip - 1) if clip_skip is not None else default_layers
    if native_text_encoder:
        text_encoder = load_native_text_encoder(os.path.join(path, "text_encoder"), nl, weight_dtype=weight_dtype)
    else:
        from transformers import CLIPTextModel
        text_encoder = CLIPTextModel.from_pretrained(path, subfolder="text_encoder", num_hidden_layers=nl,
                                                     torch_dtype=weight_dtype)
    unet = _load_unet_folder(os.path.join(path, "unet")).to(weight_dtype)
    return tokenizer, text_encoder, unet


def load_unet_single_file(path: str) -> UNet2DConditionModel:
    """UNet of a single-file (LDM-layout) checkpoint; the architecture is detected from the tensor shapes."""
    from . import ckpt_convert as cc
    sd = cc.read_checkpoint(path)
    cfg = cc.detect_unet_config(sd)
    unet = UNet2DConditionModel(cfg)
    missing, unexpected = unet.load_state_dict(cc.convert_ldm_unet(sd, cfg), strict=False)
    if missing or unexpected:
        raise KeyError(f"{path}: UNet keys do not match the detected architecture "
                       f"(missing {missing[:3]}, unexpected {unexpected[:3]})")
    return unet


def _find_tokenizer_dir(ckpt_path: str) -> str:
    """CLIP vocabulary files cannot be fetched (no network): `<ckpt dir>/tokenizer/` or $LECO_TOKENIZER_DIR."""
    for d in (os.environ.get("LECO_TOKENIZER_DIR"), os.path.join(os.path.dirname(os.path.abspath(ckpt_path)), "tokenizer")):
        if d and os.path.isfile(os.path.join(d, "vocab.json")):
            return d
    raise FileNotFoundError("single-file checkpoints carry no tokenizer files: put the CLIP tokenizer (vocab.json, "
                            "merges.txt, ...) in a 'tokenizer' folder next to the checkpoint or set LECO_TOKENIZER_DIR")


def load_checkpoint_model(checkpoint_path: str, v2: bool = False, clip_skip: Optional[int] = None,
                          weight_dtype: torch.dtype = torch.float32, native_text_encoder: bool = False):
    """model_util.py:75-101 (`StableDiffusionPipeline.from_single_file`): tokenizer, text encoder and UNet of a
    `.ckpt` / `.safetensors` file in the LDM key layout; the VAE is never touched.  ``native_text_encoder``: the converted
    state dict goes straight into a `leco_amd.clip.CLIPTextModel` (no ``transformers`` model object is built)."""
    from transformers import CLIPTokenizer
    from . import ckpt_convert as cc
    tokenizer_dir = _find_tokenizer_dir(checkpoint_path)                # fail fast: nothing below can fetch it
    sd = cc.read_checkpoint(checkpoint_path)
    cfg = cc.detect_unet_config(sd)
    unet = UNet2DConditionModel(cfg)
    missing, unexpected = unet.load_state_dict(cc.convert_ldm_unet(sd, cfg), strict=False)
    if missing or unexpected:
        raise KeyError(f"{checkpoint_path}: UNet keys do not match the detected architecture "
                       f"(missing {missing[:3]}, unexpected {unexpected[:3]})")
    if any(k.startswith("cond_stage_model.model.") for k in sd):        # SD2.x: OpenCLIP ViT-H text tower
        te_sd = cc.convert_open_clip(sd)
        act, drop_last = "gelu", 1                                      # penultimate layer (model_util.py:43-49)
    elif any(k.startswith("cond_stage_model.transformer.") for k in sd):  # SD1.x: HF CLIP-L names already
        te_sd = cc.convert_ldm_clip(sd)
        act, drop_last = "quick_gelu", 0
    else:
        raise KeyError(f"{checkpoint_path}: no text encoder (cond_stage_model.*) in the checkpoint")
    # geometry from the tensors themselves (CLIP-L: 768 / 12 layers, OpenCLIP-H: 1024 / 24 layers, heads = width / 64)
    emb = te_sd["text_model.embeddings.token_embedding.weight"]
    full = 1 + max(int(k.split(".")[3]) for k in te_sd if k.startswith("text_model.encoder.layers."))
    hidden = int(emb.shape[1])
    tcfg = dict(vocab_size=int(emb.shape[0]), hidden_size=hidden, projection_dim=hidden, hidden_act=act,
                intermediate_size=int(te_sd["text_model.encoder.layers.0.mlp.fc1.weight"].shape[0]),
                num_attention_heads=max(1, hidden // 64),
                max_position_embeddings=int(te_sd["text_model.embeddings.position_embedding.weight"].shape[0]))
    nl = full - (clip_skip - 1) if clip_skip is not None else full - drop_last   # model_util.py:92-96
    if native_text_encoder:
        from . import clip as CL
        ncfg = CL.CLIPTextConfig(num_hidden_layers=nl, bos_token_id=tcfg["vocab_size"] - 2, eos_token_id=tcfg["vocab_size"] - 1,
                                 **tcfg)
        text_encoder = CL.CLIPTextModel(ncfg)
        try:
            text_encoder.load_state_dict(_native_clip_state(te_sd, nl, False))
        except KeyError as e:
            raise KeyError(f"{checkpoint_path}: {e.args[0]}") from None
        tokenizer = CLIPTokenizer.from_pretrained(tokenizer_dir)
        return tokenizer, text_encoder.to(weight_dtype), unet.to(weight_dtype)
    from transformers import CLIPTextConfig, CLIPTextModel
    # CLIP's BPE vocabulary ends with <|startoftext|>, <|endoftext|> (49406 / 49407); pooling looks for the latter
    text_encoder = CLIPTextModel(CLIPTextConfig(num_hidden_layers=nl, bos_token_id=tcfg["vocab_size"] - 2,
                                                eos_token_id=tcfg["vocab_size"] - 1, **tcfg))
    want = text_encoder.state_dict()
    if not any(k.startswith("text_model.") for k in want):             # transformers >= 5 dropped the prefix
        te_sd = {k[len("text_model."):] if k.startswith("text_model.") else k: v for k, v in te_sd.items()}
    te_sd = {k: v for k, v in te_sd.items() if k in want}               # layers beyond `nl` are dropped
    lacking = [k for k in want if k not in te_sd and not k.endswith("position_ids")]
    if lacking:
        raise KeyError(f"{checkpoint_path}: text encoder lacks {lacking[:3]}")
    text_encoder.load_state_dict(te_sd, strict=False)
    tokenizer = CLIPTokenizer.from_pretrained(tokenizer_dir)
    return tokenizer, text_encoder.to(weight_dtype), unet.to(weight_dtype)


def load_synthetic_model(kind: str, seed: int = 1234):
    cfg = SYNTHETIC[kind]()
    unet = init_synthetic_(UNet2DConditionModel(cfg), seed)
    return SyntheticTokenizer(), SyntheticTextEncoder(cfg.cross_attention_dim), unet


def _load_state_into_vae(vae, sd, what: str):
    missing, unexpected = vae.load_state_dict(sd, strict=False)
    if missing:
        raise KeyError(f"{what}: the VAE lacks {missing[0]!r}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
    if unexpected:
        raise KeyError(f"{what}: unexpected VAE key {unexpected[0]!r}"
                       + (f" (and {len(unexpected) - 1} more)" if len(unexpected) > 1 else ""))
    return vae


SYNTHETIC_VAE = {"sd15": 0.18215, "sd21": 0.18215, "sdxl": 0.13025}      # real decoder shape, scaling factor


def load_vae(path: str, precision: str = "bfloat16", scaling_factor: Optional[float] = None, encoder: bool = False):
    """The VAE (`leco_amd.vae.AutoencoderKL`: the decoder half; with ``encoder=True`` also ``encoder`` + ``quant_conv``, for
    `encode` / `encode_to_latents`) of

    * a diffusers pipeline folder (its ``vae/`` subfolder) or the ``vae`` folder itself: ``config.json`` +
      ``diffusion_pytorch_model.safetensors`` / ``.bin``; both attention spellings (``to_q`` ... / ``query`` ...);
    * a single-file LDM checkpoint (``first_stage_model.*``; without ``encoder=True`` its encoder and ``quant_conv`` are ignored);
    * ``synthetic:<sd15|sd21|sdxl>`` (the real decoder shape, seeded random weights) / ``synthetic:<tiny|tiny_xl>``.

    A missing or unexpected key of a half that is built is an error naming it.  The VAE computes in bfloat16 only.  Synthetic
    encoder weights come from a generator of their own: the decoder weights do not depend on ``encoder``."""
    from . import ckpt_convert as cc
    from . import vae as V
    if precision not in ("bfloat16", "bf16", torch.bfloat16):
        raise NotImplementedError(f"load_vae: compute precision {precision!r} is not implemented for the VAE decoder (bfloat16 only)")
    p = path
    if p.startswith("synthetic:"):
        kind = p.split(":", 1)[1]
        if kind in SYNTHETIC_VAE:
            cfg = V.VAEConfig(scaling_factor=SYNTHETIC_VAE[kind])
        elif kind in ("tiny", "tiny_xl", "tinyxl"):
            cfg = V.tiny_vae_config(0.18215 if kind == "tiny" else 0.13025)
        else:
            raise ValueError(f"{p}: unknown synthetic VAE (sd15 | sd21 | sdxl | tiny | tiny_xl)")
        return V.init_synthetic_vae_(V.AutoencoderKL(cfg, encoder=encoder))
    if os.path.isdir(p):
        d = os.path.join(p, "vae") if os.path.isfile(os.path.join(p, "vae", "config.json")) else p
        if not os.path.isfile(os.path.join(d, "config.json")):
            raise FileNotFoundError(f"{p}: no vae/config.json or config.json")
        cfg = V.VAEConfig.from_json(os.path.join(d, "config.json"))
        if scaling_factor is not None:
            cfg.scaling_factor = scaling_factor
        st = os.path.join(d, "diffusion_pytorch_model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        else:
            sd = torch.load(os.path.join(d, "diffusion_pytorch_model.bin"), map_location="cpu")
        return _load_state_into_vae(V.AutoencoderKL(cfg, encoder=encoder), cc.normalise_vae_keys(sd, encoder), d)
    if p.endswith(".ckpt") or p.endswith(".safetensors"):
        sd = cc.convert_ldm_vae(cc.read_checkpoint(p), encoder)
        return _load_state_into_vae(V.AutoencoderKL(cc.detect_vae_config(sd, scaling_factor), encoder=encoder), sd, p)
    raise FileNotFoundError(f"{p}: not a local diffusers folder, single-file checkpoint or synthetic:<sd15|sd21|sdxl|tiny|tiny_xl>")


SYNTHETIC_CLIP_SCORER = ("vit_tiny", "vit_l")


def load_clip_scorer(path: str, native_text_encoder: bool = False):
    """A `leco_amd.clip_vision.ClipScorer` (native image tower + a text side + tokenizer) from

    * a local transformers ``CLIPModel`` folder: ``config.json`` with ``vision_config`` / ``text_config``,
      ``model.safetensors`` / ``pytorch_model.bin``, the tokenizer files.  The text side is transformers'
      ``CLIPTextModelWithProjection``, or with ``native_text_encoder=True`` the native one (`leco_amd.clip`, bf16 only);
    * ``synthetic:vit_tiny`` / ``synthetic:vit_l``: seeded random weights of that shape; the text side is a hash-noise
      stand-in vector of ``projection_dim`` per prompt (as `SyntheticTextEncoder`), whatever ``native_text_encoder`` says.

    Anything else is a FileNotFoundError: nothing is fetched.  A missing or unexpected key of a tower is a KeyError naming it."""
    from . import clip as CL
    from . import clip_vision as CV
    if path.startswith("synthetic:"):
        kind = path.split(":", 1)[1]
        if kind not in SYNTHETIC_CLIP_SCORER:
            raise FileNotFoundError(f"{path}: unknown synthetic CLIP model (synthetic:vit_tiny | synthetic:vit_l)")
        cfg = CV.vit_tiny_config() if kind == "vit_tiny" else CV.vit_l_14_config()
        vision = CV.init_synthetic_clip_vision_(CV.CLIPVisionModelWithProjection(cfg)).to(torch.bfloat16)
        return CV.ClipScorer(vision, CV.SyntheticTextEmbedder(cfg.projection_dim), CV.SyntheticTokenizer())
    if not (os.path.isdir(path) and os.path.isfile(os.path.join(path, "config.json"))):
        raise FileNotFoundError(f"{path}: not a local transformers CLIPModel folder (config.json, weights, tokenizer files) and "
                                f"not synthetic:vit_tiny | synthetic:vit_l; nothing is fetched")
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    if "vision_config" not in cfg or "text_config" not in cfg:
        raise FileNotFoundError(f"{path}/config.json: no vision_config / text_config (not a CLIPModel folder)")
    from transformers import CLIPTokenizer
    tokenizer = CLIPTokenizer.from_pretrained(path)
    sd = _read_state_folder(path)
    vision = CV.CLIPVisionModelWithProjection(CV.CLIPVisionConfig.from_json(os.path.join(path, "config.json")))
    vision.load_state_dict(CV.vision_state_dict(sd))
    tc = {k: v for k, v in cfg["text_config"].items() if v is not None}
    if cfg.get("projection_dim"):
        tc["projection_dim"] = cfg["projection_dim"]
    tc.setdefault("eos_token_id", tokenizer.eos_token_id)
    tc.setdefault("bos_token_id", tokenizer.bos_token_id)
    tsd = CV.text_state_dict(sd)
    if native_text_encoder:
        text = CL.CLIPTextModelWithProjection(CL.CLIPTextConfig.from_dict(tc))
        text.load_state_dict(tsd)
        text = text.to(torch.bfloat16)
    else:
        from transformers import CLIPTextConfig, CLIPTextModelWithProjection
        known = set(CL.CLIPTextConfig.__dataclass_fields__)
        text = CLIPTextModelWithProjection(CLIPTextConfig(**{k: v for k, v in tc.items() if k in known})).eval()
        want = text.state_dict()
        if not any(k.startswith("text_model.") for k in want):              # transformers >= 5 dropped the prefix
            tsd = {k[len("text_model."):] if k.startswith("text_model.") else k: v for k, v in tsd.items()}
        lacking = [k for k in want if k not in tsd and not k.endswith("position_ids")]
        if lacking:
            raise KeyError(f"{path}: the text tower lacks {lacking[0]!r}")
        text.load_state_dict({k: v for k, v in tsd.items() if k in want}, strict=False)
        text.requires_grad_(False)
    scale = float(sd["logit_scale"]) if "logit_scale" in sd else math.log(1 / 0.07)
    return CV.ClipScorer(vision.to(torch.bfloat16), text, tokenizer, logit_scale=scale)


def load_models(pretrained_model_name_or_path: str, scheduler_name: str, v2: bool = False, v_pred: bool = False,
                weight_dtype: torch.dtype = torch.float32, native_text_encoder: bool = False):
    p = pretrained_model_name_or_path
    if p.startswith("synthetic:"):
        if native_text_encoder:
            raise ValueError(NATIVE_SYNTHETIC_ERROR)
        tokenizer, text_encoder, unet = load_synthetic_model(p.split(":", 1)[1])
    elif p.endswith(".ckpt") or p.endswith(".safetensors"):
        tokenizer, text_encoder, unet = load_checkpoint_model(p, v2=v2, weight_dtype=weight_dtype,
                                                              native_text_encoder=native_text_encoder)
    elif os.path.isdir(p):
        tokenizer, text_encoder, unet = load_diffusers_model(p, v2=v2, weight_dtype=weight_dtype,
                                                             native_text_encoder=native_text_encoder)
    else:
        raise FileNotFoundError(f"{p}: not a local diffusers folder (no network access on this system); "
                                f"use a local path or synthetic:<sd15|sd21|sdxl|tiny>")
    scheduler = create_noise_scheduler(scheduler_name, prediction_type="v_prediction" if v_pred else "epsilon")
    return tokenizer, text_encoder, unet, scheduler


def load_models_xl(pretrained_model_name_or_path: str, scheduler_name: str, weight_dtype: torch.dtype = torch.float32,
                   native_text_encoder: bool = False):
    """model_util.py:205-227: returns ([tokenizer, tokenizer_2], [text_encoder, text_encoder_2], unet, scheduler)."""
    p = pretrained_model_name_or_path
    if native_text_encoder and p.startswith("synthetic:"):
        raise ValueError(NATIVE_SYNTHETIC_ERROR)
    if p.startswith("synthetic:"):
        kind = p.split(":", 1)[1]
        cfg = tiny_xl_config() if kind in ("tiny_xl", "tinyxl") else SYNTHETIC[kind]()
        if cfg.addition_embed_type != "text_time":
            raise ValueError(f"{p} is not an SDXL-style architecture")
        unet = init_synthetic_(UNet2DConditionModel(cfg), 1234)
        pooled = cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim
        d1 = cfg.cross_attention_dim * 3 // 8
        d2 = cfg.cross_attention_dim - d1           # 768 + 1280 = 2048 for SDXL
        tokenizers = [SyntheticTokenizer(), SyntheticTokenizer()]
        text_encoders = [SyntheticTextEncoderXL(d1, pooled), SyntheticTextEncoderXL(d2, pooled)]
    elif os.path.isdir(p):
        from transformers import CLIPTextModel, CLIPTextModelWithProjection, CLIPTokenizer
        tokenizers = [CLIPTokenizer.from_pretrained(p, subfolder="tokenizer"),
                      CLIPTokenizer.from_pretrained(p, subfolder="tokenizer_2", pad_token_id=0)]
        if native_text_encoder:
            text_encoders = [load_native_text_encoder(os.path.join(p, "text_encoder"), weight_dtype=weight_dtype),
                             load_native_text_encoder(os.path.join(p, "text_encoder_2"), projection=True,
                                                      weight_dtype=weight_dtype)]
        else:
            text_encoders = [CLIPTextModel.from_pretrained(p, subfolder="text_encoder", torch_dtype=weight_dtype),
                             CLIPTextModelWithProjection.from_pretrained(p, subfolder="text_encoder_2",
                                                                         torch_dtype=weight_dtype)]
        unet = _load_unet_folder(os.path.join(p, "unet")).to(weight_dtype)
    else:
        raise FileNotFoundError(f"{p}: not a local diffusers folder; use a local path or synthetic:<sdxl|tiny_xl>")
    return tokenizers, text_encoders, unet, create_noise_scheduler(scheduler_name)
