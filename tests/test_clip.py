"""The native CLIP text encoder (leco_amd/clip.py) against a plain-torch fp32 restatement of the CLIP text transformer
written here (pinned to `transformers` in one CPU test), and the opt-in loaders / CLI flag around it.

Bar for the native path, the project's calibrated one (tests/test_vae.py): rel_native <= 1.25 x rel_torch_bf16, both
relative L2 against the fp32 restatement; rel_torch_bf16 is the restatement run in bf16 in the same test."""
import importlib.util
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, rel_err
from leco_amd import clip as CL
from leco_amd import model_util, train_util

bf = torch.bfloat16
OUTPUTS = ("last_hidden_state", "pooler_output", "text_embeds", "hidden_states[-2]")


# ---- the restatement ------------------------------------------------------------------------------------------------
def clip_ref(sd, cfg, ids, dtype=torch.float32):
    """transformers' CLIPTextModel(WithProjection) forward as plain torch ops on a state dict with the HF names.  Returns
    a dict: last_hidden_state, pooler_output, text_embeds (None without `text_projection.weight`), hidden_states."""
    w = {k: v.to(ids.device, dtype) for k, v in sd.items()}
    B, S = ids.shape
    H, pre = cfg.num_attention_heads, "text_model."
    x = w[pre + "embeddings.token_embedding.weight"][ids] + w[pre + "embeddings.position_embedding.weight"][:S]
    mask = torch.full((S, S), float("-inf"), device=ids.device).triu(1)
    act = (lambda z: z * torch.sigmoid(1.702 * z)) if cfg.hidden_act == "quick_gelu" else F.gelu
    ln = lambda t, n: F.layer_norm(t, t.shape[-1:], w[n + ".weight"], w[n + ".bias"], cfg.layer_norm_eps)      # noqa: E731
    lin = lambda t, n: F.linear(t, w[n + ".weight"], w[n + ".bias"])                                           # noqa: E731
    hidden = [x]
    for i in range(cfg.num_hidden_layers):
        L = f"{pre}encoder.layers.{i}."
        n = ln(x, L + "layer_norm1")
        q, k, v = (lin(n, L + f"self_attn.{p}_proj").view(B, S, H, -1).transpose(1, 2) for p in "qkv")
        s = q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5 + mask.to(dtype)
        p = torch.softmax(s, -1, dtype=torch.float32).to(dtype)         # (HF's eager attention: fp32 softmax, cast back)
        x = x + lin((p @ v).transpose(1, 2).reshape(B, S, -1), L + "self_attn.out_proj")
        x = x + lin(act(lin(ln(x, L + "layer_norm2"), L + "mlp.fc1")), L + "mlp.fc2")
        hidden.append(x)
    last = ln(x, pre + "final_layer_norm")
    pos = ids.argmax(-1) if cfg.eos_token_id == 2 else (ids == cfg.eos_token_id).int().argmax(-1)
    pooled = last[torch.arange(B, device=ids.device), pos]
    te = F.linear(pooled, w["text_projection.weight"]) if "text_projection.weight" in w else None
    return {"last_hidden_state": last, "pooler_output": pooled, "text_embeds": te, "hidden_states": hidden}


def _pick(out, name):
    if name == "hidden_states[-2]":
        return out["hidden_states"][-2] if isinstance(out, dict) else out.hidden_states[-2]
    return out[name] if isinstance(out, dict) else getattr(out, name)


def _model(cfg, projection, seed=5):
    m = (CL.CLIPTextModelWithProjection if projection else CL.CLIPTextModel)(cfg)
    CL.init_synthetic_clip_(m, seed)
    with torch.no_grad():           # bf16-representable weights: the fp32 reference and the bf16 paths see the same model
        for p in m.parameters():
            p.copy_(p.to(bf).float())
    return m


def _ids(cfg, B, pad):
    """BOS first, EOS at position 5 (then padding) or at position 76 (a full prompt); the words avoid the special ids."""
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(3, cfg.vocab_size - 2, (B, 77), generator=g)
    ids[:, 0] = cfg.vocab_size - 2
    for b in range(B):
        e = 76 if b % 2 else 5
        ids[b, e] = cfg.vocab_size - 1
        ids[b, e + 1:] = pad
    return ids


def tiny_cfg(act, projection_dim=128, eos=None, layers=3):
    return CL.CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=layers,
                             num_attention_heads=2, hidden_act=act, projection_dim=projection_dim,
                             eos_token_id=999 if eos is None else eos, bos_token_id=998)


def _check(model, ids, dev, label, ref_dev=None):
    """All four outputs of the native model against the fp32 restatement, under the bar of the module docstring."""
    cfg = model.cfg
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    ref_dev = ref_dev or torch.device("cpu")
    with torch.no_grad():
        ref = clip_ref(sd, cfg, ids.to(ref_dev))
        ref_bf = clip_ref(sd, cfg, ids.to(ref_dev), bf)
    model = model.to(dev, bf)
    got = model(ids.to(dev), output_hidden_states=True)
    assert len(got.hidden_states) == cfg.num_hidden_layers + 1
    assert got[0] is (got.text_embeds if ref["text_embeds"] is not None else got.last_hidden_state)
    for name in OUTPUTS:
        r = _pick(ref, name)
        if r is None:
            assert got.text_embeds is None
            continue
        g, rb = _pick(got, name), _pick(ref_bf, name)
        assert g.shape == r.shape and g.dtype == bf and g.device.type == dev.type and torch.isfinite(g.float()).all()
        rel_native, rel_bf16 = rel_err(g.cpu(), r.cpu()), rel_err(rb.cpu(), r.cpu())
        print(f"{label} {name}: rel_native {rel_native:.4e}  rel_torch_bf16 {rel_bf16:.4e}  ratio {rel_native / rel_bf16:.3f}")
        assert rel_native <= 1.25 * rel_bf16, (name, rel_native, rel_bf16)
    return got


# ---- the restatement is transformers' model --------------------------------------------------------------------------
@pytest.mark.parametrize("act,projection,eos", [("quick_gelu", False, 2), ("gelu", True, None)])
def test_restatement_equals_transformers(act, projection, eos):
    tr = pytest.importorskip("transformers")
    cfg = tiny_cfg(act, 64 if projection else 128, eos)
    sd = {k: v.detach().clone() for k, v in _model(cfg, projection).state_dict().items()}
    hcfg = tr.CLIPTextConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                             num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                             max_position_embeddings=77, hidden_act=act, projection_dim=cfg.projection_dim,
                             eos_token_id=cfg.eos_token_id, bos_token_id=cfg.bos_token_id)
    hf = (tr.CLIPTextModelWithProjection if projection else tr.CLIPTextModel)(hcfg).eval()
    want = hf.state_dict()
    if not any(k.startswith("text_model.") for k in want):      # newer transformers dropped the prefix
        sd_hf = {(k if k.startswith("text_projection.") else k[len("text_model."):]): v for k, v in sd.items()}
    else:
        sd_hf = sd
    missing, unexpected = hf.load_state_dict(sd_hf, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    ids = _ids(cfg, 3, 0 if projection else 999)
    with torch.no_grad():
        h = hf(ids, output_hidden_states=True)
        r = clip_ref(sd, cfg, ids)
    names = [n for n in OUTPUTS if n != "text_embeds" or projection]
    for name in names:
        a = h.hidden_states[-2] if name == "hidden_states[-2]" else getattr(h, name, None)
        if a is None:           # CLIPTextModelWithProjection has no pooler_output: the row text_projection consumes
            continue
        assert rel_err(_pick(r, name), a) <= 1e-5, name
    assert len(h.hidden_states) == len(r["hidden_states"]) == cfg.num_hidden_layers + 1


# ---- the native model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("act,projection,eos", [("quick_gelu", False, 2), ("gelu", True, None)])
def test_tiny_encoder_matches_reference(dev, act, projection, eos, B):
    """hidden 128 / 2 heads / 512 / 3 layers; the quick_gelu case carries the legacy `eos_token_id == 2` (argmax pooling)."""
    cfg = tiny_cfg(act, 64 if projection else 128, eos)
    got = _check(_model(cfg, projection), _ids(cfg, B, 0 if projection else 999), dev, f"tiny {act} B={B}")
    assert got.last_hidden_state.shape == (B, 77, 128)
    assert got[0].shape == ((B, 64) if projection else (B, 77, 128))


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,projection", [
    ("CLIP-L x 12 layers", dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                                hidden_act="quick_gelu", projection_dim=768), False),
    ("bigG x 4 layers", dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=4, num_attention_heads=20,
                             hidden_act="gelu", projection_dim=1280), True)])
def test_real_width_encoder_matches_reference(name, kw, projection):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conftest import _bind_hip
    _bind_hip()
    dev = torch.device("cuda:0")
    cfg = CL.CLIPTextConfig(vocab_size=1000, eos_token_id=999, bos_token_id=998, **kw)
    _check(_model(cfg, projection), _ids(cfg, 2, 0 if projection else 999), dev, name, ref_dev=dev)


@pytest.mark.gpu
def test_graph_replay_equals_eager_and_plans_are_cached_per_batch():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conftest import _bind_hip
    _bind_hip()
    dev = torch.device("cuda:0")
    cfg = tiny_cfg("gelu", 64)
    m = _model(cfg, True).to(dev, bf)
    ids3, ids1 = _ids(cfg, 3, 0), _ids(cfg, 1, 0)
    bits = lambda o: [t.cpu().view(torch.int16) for t in (o.last_hidden_state, o.pooler_output, o.text_embeds, o.hidden_states[-2])]  # noqa: E731
    m.use_graphs = False
    eager = bits(m(ids3.to(dev), output_hidden_states=True))
    m.release()
    m.use_graphs = True
    first = bits(m(ids3.to(dev), output_hidden_states=True))          # eager once + capture + first replay
    assert m.engine().plans[(3, 77)].graph is not None
    second = bits(m(ids3.to(dev), output_hidden_states=True))         # replay
    assert all(torch.equal(a, b) for a, b in zip(eager, first)) and all(torch.equal(a, b) for a, b in zip(first, second))
    one = bits(m(ids1.to(dev), output_hidden_states=True))            # another batch size: a second plan
    assert sorted(m.engine().plans) == [(1, 77), (3, 77)]
    again = bits(m(ids3.to(dev), output_hidden_states=True))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert all(torch.equal(a, b[:1]) for a, b in zip(one, first))     # sample 0 of the batch of 3 is the batch of 1
    m.release()
    assert m._engine is None


def test_module_contract(dev):
    """`.device`, `.dtype`, `.to`, `.eval`, `.requires_grad_`, the bf16-only precision, host-side id validation."""
    cfg = tiny_cfg("quick_gelu", layers=1)
    m = _model(cfg, False)
    assert m.eval() is m and m.requires_grad_(False) is m and m.dtype == torch.float32 and m.device.type == "cpu"
    assert m.set_precision("bfloat16") is m
    with pytest.raises(NotImplementedError, match="bfloat16 only"):
        m.set_precision("float32")
    m = m.to(dev, dtype=torch.float32)
    ids = _ids(cfg, 2, 999)[:, :9]                       # a shorter sequence than max_position_embeddings
    out = m(ids.to(dev))
    assert out[0].dtype == torch.float32 and out[0].shape == (2, 9, 128) and out.hidden_states is None
    assert out.pooler_output.shape == (2, 128) and out.text_embeds is None
    assert m.to(dev, dtype=bf).dtype == bf and m(ids.to(dev))[0].dtype == bf
    bad = ids.clone()
    bad[1, 3] = cfg.vocab_size
    with pytest.raises(IndexError, match=str(cfg.vocab_size)):
        m(bad.to(dev))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        m(torch.zeros(1, 78, dtype=torch.long))
    with pytest.raises(ValueError, match="must be 64"):
        CL.CLIPTextConfig(hidden_size=320, num_attention_heads=8)
    sd = dict(m.state_dict())
    gone = "text_model.encoder.layers.0.mlp.fc2.bias"
    sd.pop(gone)
    with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
        CL.CLIPTextModel(cfg).load_state_dict(sd)
    with pytest.raises(KeyError, match="text_projection"):
        CL.CLIPTextModel(cfg).load_state_dict({**m.state_dict(), "text_projection.weight": torch.zeros(128, 128)})


# ---- interface and loaders -------------------------------------------------------------------------------------------
def _write_unet(folder, cfg):
    from safetensors.torch import save_file
    from leco_amd.unet import UNet2DConditionModel
    os.makedirs(os.path.join(folder, "unet"), exist_ok=True)
    with open(os.path.join(folder, "unet", "config.json"), "w") as f:
        json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.__dict__.items()}, f)
    unet = model_util.init_synthetic_(UNet2DConditionModel(cfg), 3)
    save_file({k: v.contiguous() for k, v in unet.state_dict().items()},
              os.path.join(folder, "unet", "diffusion_pytorch_model.safetensors"))
    return unet


def _write_tokenizer(d):
    """A synthetic BPE vocabulary transformers' CLIPTokenizer accepts (single letters, no merges)."""
    chars = list("abcdefghijklmnopqrstuvwxyz")
    vocab = {c: i for i, c in enumerate(chars)}
    vocab.update({c + "</w>": len(chars) + i for i, c in enumerate(chars)})
    vocab["<|startoftext|>"] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    os.makedirs(d, exist_ok=True)
    json.dump(vocab, open(os.path.join(d, "vocab.json"), "w"))
    open(os.path.join(d, "merges.txt"), "w").write("#version: 0.2\n")
    json.dump({"model_max_length": 77, "bos_token": "<|startoftext|>", "eos_token": "<|endoftext|>",
               "unk_token": "<|endoftext|>", "pad_token": "<|endoftext|>", "tokenizer_class": "CLIPTokenizer"},
              open(os.path.join(d, "tokenizer_config.json"), "w"))
    return len(vocab)


def _write_text_encoder(d, cfg, projection, seed):
    """text_encoder/config.json + model.safetensors in the diffusers folder layout, from a native model's weights."""
    from safetensors.torch import save_file
    os.makedirs(d, exist_ok=True)
    m = _model(cfg, projection, seed)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({**{k: getattr(cfg, k) for k in cfg.__dataclass_fields__}, "model_type": "clip_text_model",
                   "architectures": ["CLIPTextModelWithProjection" if projection else "CLIPTextModel"]}, f)
    save_file({k: v.contiguous() for k, v in m.state_dict().items()}, os.path.join(d, "model.safetensors"))
    return m


def _folder(tmp_path, layers=4, xl=False, cross=128):
    folder = str(tmp_path / "model")
    vocab = _write_tokenizer(os.path.join(folder, "tokenizer"))
    cfg = CL.CLIPTextConfig(vocab_size=vocab, hidden_size=128, intermediate_size=256, num_hidden_layers=layers,
                            num_attention_heads=2, projection_dim=128, eos_token_id=vocab - 1, bos_token_id=vocab - 2)
    te = _write_text_encoder(os.path.join(folder, "text_encoder"), cfg, False, 11)
    te2 = None
    if xl:
        _write_tokenizer(os.path.join(folder, "tokenizer_2"))
        cfg2 = CL.CLIPTextConfig(vocab_size=vocab, hidden_size=64, intermediate_size=128, num_hidden_layers=layers,
                                 num_attention_heads=1, hidden_act="gelu", projection_dim=96, eos_token_id=vocab - 1,
                                 bos_token_id=vocab - 2)
        te2 = _write_text_encoder(os.path.join(folder, "text_encoder_2"), cfg2, True, 12)
        ucfg = model_util.tiny_xl_config()
    else:
        from leco_amd.unet import UNetConfig
        ucfg = UNetConfig(**{**model_util.tiny_config().__dict__, "cross_attention_dim": cross})
    unet = _write_unet(folder, ucfg)
    return folder, te, te2, unet, ucfg


PROMPTS = ["van gogh", "", "a b c " * 60]      # incl. the empty prompt and one that is truncated at 77


def _within_bar(native, hf32, hf_bf, label):
    rel_native, rel_bf16 = rel_err(native.cpu(), hf32.cpu()), rel_err(hf_bf.cpu(), hf32.cpu())
    print(f"{label}: rel_native {rel_native:.4e}  rel_torch_bf16 {rel_bf16:.4e}  ratio {rel_native / rel_bf16:.3f}")
    assert rel_native <= 1.25 * rel_bf16, (label, rel_native, rel_bf16)


def test_encode_prompts_on_a_loaded_folder_matches_the_transformers_path(dev, tmp_path):
    """`load_models(..., native_text_encoder=True)` + `encode_prompts` with a real CLIPTokenizer, beside the default
    (transformers) loader on the same folder: same shapes and dtypes, values within the bar."""
    pytest.importorskip("transformers")
    folder, _, _, _, _ = _folder(tmp_path)
    tok, enc, _, _ = model_util.load_models(folder, "ddim", native_text_encoder=True)
    assert isinstance(enc, CL.CLIPTextModel) and not isinstance(enc, CL.CLIPTextModelWithProjection)
    htok, henc, _, _ = model_util.load_models(folder, "ddim")
    assert type(henc).__module__.startswith("transformers")
    enc = enc.to(dev, dtype=bf)
    enc.eval()
    ids = train_util.text_tokenize(tok, PROMPTS)
    assert torch.equal(ids, train_util.text_tokenize(htok, PROMPTS))
    with torch.no_grad():
        e32 = train_util.encode_prompts(htok, henc, PROMPTS)
        ebf = train_util.encode_prompts(htok, henc.to(bf), PROMPTS)
    e = train_util.encode_prompts(tok, enc, PROMPTS)
    assert e.shape == e32.shape == (3, 77, 128) and e.dtype == ebf.dtype == bf and e.device.type == dev.type
    _within_bar(e, e32, ebf, "encode_prompts")
    assert train_util.text_encode(enc, ids).shape == (3, 77, 128)


def test_encode_prompts_xl_on_a_loaded_folder_matches_the_transformers_path(dev, tmp_path):
    pytest.importorskip("transformers")
    folder, _, _, _, _ = _folder(tmp_path, xl=True)
    toks, encs, _, _ = model_util.load_models_xl(folder, "ddim", native_text_encoder=True)
    assert type(encs[0]) is CL.CLIPTextModel and type(encs[1]) is CL.CLIPTextModelWithProjection
    htoks, hencs, _, _ = model_util.load_models_xl(folder, "ddim")
    for te in encs:
        te.to(dev, dtype=bf)
    with torch.no_grad():
        e32, p32 = train_util.encode_prompts_xl(htoks, hencs, PROMPTS, 2)
        ebf, pbf = train_util.encode_prompts_xl(htoks, [h.to(bf) for h in hencs], PROMPTS, 2)
    e, p = train_util.encode_prompts_xl(toks, encs, PROMPTS, 2)
    assert e.shape == e32.shape == (6, 77, 128 + 64) and p.shape == p32.shape == (6, 96)
    assert e.dtype == ebf.dtype == bf and p.dtype == pbf.dtype == bf
    _within_bar(e, e32, ebf, "encode_prompts_xl hidden_states[-2]")
    _within_bar(p, p32, pbf, "encode_prompts_xl pooled")
    pe, pp = train_util.text_encode_xl(encs[1], train_util.text_tokenize(toks[1], PROMPTS), 1)
    assert pe.shape == (3, 77, 64) and pp.shape == (3, 96)


@pytest.mark.parametrize("v2,clip_skip", [(False, None), (False, 2), (True, None)])
def test_native_loader_keeps_the_layer_count_rule(tmp_path, v2, clip_skip):
    pytest.importorskip("transformers")
    folder, te, _, _, _ = _folder(tmp_path, layers=4)
    _, henc, _ = model_util.load_diffusers_model(folder, v2=v2, clip_skip=clip_skip)
    _, enc, _ = model_util.load_diffusers_model(folder, v2=v2, clip_skip=clip_skip, native_text_encoder=True)
    expect = 4 - (clip_skip - 1) if clip_skip is not None else (3 if v2 else 4)
    assert henc.config.num_hidden_layers == enc.cfg.num_hidden_layers == len(enc.text_model.encoder.layers) == expect
    a = te.state_dict()
    assert all(torch.equal(v, a[k]) for k, v in enc.state_dict().items())


def _ldm_checkpoint(tmp_path, layout):
    """One LDM-layout file: the UNet + the text tower as `cond_stage_model.transformer.*` (HF names) or as OpenCLIP's
    `cond_stage_model.model.*` with a fused in_proj; the tokenizer next to it."""
    from safetensors.torch import save_file
    from leco_amd import ckpt_convert as cc
    folder, te, _, unet, ucfg = _folder(tmp_path, layers=4, cross=128)
    ldm = cc.diffusers_unet_to_ldm(unet.state_dict(), ucfg)
    sd = te.state_dict()
    if layout == "transformer":
        ldm.update({"cond_stage_model.transformer." + k: v for k, v in sd.items()})
    else:
        pre, t = "cond_stage_model.model.", "text_model."
        ldm[pre + "token_embedding.weight"] = sd[t + "embeddings.token_embedding.weight"]
        ldm[pre + "positional_embedding"] = sd[t + "embeddings.position_embedding.weight"]
        ldm[pre + "ln_final.weight"], ldm[pre + "ln_final.bias"] = sd[t + "final_layer_norm.weight"], sd[t + "final_layer_norm.bias"]
        names = {"layer_norm1": "ln_1", "layer_norm2": "ln_2", "mlp.fc1": "mlp.c_fc", "mlp.fc2": "mlp.c_proj",
                 "self_attn.out_proj": "attn.out_proj"}
        for i in range(4):
            L, R = f"{t}encoder.layers.{i}.", f"{pre}transformer.resblocks.{i}."
            for wb in ("weight", "bias"):
                for a, b in names.items():
                    ldm[R + b + "." + wb] = sd[L + a + "." + wb]
                ldm[R + "attn.in_proj_" + wb] = torch.cat([sd[L + f"self_attn.{p}_proj." + wb] for p in "qkv"], 0)
    ck = os.path.join(folder, "tiny.safetensors")
    save_file({k: v.contiguous() for k, v in ldm.items()}, ck)
    return ck, te, ldm


@pytest.mark.parametrize("layout", ["transformer", "model"])
def test_native_loader_reads_single_file_checkpoints(tmp_path, monkeypatch, layout):
    pytest.importorskip("transformers")
    from safetensors.torch import save_file
    ck, te, ldm = _ldm_checkpoint(tmp_path, layout)
    import transformers
    monkeypatch.setattr(transformers.CLIPTextModel, "__init__", lambda *a, **k: pytest.fail("a transformers model was built"))
    _, enc, _, _ = model_util.load_models(ck, "ddim", native_text_encoder=True)
    expect = 3 if layout == "model" else 4                  # OpenCLIP towers: the penultimate layer
    assert type(enc) is CL.CLIPTextModel and enc.cfg.num_hidden_layers == expect
    assert enc.cfg.hidden_act == ("gelu" if layout == "model" else "quick_gelu")
    a = te.state_dict()
    assert all(torch.equal(v, a[k]) for k, v in enc.state_dict().items())
    _, enc2, _ = model_util.load_checkpoint_model(ck, clip_skip=2, native_text_encoder=True)
    assert enc2.cfg.num_hidden_layers == 3
    gone = ("cond_stage_model.transformer.text_model.encoder.layers.1.mlp.fc1.bias" if layout == "transformer" else
            "cond_stage_model.model.transformer.resblocks.1.mlp.c_fc.bias")
    save_file({k: v.contiguous() for k, v in ldm.items() if k != gone}, ck)
    with pytest.raises(KeyError, match=r"text_model\.encoder\.layers\.1\.mlp\.fc1\.bias"):
        model_util.load_models(ck, "ddim", native_text_encoder=True)


def test_flag_is_refused_for_synthetic_models_and_for_fp32_training(tmp_path):
    with pytest.raises(ValueError, match="synthetic.*stand-in"):
        model_util.load_models("synthetic:tiny", "ddim", native_text_encoder=True)
    with pytest.raises(ValueError, match="synthetic.*stand-in"):
        model_util.load_models_xl("synthetic:tiny_xl", "ddim", native_text_encoder=True)
    from leco_amd import config_util
    from leco_amd.train import train
    for precision in ("float32", "float16"):
        cfg = config_util.RootConfig(prompts_file="unused.yaml", pretrained_model={"name_or_path": "synthetic:tiny"},
                                     network={"type": "lierla", "rank": 4, "alpha": 1.0},
                                     train={"precision": precision, "iterations": 1},
                                     save={"name": "x", "path": str(tmp_path), "per_steps": 1, "precision": precision},
                                     logging={}, other={})
        with pytest.raises(NotImplementedError, match="bf16-only"):
            train(cfg, [], device=torch.device("cpu"), native_text_encoder=True)


def test_infer_script_runs_on_the_native_text_encoder(dev, tmp_path, monkeypatch):
    """examples/infer.py --model <folder> --native_text_encoder on a tiny UNet folder with cross_attention_dim 128."""
    pytest.importorskip("transformers")
    folder, _, _, _, _ = _folder(tmp_path, layers=2, cross=128)
    spec = importlib.util.spec_from_file_location("infer", os.path.join(ROOT, "examples", "infer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = []
    real = model_util.load_models

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append((k.get("native_text_encoder"), out[1]))
        return out
    monkeypatch.setattr(mod.model_util, "load_models", spy)
    lat = mod.main(["--model", folder, "--native_text_encoder", "--height", "128", "--width", "128", "--steps", "2",
                    "--no_graphs", "--device", str(dev), "--out", str(tmp_path / "latents.safetensors")])
    assert lat.shape == (1, 4, 16, 16) and torch.isfinite(lat.float()).all()
    (flag, enc), = seen
    assert flag is True and type(enc) is CL.CLIPTextModel and enc._engine is not None and (1, 77) in enc._engine.plans
