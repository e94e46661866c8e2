"""The native CLIP image tower (leco_amd/clip_vision.py) against a plain-torch fp32 restatement of the CLIP vision transformer
written here (pinned to `transformers` in one CPU test), the scorer, the loader and the `--clip_score` flag of the sampling
scripts.

Bar for the native path, the project's calibrated one (tests/test_clip.py): rel_native <= 1.25 x rel_torch_bf16, both
relative L2 against the fp32 restatement; rel_torch_bf16 is the restatement run in bf16 in the same test."""
import contextlib
import importlib.util
import io
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, rel_err
from leco_amd import clip as CL
from leco_amd import clip_vision as CV
from leco_amd import model_util

bf = torch.bfloat16
OUTPUTS = ("image_embeds", "pooler_output", "last_hidden_state")


# ---- the restatement ------------------------------------------------------------------------------------------------
def vision_ref(sd, cfg, pixel_values, dtype=torch.float32):
    """transformers' CLIPVisionModelWithProjection forward as plain torch ops on a state dict with the HF names."""
    dev = pixel_values.device
    w = {k: v.to(dev, dtype) for k, v in sd.items()}
    x = pixel_values.to(dtype)
    B, H, pre = x.shape[0], cfg.num_attention_heads, "vision_model."
    pe = F.conv2d(x, w[pre + "embeddings.patch_embedding.weight"], stride=cfg.patch_size).flatten(2).transpose(1, 2)
    x = torch.cat([w[pre + "embeddings.class_embedding"].expand(B, 1, -1), pe], 1) + w[pre + "embeddings.position_embedding.weight"]
    S = x.shape[1]
    act = (lambda z: z * torch.sigmoid(1.702 * z)) if cfg.hidden_act == "quick_gelu" else F.gelu
    ln = lambda t, n: F.layer_norm(t, t.shape[-1:], w[n + ".weight"], w[n + ".bias"], cfg.layer_norm_eps)      # noqa: E731
    lin = lambda t, n: F.linear(t, w[n + ".weight"], w[n + ".bias"])                                           # noqa: E731
    x = ln(x, pre + "pre_layrnorm")
    for i in range(cfg.num_hidden_layers):
        L = f"{pre}encoder.layers.{i}."
        n = ln(x, L + "layer_norm1")
        q, k, v = (lin(n, L + f"self_attn.{p}_proj").view(B, S, H, -1).transpose(1, 2) for p in "qkv")
        s = q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5
        p = torch.softmax(s, -1, dtype=torch.float32).to(dtype)         # (HF's eager attention: fp32 softmax, cast back)
        x = x + lin((p @ v).transpose(1, 2).reshape(B, S, -1), L + "self_attn.out_proj")
        x = x + lin(act(lin(ln(x, L + "layer_norm2"), L + "mlp.fc1")), L + "mlp.fc2")
    pooled = ln(x[:, 0], pre + "post_layernorm")
    return {"last_hidden_state": x, "pooler_output": pooled, "image_embeds": F.linear(pooled, w["visual_projection.weight"])}


def tiny_cfg(act="quick_gelu", **kw):
    """hidden 128, 2 heads of 64, 2 layers, image 56 / patch 14 (17 tokens), intermediate 256, projection 64."""
    return CV.vit_tiny_config(hidden_act=act, **kw)


def wide_head_cfg():
    """hidden 320, 4 heads of 80, 1 layer, image 28 (5 tokens)."""
    return CV.CLIPVisionConfig(hidden_size=320, intermediate_size=640, num_hidden_layers=1, num_attention_heads=4, image_size=28,
                               patch_size=14, hidden_act="gelu", projection_dim=64)


def _model(cfg, seed=5):
    m = CV.init_synthetic_clip_vision_(CV.CLIPVisionModelWithProjection(cfg), seed)
    with torch.no_grad():           # bf16-representable weights: the fp32 reference and the bf16 paths see the same model
        for p in m.parameters():
            p.copy_(p.to(bf).float())
    return m


def _pixels(cfg, B, seed=9):
    """Normalised pixels of the scale CLIPImageProcessor produces, bf16-representable."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g) * 1.2).to(bf).float()


def _get(out, name):
    return out[name] if isinstance(out, dict) else getattr(out, name)


def _within_bar(got, ref, ref_bf, label):
    rel_native, rel_bf16 = rel_err(got.cpu(), ref.cpu()), rel_err(ref_bf.cpu(), ref.cpu())
    print(f"{label}: rel_native {rel_native:.4e}  rel_torch_bf16 {rel_bf16:.4e}  ratio {rel_native / rel_bf16:.3f}")
    assert rel_native <= 1.25 * rel_bf16, (label, rel_native, rel_bf16)


def _check(model, px, dev, label, run=None, bf_dev=None):
    """Every output of the native model against the fp32 restatement, under the bar of the module docstring."""
    cfg = model.cfg
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        ref = vision_ref(sd, cfg, px)
        ref_bf = vision_ref(sd, cfg, px.to(bf_dev or "cpu"), bf)
    model = model.to(dev, bf)
    got = run(model) if run else model(px.to(dev))
    T = cfg.num_patches + 1
    assert got[0] is got.image_embeds and got.last_hidden_state.shape == (px.shape[0], T, cfg.hidden_size)
    for name in OUTPUTS:
        g = _get(got, name)
        assert g.shape == _get(ref, name).shape and g.dtype == bf and g.device.type == dev.type and torch.isfinite(g.float()).all()
        _within_bar(g, _get(ref, name), _get(ref_bf, name), f"{label} {name}")
    return got


# ---- the restatement is transformers' model --------------------------------------------------------------------------
def _hf_vision_config(tr, cfg):
    return tr.CLIPVisionConfig(hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                               num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                               image_size=cfg.image_size, patch_size=cfg.patch_size, hidden_act=cfg.hidden_act,
                               projection_dim=cfg.projection_dim, layer_norm_eps=cfg.layer_norm_eps)


def _hf_vision(tr, cfg, sd):
    hf = tr.CLIPVisionModelWithProjection(_hf_vision_config(tr, cfg)).eval()
    want = hf.state_dict()
    if not any(k.startswith("vision_model.") for k in want):
        sd = {(k if k.startswith("visual_projection.") else k[len("vision_model."):]): v for k, v in sd.items()}
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    return hf


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_restatement_equals_transformers(act):
    tr = pytest.importorskip("transformers")
    cfg = tiny_cfg(act)
    sd = {k: v.detach().clone() for k, v in _model(cfg).state_dict().items()}
    hf = _hf_vision(tr, cfg, sd)
    px = _pixels(cfg, 2)
    with torch.no_grad():
        h, r = hf(pixel_values=px), vision_ref(sd, cfg, px)
    for name in OUTPUTS:
        a = getattr(h, name, None)
        if a is None:           # (a transformers whose projection class does not return the pooled row)
            continue
        err = rel_err(r[name], a)
        print(f"restatement {act} {name}: rel {err:.3e}")
        assert err <= 1e-5, name
    assert h.image_embeds is not None and h.last_hidden_state is not None


# ---- the native model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_tiny_tower_matches_reference(dev, act, B):
    cfg = tiny_cfg(act)
    got = _check(_model(cfg), _pixels(cfg, B), dev, f"tiny {act} B={B}")
    assert got.image_embeds.shape == (B, 64) and got.pooler_output.shape == (B, 128)


def test_80_wide_heads_match_reference(dev):
    cfg = wide_head_cfg()
    got = _check(_model(cfg, 6), _pixels(cfg, 2), dev, "4 heads of 80")
    assert got.last_hidden_state.shape == (2, 5, 320)


def _preprocess64(img, cfg):
    """The test's own float64 statement of CLIPImageProcessor on uint8 [B][H][W][3] (the filter of `resize_taps`)."""
    from test_clip_vision_kernels import _dense
    B, H, W, _ = img.shape
    (rt, rw, _), (ct, cw, _) = CV.preprocess_tables(H, W, cfg.image_size)
    x = img.double().permute(0, 3, 1, 2)
    v = (_dense(rt, rw, H) @ (x @ _dense(ct, cw, W).T).clamp(0, 255)).clamp(0, 255) / 255
    return (v - torch.tensor(cfg.image_mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(cfg.image_std, dtype=torch.float64).view(1, 3, 1, 1)


def _pictures(B, H, W, seed=3):
    from test_clip_vision_kernels import _picture
    return _picture(B, H, W, seed)


def test_raw_pixels_equal_forward_on_the_preprocessed_picture(dev):
    """`encode_images` on uint8 64x48 input against the restatement on the test's float64 preprocessing of it."""
    cfg = tiny_cfg()
    img = _pictures(2, 64, 48)
    px = _preprocess64(img, cfg).float()
    m = _model(cfg)
    got = _check(m, px, dev, "raw 64x48", run=lambda mod: mod.encode_images_output(img.to(dev)))
    m = m.to(dev, bf)
    assert torch.equal(m.encode_images(img).cpu(), got.image_embeds.cpu())            # a CPU tensor is accepted too
    fwd = m(px.to(dev)).image_embeds
    print(f"encode_images vs forward(preprocessed): rel {rel_err(got.image_embeds.cpu(), fwd.cpu()):.3e}")
    assert sorted(m.engine().plans) == [(2,), (2, 64, 48)]
    one = m.encode_images(img[:1, :30, :17].contiguous())                              # any H, W: another plan
    assert one.shape == (1, 64) and torch.isfinite(one.float()).all()
    with pytest.raises(ValueError, match="uint8"):
        m.encode_images(img.float())
    with pytest.raises(ValueError, match="pixel_values"):
        m(px[:, :, :28, :28])


def _graph_replay(dev):
    cfg = tiny_cfg("gelu")
    m = _model(cfg).to(dev, bf)
    px3, px1, other = _pixels(cfg, 3).to(dev), _pixels(cfg, 1).to(dev), _pixels(cfg, 3, seed=10).to(dev)
    bits = lambda o: [t.cpu().view(torch.int16) for t in (o.image_embeds, o.pooler_output, o.last_hidden_state)]      # noqa: E731
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))                                                     # noqa: E731
    m.use_graphs = False
    eager, eager_other = bits(m(px3)), bits(m(other))
    m.release()
    m.use_graphs = True
    first = bits(m(px3))              # eager once + capture + first replay
    if dev.type == "cuda":
        assert m.engine().plans[(3,)].graph is not None
    second = bits(m(other))           # replay with other pixels
    assert same(eager, first) and same(eager_other, second) and not same(first, second)
    one = bits(m(px1))                # another batch size: a second plan
    assert sorted(m.engine().plans) == [(1,), (3,)]
    assert same(first, bits(m(px3)))
    assert all(torch.equal(a, b[:1]) for a, b in zip(one, first))     # sample 0 of the batch of 3 is the batch of 1
    m.release()
    assert m._engine is None


def test_replay_equals_the_eager_launch_list(dev):
    """Graph replay (on gfx950; the emulator launches eagerly) equals the eager list bitwise; a second call with other
    pixels and a second batch size give the right result."""
    _graph_replay(dev)


def test_state_dicts_and_refusals(dev, tmp_path):
    tr = pytest.importorskip("transformers")
    cfg = tiny_cfg()
    hf = tr.CLIPVisionModelWithProjection(_hf_vision_config(tr, cfg)).eval()
    sd = dict(hf.state_dict())
    m = CV.CLIPVisionModelWithProjection(cfg)
    m.load_state_dict(sd)                                             # a transformers state dict, as is
    mine = m.state_dict()
    assert all(k.split("vision_model.")[-1] in {q.split("vision_model.")[-1] for q in mine} for k in sd if not k.endswith("position_ids"))
    assert torch.equal(mine["vision_model.pre_layrnorm.weight"], [v for k, v in sd.items() if k.endswith("pre_layrnorm.weight")][0])
    px = _pixels(cfg, 1)
    with torch.no_grad():
        want = hf(pixel_values=px).image_embeds
    got = m.to(dev, bf)(px.to(dev)).image_embeds
    assert rel_err(got.cpu(), want) < 3e-2                           # (the bar proper is test_tiny_tower_matches_reference's)
    # a full CLIPModel state dict goes through the loader's key filter
    full = {**{k: v for k, v in mine.items()}, "logit_scale": torch.tensor(2.0), "text_projection.weight": torch.zeros(64, 128),
            "text_model.final_layer_norm.weight": torch.zeros(128)}
    with pytest.raises(KeyError, match="logit_scale|text_"):
        CV.CLIPVisionModelWithProjection(cfg).load_state_dict(full)
    CV.CLIPVisionModelWithProjection(cfg).load_state_dict(CV.vision_state_dict(full))
    assert set(CV.text_state_dict(full)) == {"text_projection.weight", "text_model.final_layer_norm.weight"}
    gone = "vision_model.encoder.layers.1.mlp.fc2.bias"
    with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
        CV.CLIPVisionModelWithProjection(cfg).load_state_dict({k: v for k, v in mine.items() if k != gone})
    # refusals
    with pytest.raises(ValueError, match="104"):
        CV.CLIPVisionConfig(hidden_size=1664, intermediate_size=8192, num_hidden_layers=48, num_attention_heads=16, projection_dim=1280)
    with pytest.raises(ValueError, match="multiple of patch_size"):
        CV.CLIPVisionConfig(image_size=225)
    with pytest.raises(ValueError, match="hidden_act"):
        CV.CLIPVisionConfig(hidden_act="relu")
    with pytest.raises(ValueError, match="multiples of 64"):
        CV.CLIPVisionConfig(intermediate_size=4000)
    assert m.set_precision("bfloat16") is m
    with pytest.raises(NotImplementedError, match="bfloat16 only"):
        m.set_precision("float32")
    l, h = CV.vit_l_14_config(), CV.vit_h_14_config()
    assert (l.hidden_size, l.num_hidden_layers, l.head_dim, l.intermediate_size, l.hidden_act, l.projection_dim, l.patch_k) == \
        (1024, 24, 64, 4096, "quick_gelu", 768, 640)
    assert (h.hidden_size, h.num_hidden_layers, h.head_dim, h.intermediate_size, h.hidden_act, h.projection_dim) == \
        (1280, 32, 80, 5120, "gelu", 1024)
    p = tmp_path / "config.json"
    p.write_text(json.dumps({"projection_dim": 512, "vision_config": {"hidden_size": 128, "num_attention_heads": 2,
                                                                     "intermediate_size": 256, "num_hidden_layers": 1, "foo": 1}}))
    c = CV.CLIPVisionConfig.from_json(str(p))
    assert (c.hidden_size, c.projection_dim, c.image_size) == (128, 512, 224)


@pytest.mark.gpu
def test_vit_l_matches_reference():
    """The full-size tower (`synthetic:vit_l`), B = 1, against the fp32 restatement on the CPU."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conftest import _bind_hip
    _bind_hip()
    dev = torch.device("cuda:0")
    scorer = model_util.load_clip_scorer("synthetic:vit_l")
    m = scorer.vision.float()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.to(bf).float())
    _check(m, _pixels(m.cfg, 1), dev, "ViT-L/14", bf_dev=dev)
    m.release()


# ---- the scorer and the loader -----------------------------------------------------------------------------------------------
def test_scorer_equals_the_cosine_of_its_own_embeddings(dev):
    scorer = model_util.load_clip_scorer("synthetic:vit_tiny").to(dev)
    assert isinstance(scorer.vision, CV.CLIPVisionModelWithProjection) and scorer.vision.dtype == bf
    img = _pictures(3, 40, 56)
    te = torch.randn(2, 64, generator=torch.Generator().manual_seed(4)).to(bf)
    got = scorer.score(img.to(dev), text_embeds=te)
    emb = scorer.vision.encode_images(img.to(dev))
    ref = F.normalize(emb.cpu().double(), dim=1) @ F.normalize(te.double(), dim=1).T
    assert got.shape == (3, 2) and got.dtype == torch.float32 and got.device.type == dev.type
    assert (got.cpu().double() - ref).abs().max() <= 1e-5
    lg = scorer.score(img, text_embeds=te, logits=True)
    assert (lg.cpu().double() / torch.tensor(scorer.logit_scale).exp().double() - ref).abs().max() <= 1e-5
    by_prompt = scorer.score(img, ["van gogh", "a photo"])
    again = scorer.score(img, ["a photo"])
    assert by_prompt.shape == (3, 2) and torch.equal(by_prompt[:, 1:].cpu(), again.cpu()) and (by_prompt.abs() <= 1).all()
    assert torch.equal(scorer.encode_text(["van gogh"]), scorer.encode_text(["van gogh"])) and scorer.encode_text(["x"]).shape == (1, 64)
    with pytest.raises(ValueError, match="either"):
        scorer.score(img)
    for bad in ("synthetic:vit_x", "openai/clip-vit-large-patch14", str(ROOT)):
        with pytest.raises(FileNotFoundError):
            model_util.load_clip_scorer(bad)
    scorer.release()


def _write_clip_folder(tr, folder):
    """A tiny transformers CLIPModel (bf16-representable weights) with a synthetic BPE vocabulary, saved as a folder."""
    from test_clip import _write_tokenizer
    vocab = _write_tokenizer(folder)
    vc = _hf_vision_config(tr, tiny_cfg())
    tc = tr.CLIPTextConfig(vocab_size=vocab, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                           max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=64, eos_token_id=vocab - 1,
                           bos_token_id=vocab - 2, pad_token_id=vocab - 1)
    torch.manual_seed(12)
    hf = tr.CLIPModel(tr.CLIPConfig(text_config=tc.to_dict(), vision_config=vc.to_dict(), projection_dim=64)).eval()
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if p.ndim >= 2 and "embedding" not in n:
                p.mul_(3.0)           # (the default init is tiny: keep the activations O(1) so that bf16 error is what it usually is)
            p.copy_(p.to(bf).float())
    hf.save_pretrained(folder, safe_serialization=True)
    return hf


def test_scorer_on_a_clip_model_folder_matches_transformers(dev, tmp_path):
    """Both text paths (transformers' and the native one) against transformers' logits_per_image on the CPU, the pixels
    preprocessed by the test's float64 statement."""
    tr = pytest.importorskip("transformers")
    folder = str(tmp_path / "clip")
    hf = _write_clip_folder(tr, folder)
    prompts = ["van gogh", "a photo of lemonade", "", "starry night", "a b c " * 60, "oil painting of a harbour"]
    img = _pictures(4, 64, 48, seed=8)
    tok = tr.CLIPTokenizer.from_pretrained(folder)
    ids = tok(prompts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    px = _preprocess64(img, tiny_cfg()).float()
    with torch.no_grad():
        want = hf(input_ids=ids, pixel_values=px).logits_per_image
        hfb = hf.to(bf)
        want_bf = hfb(input_ids=ids, pixel_values=px.to(bf)).logits_per_image.float()
        hf.float()
    for native in (False, True):
        scorer = model_util.load_clip_scorer(folder, native_text_encoder=native).to(dev)
        assert isinstance(scorer.text_encoder, CL.CLIPTextModelWithProjection) == native
        assert abs(scorer.logit_scale - float(hf.logit_scale)) < 1e-6
        got = scorer.score(img.to(dev), prompts, logits=True)
        assert got.shape == want.shape == (4, 6)
        _within_bar(got, want, want_bf, f"logits_per_image native_text_encoder={native}")
        cos = scorer.score(img.to(dev), prompts)
        assert (cos.abs() <= 1).all() and rel_err(cos.cpu() * float(hf.logit_scale.exp()), got.cpu()) < 1e-6
        scorer.release()
    gone = "vision_model.post_layernorm.bias"
    from safetensors.torch import load_file, save_file
    f = os.path.join(folder, "model.safetensors")
    save_file({k: v for k, v in load_file(f).items() if k != gone}, f)
    with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
        model_util.load_clip_scorer(folder)


# ---- the sampling scripts ----------------------------------------------------------------------------------------------------
def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lora_file(model, xl, dev, path):
    from leco_amd.lora import LoRANetwork
    unet = (model_util.load_models_xl if xl else model_util.load_models)(model, "ddim")[2]
    with contextlib.redirect_stdout(io.StringIO()):
        net = LoRANetwork(unet.to(dev, bf), rank=4, multiplier=1.0, alpha=1.0)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for l in net.unet_loras:
            l.lora_up.weight.copy_(torch.randn(l.lora_up.weight.shape, generator=g) * 0.3)
    net.save_weights(path, dtype=torch.float32)
    return path


def _run(mod, argv):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        mod.main(argv)
    return out.getvalue()


def _bytes(path):
    """The bytes of a PNG; of a safetensors file the bytes of its tensors and its metadata (the serialiser orders the
    metadata entries of the header differently from run to run, whatever is written)."""
    if path.endswith(".safetensors"):
        from safetensors import safe_open
        with safe_open(path, "pt") as f:
            return sorted(f.metadata().items()), {k: f.get_tensor(k).contiguous().view(torch.uint8).numpy().tobytes() for k in f.keys()}
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("script,model,sweep", [("infer", "synthetic:tiny", False), ("infer", "synthetic:tiny", True),
                                                ("infer_xl", "synthetic:tiny_xl", True)])
def test_infer_scripts_clip_score(dev, tmp_path, script, model, sweep):
    mod = _script(script)
    png, out = str(tmp_path / "x.png"), str(tmp_path / "latents.safetensors")
    base = ["--model", model, "--height", "64", "--width", "64", "--steps", "2", "--device", str(dev), "--out", out, "--image", png]
    if sweep:
        base += ["--lora", _lora_file(model, script == "infer_xl", dev, str(tmp_path / "x_last.safetensors")), "--lora_scales", "-1,0,1"]
    n = 3 if sweep else 1
    plain_text = _run(mod, base)
    plain_png, plain_lat = _bytes(png), _bytes(out)
    scores = str(tmp_path / "x.scores.json")
    assert not os.path.exists(scores) and "clip score" not in plain_text
    text = _run(mod, base + ["--clip_score", "a", "--clip_score", "b"])
    assert _bytes(png) == plain_png and _bytes(out) == plain_lat                 # scoring changes neither output
    table = json.load(open(scores))
    assert table["prompts"] == ["a", "b"] and table["clip_model"] == "synthetic:vit_tiny"
    assert table["strengths"] == ([[-1.0], [0.0], [1.0]] if sweep else [None])
    cos = torch.tensor(table["cosines"])
    assert cos.shape == (n, 2) and torch.isfinite(cos).all() and (cos.abs() <= 1).all()
    lines = [l for l in text.splitlines() if l.startswith("clip score")]
    assert len(lines) == n + 1 and all("'a'" in l and "'b'" in l for l in lines[:n])
    if sweep:
        assert [l.split(":")[0] for l in lines[:n]] == ["clip score strengths -1", "clip score strengths 0", "clip score strengths 1"]
        assert len({tuple(r) for r in table["cosines"]}) == n                      # the strengths give different pictures
    # the table is the scorer's own answer on the written pictures
    from leco_amd.vae import load_png
    sheet = load_png(png)
    panels = torch.stack([sheet[:, 64 * i:64 * (i + 1)] for i in range(n)]).contiguous()
    scorer = model_util.load_clip_scorer("synthetic:vit_tiny").to(dev)
    assert torch.equal(scorer.score(panels.to(dev), ["a", "b"]).cpu(), cos)
    scorer.release()
    # flag errors
    no_image = [a for i, a in enumerate(base) if a != "--image" and base[i - 1] != "--image"]
    for bad in (no_image + ["--clip_score", "a"], base + ["--clip_model", "synthetic:vit_tiny"]):
        with pytest.raises(SystemExit):
            with contextlib.redirect_stderr(io.StringIO()):
                mod.main(bad)
    with pytest.raises(FileNotFoundError):
        _run(mod, base + ["--clip_score", "a", "--clip_model", str(tmp_path / "nowhere")])
