"""The VAE decoder (leco_amd/vae.py): the whole decoder against a plain PyTorch restatement of diffusers 0.20's `Decoder`
written here, the loaders (diffusers folder, old attention spelling, single-file LDM layout) and the sampling scripts'
`--image` path.  Kernel-level checks are in tests/test_vae_kernels.py."""
import importlib.util
import json
import os
import struct

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from leco_amd import model_util
from leco_amd import vae as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bf = torch.bfloat16


# ---- the reference: diffusers 0.20 AutoencoderKL.decode (Decoder, UNetMidBlock2D, UpDecoderBlock2D), functional -----------------
def decoder_ref(sd, cfg, latents, dtype=torch.float32):
    """decode(latents / scaling_factor) from a diffusers-named state dict `sd`, computed in `dtype` on latents' device."""
    dev = latents.device
    P = {k: v.to(dev, dtype) for k, v in sd.items()}
    G = cfg.norm_num_groups

    def gn(x, n):
        return F.group_norm(x, G, P[n + ".weight"], P[n + ".bias"], 1e-6)

    def conv(x, n, pad):
        return F.conv2d(x, P[n + ".weight"], P[n + ".bias"], padding=pad)

    def resnet(x, n):
        h = conv(F.silu(gn(x, n + ".norm1")), n + ".conv1", 1)
        h = conv(F.silu(gn(h, n + ".norm2")), n + ".conv2", 1)
        if n + ".conv_shortcut.weight" in P:
            x = conv(x, n + ".conv_shortcut", 0)
        return x + h

    def attn(x, n):
        B, Cc, H, W = x.shape
        t = gn(x, n + ".group_norm").reshape(B, Cc, H * W).transpose(1, 2)
        q, k, v = (F.linear(t, P[f"{n}.to_{c}.weight"], P[f"{n}.to_{c}.bias"]) for c in "qkv")
        p = torch.softmax(q @ k.transpose(1, 2) * Cc ** -0.5, -1)
        o = F.linear(p @ v, P[n + ".to_out.0.weight"], P[n + ".to_out.0.bias"])
        return x + o.transpose(1, 2).reshape(B, Cc, H, W)

    x = (latents.to(dtype) / cfg.scaling_factor)
    x = conv(conv(x, "post_quant_conv", 0), "decoder.conv_in", 1)
    x = resnet(x, "decoder.mid_block.resnets.0")
    x = attn(x, "decoder.mid_block.attentions.0")
    x = resnet(x, "decoder.mid_block.resnets.1")
    L = len(cfg.block_out_channels)
    for i in range(L):
        for j in range(cfg.layers_per_block + 1):
            x = resnet(x, f"decoder.up_blocks.{i}.resnets.{j}")
        if i != L - 1:
            x = conv(F.interpolate(x, scale_factor=2.0, mode="nearest"), f"decoder.up_blocks.{i}.upsamplers.0.conv", 1)
    return conv(F.silu(gn(x, "decoder.conv_norm_out")), "decoder.conv_out", 1).float()


def _bf16_weights(vae):
    """The decoder holds bf16-representable weights, so the fp32 reference and the bf16 paths see the same model."""
    with torch.no_grad():
        for p in vae.parameters():
            p.copy_(p.to(bf).float())
    return vae


def _check_against_ref(vae, lat, dev, label):
    """The project's calibrated bar: rel_hip <= 1.25 x rel_torch_bf16, both relative L2 against the
    fp32 restatement; rel_torch_bf16 is the same restatement run in bf16."""
    sd = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    ref_dev = dev if dev.type == "cuda" else torch.device("cpu")
    with torch.no_grad():
        ref = decoder_ref(sd, vae.cfg, lat.to(ref_dev)).cpu()
        ref_bf = decoder_ref(sd, vae.cfg, lat.to(ref_dev), bf).cpu()
    got = vae.decode(lat.to(dev)).sample.cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.isfinite(got).all()
    rel_hip, rel_bf = rel_err(got, ref), rel_err(ref_bf, ref)
    print(f"{label}: rel_hip {rel_hip:.4e}  rel_torch_bf16 {rel_bf:.4e}  ratio {rel_hip / rel_bf:.3f}")
    assert rel_hip <= 1.25 * rel_bf, (rel_hip, rel_bf)
    return got


def test_decoder_tiny_matches_reference(dev):
    """Latents (2,4,8,8) -> (2,3,64,64) on the tiny synthetic decoder."""
    vae = _bf16_weights(model_util.load_vae("synthetic:tiny")).to(dev)
    lat = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(70)) * 0.18215 * 1.5
    got = _check_against_ref(vae, lat, dev, "tiny decoder")
    assert got.shape == (2, 3, 64, 64)
    # the 8-bit image is the quantised sample of the same plan
    img = vae.decode_to_uint8(lat.to(dev)).cpu()
    assert img.shape == (2, 64, 64, 3) and img.dtype == torch.uint8
    q = torch.floor((got / 2 + 0.5).clamp(0, 1) * 255 + 0.5).permute(0, 2, 3, 1)
    assert (img.float() - q).abs().max().item() <= 1
    # a second call at another (h, w) builds its own plan; the first plan still gives the first answer
    lat2 = torch.randn(1, 4, 4, 6, generator=torch.Generator().manual_seed(71)) * 0.2
    got2 = vae.decode(lat2.to(dev)).sample.cpu()
    assert got2.shape == (1, 3, 32, 48) and torch.isfinite(got2).all()
    sd = {k: v.detach().cpu() for k, v in vae.state_dict().items()}
    ref2 = decoder_ref(sd, vae.cfg, lat2)
    assert rel_err(got2, ref2) <= 1.25 * rel_err(decoder_ref(sd, vae.cfg, lat2, bf), ref2)
    assert torch.equal(vae.decode(lat.to(dev)).sample.cpu(), got)
    vae.release()


@pytest.mark.gpu
def test_decoder_graph_replay_equals_eager():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conftest import _bind_hip
    _bind_hip()
    dev = torch.device("cuda:0")
    vae = _bf16_weights(model_util.load_vae("synthetic:tiny")).to(dev)
    lat = (torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(72)) * 0.25).to(dev)
    eager = vae.decode(lat).sample.clone()
    eager_img = vae.decode_to_uint8(lat).clone()
    vae.release()
    vae.use_graphs = True
    first = vae.decode(lat).sample.clone()          # captures
    again = vae.decode(lat).sample.clone()          # replays
    assert vae.engine().plan(2, 8, 8).graph is not None
    assert torch.equal(first, eager) and torch.equal(again, eager)
    assert torch.equal(vae.decode_to_uint8(lat), eager_img)
    vae.release()


@pytest.mark.gpu
def test_decoder_real_widths_matches_reference():
    """synthetic:sd15 decoder, latents (1,4,16,16) -> 128^2: the smallest size that reaches the three-launch GroupNorm
    (hw = 16384 at C = 128), the real channel counts in every conv tile, and d = 512."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conftest import _bind_hip
    _bind_hip()
    dev = torch.device("cuda:0")
    vae = _bf16_weights(model_util.load_vae("synthetic:sd15")).to(dev)
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(73)) * 0.18215 * 1.5
    got = _check_against_ref(vae, lat, dev, "sd15 decoder 128^2")
    assert got.shape == (1, 3, 128, 128)
    vae.release()


def test_decoder_rejects_fp32_compute_and_bad_latents():
    with pytest.raises(NotImplementedError, match="bfloat16"):
        model_util.load_vae("synthetic:tiny", precision="float32")
    vae = model_util.load_vae("synthetic:tiny")
    with pytest.raises(NotImplementedError, match="bfloat16"):
        vae.set_precision("float32")
    assert model_util.load_vae("synthetic:sdxl").cfg.scaling_factor == 0.13025
    assert model_util.load_vae("synthetic:sd15").cfg.block_out_channels == (128, 256, 512, 512)


# ---- loaders (CPU, no kernels) -------------------------------------------------------------------------------------------------
def _write_folder(d, vae, sd):
    from safetensors.torch import save_file
    os.makedirs(d, exist_ok=True)
    c = vae.cfg
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"_class_name": "AutoencoderKL", "latent_channels": c.latent_channels, "out_channels": 3, "in_channels": 3,
                   "block_out_channels": list(c.block_out_channels), "layers_per_block": c.layers_per_block,
                   "norm_num_groups": c.norm_num_groups, "scaling_factor": c.scaling_factor, "sample_size": 64}, f)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(d, "diffusion_pytorch_model.safetensors"))


def _same(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def _to_ldm(sd, levels):
    """diffusers decoder names -> LDM `first_stage_model.*` names (conv-shaped attention weights, reversed `up` indices)."""
    import re
    attn = {"group_norm": "norm", "to_q": "q", "to_k": "k", "to_v": "v", "to_out.0": "proj_out"}
    out = {}
    for k, v in sd.items():
        m = re.match(r"decoder\.mid_block\.resnets\.(\d)\.(.+)", k)
        m2 = re.match(r"decoder\.mid_block\.attentions\.0\.(group_norm|to_q|to_k|to_v|to_out\.0)\.(weight|bias)", k)
        m3 = re.match(r"decoder\.up_blocks\.(\d+)\.resnets\.(\d+)\.(.+)", k)
        m4 = re.match(r"decoder\.up_blocks\.(\d+)\.upsamplers\.0\.conv\.(.+)", k)
        if m:
            nk = f"decoder.mid.block_{int(m.group(1)) + 1}.{m.group(2)}"
        elif m2:
            nk = f"decoder.mid.attn_1.{attn[m2.group(1)]}.{m2.group(2)}"
            if m2.group(1) != "group_norm" and m2.group(2) == "weight":
                v = v.reshape(*v.shape, 1, 1)
        elif m3:
            nk = f"decoder.up.{levels - 1 - int(m3.group(1))}.block.{m3.group(2)}.{m3.group(3)}"
        elif m4:
            nk = f"decoder.up.{levels - 1 - int(m4.group(1))}.upsample.conv.{m4.group(2)}"
        elif k.startswith("decoder.conv_norm_out."):
            nk = k.replace("decoder.conv_norm_out.", "decoder.norm_out.")
        else:
            nk = k
        out["first_stage_model." + nk.replace(".conv_shortcut.", ".nin_shortcut.")] = v
    return out


def test_load_vae_diffusers_folder_both_attention_spellings(tmp_path):
    vae = model_util.load_vae("synthetic:tiny")
    sd = vae.state_dict()
    root = tmp_path / "pipe"
    _write_folder(str(root / "vae"), vae, sd)
    _same(model_util.load_vae(str(root)), vae)              # the pipeline root ...
    back = model_util.load_vae(str(root / "vae"))           # ... or the vae folder itself
    _same(back, vae)
    assert back.cfg == vae.cfg
    old = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}
    sd_old = {}
    for k, v in sd.items():
        for new, o in old.items():
            k = k.replace(f"attentions.0.{new}.", f"attentions.0.{o}.")
        sd_old[k] = v
    assert any(".query." in k for k in sd_old)
    sd_old["encoder.conv_in.weight"] = torch.zeros(8, 3, 3, 3)         # encoder / quant_conv keys are ignored
    sd_old["quant_conv.weight"] = torch.zeros(8, 8, 1, 1)
    _write_folder(str(tmp_path / "old"), vae, sd_old)
    _same(model_util.load_vae(str(tmp_path / "old")), vae)
    # a missing decoder key is an error naming it
    sd_short = {k: v for k, v in sd.items() if k != "decoder.mid_block.resnets.1.conv2.bias"}
    _write_folder(str(tmp_path / "short"), vae, sd_short)
    with pytest.raises(KeyError, match=r"decoder\.mid_block\.resnets\.1\.conv2\.bias"):
        model_util.load_vae(str(tmp_path / "short"))
    sd_extra = dict(sd)
    sd_extra["decoder.up_blocks.9.resnets.0.conv1.weight"] = torch.zeros(1)
    _write_folder(str(tmp_path / "extra"), vae, sd_extra)
    with pytest.raises(KeyError, match=r"decoder\.up_blocks\.9\.resnets\.0\.conv1\.weight"):
        model_util.load_vae(str(tmp_path / "extra"))


def test_load_vae_single_file_ldm_layout(tmp_path):
    """The key list (names and shapes only) is tests/golden/ldm_vae_decoder_keys.json: the LDM decoder layout of the tiny
    synthetic decoder as this repository understands it -- pinned to nothing outside this repository."""
    from safetensors.torch import save_file
    vae = model_util.load_vae("synthetic:tiny")
    ldm = _to_ldm(vae.state_dict(), len(vae.cfg.block_out_channels))
    with open(os.path.join(ROOT, "tests", "golden", "ldm_vae_decoder_keys.json")) as f:
        golden = json.load(f)
    assert {k: list(v.shape) for k, v in ldm.items()} == golden
    assert golden["first_stage_model.decoder.mid.attn_1.q.weight"] == [128, 128, 1, 1]
    assert "first_stage_model.decoder.up.1.block.0.nin_shortcut.weight" in golden      # 128 -> 64 is diffusers' up_blocks.2
    full = dict(ldm)
    full["first_stage_model.encoder.conv_in.weight"] = torch.zeros(8, 3, 3, 3)
    full["first_stage_model.quant_conv.weight"] = torch.zeros(8, 8, 1, 1)
    full["model.diffusion_model.out.2.bias"] = torch.zeros(4)
    path = str(tmp_path / "model.safetensors")
    save_file({k: v.contiguous() for k, v in full.items()}, path)
    back = model_util.load_vae(path)
    _same(back, vae)
    assert back.cfg.block_out_channels == vae.cfg.block_out_channels and back.cfg.layers_per_block == 1
    short = {k: v.contiguous() for k, v in full.items() if k != "first_stage_model.decoder.norm_out.weight"}
    save_file(short, str(tmp_path / "short.safetensors"))
    with pytest.raises(KeyError, match=r"decoder\.conv_norm_out\.weight"):
        model_util.load_vae(str(tmp_path / "short.safetensors"))
    extra = {k: v.contiguous() for k, v in full.items()}
    extra["first_stage_model.decoder.mid.attn_2.q.weight"] = torch.zeros(1)
    save_file(extra, str(tmp_path / "extra.safetensors"))
    with pytest.raises(KeyError, match=r"decoder\.mid\.attn_2\.q\.weight"):
        model_util.load_vae(str(tmp_path / "extra.safetensors"))


# ---- PNG + scripts -------------------------------------------------------------------------------------------------------------
def _png_header(path):
    with open(path, "rb") as f:
        b = f.read(33)
    assert b[:8] == b"\x89PNG\r\n\x1a\n" and b[12:16] == b"IHDR"
    w, h, depth, colour = struct.unpack(">IIBB", b[16:26])
    return w, h, depth, colour


def test_save_png_own_writer_round_trips(tmp_path):
    img = torch.randint(0, 256, (5, 7, 3), generator=torch.Generator().manual_seed(74), dtype=torch.uint8)
    p = str(tmp_path / "a.png")
    with open(p, "wb") as f:
        f.write(V._png_bytes(img.numpy()))
    assert _png_header(p) == (7, 5, 8, 2)
    import zlib
    raw = open(p, "rb").read()
    i = raw.index(b"IDAT")
    n = struct.unpack(">I", raw[i - 4:i])[0]
    assert zlib.crc32(raw[i:i + 4 + n]) & 0xffffffff == struct.unpack(">I", raw[i + 4 + n:i + 8 + n])[0]
    rows = zlib.decompress(raw[i + 4:i + 4 + n])
    got = torch.frombuffer(bytearray(rows), dtype=torch.uint8).reshape(5, 1 + 7 * 3)
    assert (got[:, 0] == 0).all() and torch.equal(got[:, 1:].reshape(5, 7, 3), img)
    V.save_png(img, str(tmp_path / "b.png"))
    assert _png_header(str(tmp_path / "b.png")) == (7, 5, 8, 2)
    with pytest.raises(ValueError):
        V.save_png(torch.zeros(3, 5, 7, dtype=torch.uint8), str(tmp_path / "c.png"))


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("script,model", [("infer_xl", "synthetic:tiny_xl"), ("infer", "synthetic:tiny")])
def test_infer_scripts_write_a_png(dev, tmp_path, script, model):
    mod = _script(script)
    png = str(tmp_path / "out.png")
    base = ["--model", model, "--height", "128", "--width", "128", "--steps", "3", "--no_graphs", "--device", str(dev),
            "--out", str(tmp_path / "latents.safetensors")]
    lat_img = mod.main(base + ["--image", png])
    assert _png_header(png) == (128, 128, 8, 2)             # 128 x 128, 8-bit, colour type 2 = RGB
    lat = mod.main(base)
    assert torch.equal(lat_img.cpu(), lat.cpu())
