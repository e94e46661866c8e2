"""The VAE encoder (leco_amd/vae.py, `encoder=True`): the whole encoder against a plain PyTorch restatement of diffusers
0.20's `Encoder` + `quant_conv` written here, the posterior object, `encode_to_latents`, the loaders, the PNG reader, the
schedulers' `add_noise` and the sampling scripts' `--init_image` path.  Kernel-level checks are in
tests/test_vae_encoder_kernels.py."""
import importlib.util
import json
import math
import os
import re
import struct
import zlib

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from leco_amd import model_util, scheduler
from leco_amd import vae as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bf = torch.bfloat16
TOL32 = 1e-5          # the project's bounds (tests/test_kernels.py)
TOLBF = 3e-3


# ---- the reference: diffusers 0.20 AutoencoderKL.encode (Encoder, DownEncoderBlock2D, Downsample2D(padding=0), UNetMidBlock2D) -----
def encoder_ref(sd, cfg, x, dtype=torch.float32):
    """The moments quant_conv(Encoder(x)) from a diffusers-named state dict `sd`, computed in `dtype` on x's device."""
    dev = x.device
    P = {k: v.to(dev, dtype) for k, v in sd.items()}
    G = cfg.norm_num_groups

    def gn(x, n):
        return F.group_norm(x, G, P[n + ".weight"], P[n + ".bias"], 1e-6)

    def conv(x, n, pad, stride=1):
        return F.conv2d(x, P[n + ".weight"], P[n + ".bias"], padding=pad, stride=stride)

    def resnet(x, n):
        h = conv(F.silu(gn(x, n + ".norm1")), n + ".conv1", 1)
        h = conv(F.silu(gn(h, n + ".norm2")), n + ".conv2", 1)
        if n + ".conv_shortcut.weight" in P:
            x = conv(x, n + ".conv_shortcut", 0)
        return x + h

    def attn(x, n):                                    # one head of width C
        B, Cc, H, W = x.shape
        t = gn(x, n + ".group_norm").reshape(B, Cc, H * W).transpose(1, 2)
        q, k, v = (F.linear(t, P[f"{n}.to_{c}.weight"], P[f"{n}.to_{c}.bias"]) for c in "qkv")
        p = torch.softmax(q @ k.transpose(1, 2) * Cc ** -0.5, -1)
        o = F.linear(p @ v, P[n + ".to_out.0.weight"], P[n + ".to_out.0.bias"])
        return x + o.transpose(1, 2).reshape(B, Cc, H, W)

    x = conv(x.to(dtype), "encoder.conv_in", 1)
    L = len(cfg.block_out_channels)
    for i in range(L):
        for j in range(cfg.layers_per_block):
            x = resnet(x, f"encoder.down_blocks.{i}.resnets.{j}")
        if i != L - 1:                                 # Downsample2D(padding=0): pad bottom / right, then stride 2 without padding
            x = conv(F.pad(x, (0, 1, 0, 1)), f"encoder.down_blocks.{i}.downsamplers.0.conv", 0, stride=2)
    x = resnet(x, "encoder.mid_block.resnets.0")
    x = attn(x, "encoder.mid_block.attentions.0")
    x = resnet(x, "encoder.mid_block.resnets.1")
    x = conv(F.silu(gn(x, "encoder.conv_norm_out")), "encoder.conv_out", 1)
    return conv(x, "quant_conv", 0).float()


def _bf16_weights(vae):
    with torch.no_grad():
        for p in vae.parameters():
            p.copy_(p.to(bf).float())
    return vae


def _image(B, H, W, seed):
    """A smooth-plus-noise 8-bit image and its float form in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 3, H), torch.linspace(0, 3, W), indexing="ij")
    base = torch.stack([torch.sin(yy + c) * torch.cos(xx * (c + 1)) for c in range(3)], -1)
    img = ((base[None] * 0.4 + 0.5 + 0.1 * torch.randn(B, H, W, 3, generator=g)).clamp(0, 1) * 255).round().to(torch.uint8)
    return img, (img.float() / 127.5 - 1).permute(0, 3, 1, 2).contiguous()


def _check_against_ref(vae, x, dev, label):
    """The project's calibrated bar: rel_hip <= 1.25 x rel_torch_bf16 on the moments, both relative L2 against the fp32
    restatement; rel_torch_bf16 is the same restatement run in bf16."""
    sd = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    ref_dev = dev if dev.type == "cuda" else torch.device("cpu")
    with torch.no_grad():
        ref = encoder_ref(sd, vae.cfg, x.to(ref_dev)).cpu()
        ref_bf = encoder_ref(sd, vae.cfg, x.to(ref_dev), bf).cpu()
    dist = vae.encode(x.to(dev)).latent_dist
    got = dist.parameters.cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.isfinite(got).all()
    rel_hip, rel_bf = rel_err(got, ref), rel_err(ref_bf, ref)
    print(f"{label}: rel_hip {rel_hip:.4e}  rel_torch_bf16 {rel_bf:.4e}  ratio {rel_hip / rel_bf:.3f}")
    assert rel_hip <= 1.25 * rel_bf, (rel_hip, rel_bf)
    return dist


def test_encoder_tiny_matches_reference(dev):
    """Images (2,3,64,64) -> moments (2,8,8,8), and (1,3,32,48), on the tiny synthetic encoder.
    Measured on the emulator: see DESIGN.md (VAE encoder) for the ratios."""
    vae = _bf16_weights(model_util.load_vae("synthetic:tiny", encoder=True)).to(dev)
    img, x = _image(2, 64, 64, 90)
    dist = _check_against_ref(vae, x, dev, "tiny encoder 64x64")
    mom = dist.parameters.cpu()
    assert mom.shape == (2, 8, 8, 8)
    # the posterior object
    mean, logvar = mom.chunk(2, 1)
    assert torch.equal(dist.mean.cpu(), mean) and torch.equal(dist.mode().cpu(), mean)
    assert torch.equal(dist.logvar.cpu(), logvar.clamp(-30, 20))
    assert rel_err(dist.std.cpu(), torch.exp(0.5 * logvar.clamp(-30, 20))) < TOL32
    assert rel_err(dist.var.cpu(), torch.exp(logvar.clamp(-30, 20))) < TOL32
    gdev = dev if dev.type == "cuda" else "cpu"
    s = dist.sample(generator=torch.Generator(device=gdev).manual_seed(91)).cpu()
    n = torch.randn(mean.shape, generator=torch.Generator(device=gdev).manual_seed(91), device=gdev, dtype=torch.float32).cpu()
    assert rel_err(s, mean + dist.std.cpu() * n) < TOL32
    # encode_to_latents: the 8-bit image, one plan ending in the fused epilogue
    sf = vae.cfg.scaling_factor
    lat_mode = vae.encode_to_latents(img.to(dev), sample=False).cpu()
    assert lat_mode.shape == (2, 4, 8, 8) and lat_mode.dtype == torch.float32
    e = rel_err(lat_mode, sf * mean)
    print(f"encode_to_latents(uint8, mode) vs scaling_factor * mode of encode(float): rel {e:.3e}")
    assert e < TOLBF
    lat = vae.encode_to_latents(img.to(dev), generator=torch.Generator(device=gdev).manual_seed(91)).cpu()
    mom8 = lat_mode / sf                                     # the 8-bit plan's own mean
    assert rel_err(lat, sf * (mom8 + dist.std.cpu() * n)) < TOLBF
    lat_f = vae.encode_to_latents(x.to(dev), sample=False).cpu()
    assert rel_err(lat_f, sf * mean) < TOL32                 # the float image: the same launches as `encode`
    # a second (H, W) builds its own plan; the first plan still gives the first answer
    _, x2 = _image(1, 32, 48, 92)
    d2 = _check_against_ref(vae, x2, dev, "tiny encoder 32x48")
    assert d2.parameters.shape == (1, 8, 4, 6)
    assert torch.equal(vae.encode(x.to(dev)).latent_dist.parameters.cpu(), mom)
    # the decoder's plans live in the same engine and are released together
    out = vae.decode(lat_mode.to(dev)).sample
    assert out.shape == (2, 3, 64, 64)
    assert any(k[0] == "encode" for k in vae.engine().plans) and (2, 8, 8) in vae.engine().plans
    vae.release()
    assert vae._engine is None
    with pytest.raises(ValueError, match="36 x 64"):
        vae.encode(torch.zeros(1, 3, 36, 64, device=dev))
    vae.release()


@pytest.mark.gpu
def test_encoder_graph_replay_equals_eager():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conftest import _bind_hip
    _bind_hip()
    dev = torch.device("cuda:0")
    vae = _bf16_weights(model_util.load_vae("synthetic:tiny", encoder=True)).to(dev)
    img, x = _image(2, 64, 64, 93)
    x, img = x.to(dev), img.to(dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(94)      # noqa: E731
    eager = vae.encode(x).latent_dist.parameters.clone()
    eager_lat = vae.encode_to_latents(img, generator=gen()).clone()
    vae.release()
    vae.use_graphs = True
    first = vae.encode(x).latent_dist.parameters.clone()            # captures
    again = vae.encode(x).latent_dist.parameters.clone()            # replays
    assert vae.engine().encoder_plan(2, 64, 64, False, "moments").graph is not None
    assert torch.equal(first, eager) and torch.equal(again, eager)
    assert torch.equal(vae.encode_to_latents(img, generator=gen()), eager_lat)
    assert torch.equal(vae.encode_to_latents(img, generator=gen()), eager_lat)
    vae.release()


@pytest.mark.gpu
def test_encoder_real_widths_matches_reference():
    """synthetic:sd15 encoder, one image at 128^2: the smallest size that reaches the three-launch GroupNorm (hw = 16384 at
    C = 128), the real channel counts in every conv tile, all three pad-01 downsamples, and d = 512 attention at S = 256."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conftest import _bind_hip
    _bind_hip()
    dev = torch.device("cuda:0")
    vae = _bf16_weights(model_util.load_vae("synthetic:sd15", encoder=True)).to(dev)
    _, x = _image(1, 128, 128, 95)
    dist = _check_against_ref(vae, x, dev, "sd15 encoder 128^2")
    assert dist.parameters.shape == (1, 8, 16, 16)
    vae.release()


def test_encode_needs_the_encoder_and_bf16():
    vae = model_util.load_vae("synthetic:tiny")
    with pytest.raises(RuntimeError, match="encoder=True"):
        vae.encode(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match="encoder=True"):
        vae.encode_to_latents(torch.zeros(1, 64, 64, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="bfloat16"):
        model_util.load_vae("synthetic:tiny", precision="float32", encoder=True)
    with pytest.raises(ValueError, match="latent_channels"):
        V.AutoencoderKL(V.VAEConfig(latent_channels=8), encoder=True)


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
    """diffusers names -> LDM `first_stage_model.*` names, both halves (conv-shaped attention weights, reversed `up` indices)."""
    attn = {"group_norm": "norm", "to_q": "q", "to_k": "k", "to_v": "v", "to_out.0": "proj_out"}
    out = {}
    for k, v in sd.items():
        m = re.match(r"(encoder|decoder)\.mid_block\.resnets\.(\d)\.(.+)", k)
        m2 = re.match(r"(encoder|decoder)\.mid_block\.attentions\.0\.(group_norm|to_q|to_k|to_v|to_out\.0)\.(weight|bias)", k)
        m3 = re.match(r"decoder\.up_blocks\.(\d+)\.resnets\.(\d+)\.(.+)", k)
        m4 = re.match(r"decoder\.up_blocks\.(\d+)\.upsamplers\.0\.conv\.(.+)", k)
        m5 = re.match(r"encoder\.down_blocks\.(\d+)\.resnets\.(\d+)\.(.+)", k)
        m6 = re.match(r"encoder\.down_blocks\.(\d+)\.downsamplers\.0\.conv\.(.+)", k)
        if m:
            nk = f"{m.group(1)}.mid.block_{int(m.group(2)) + 1}.{m.group(3)}"
        elif m2:
            nk = f"{m2.group(1)}.mid.attn_1.{attn[m2.group(2)]}.{m2.group(3)}"
            if m2.group(2) != "group_norm" and m2.group(3) == "weight":
                v = v.reshape(*v.shape, 1, 1)
        elif m3:
            nk = f"decoder.up.{levels - 1 - int(m3.group(1))}.block.{m3.group(2)}.{m3.group(3)}"
        elif m4:
            nk = f"decoder.up.{levels - 1 - int(m4.group(1))}.upsample.conv.{m4.group(2)}"
        elif m5:
            nk = f"encoder.down.{m5.group(1)}.block.{m5.group(2)}.{m5.group(3)}"
        elif m6:
            nk = f"encoder.down.{m6.group(1)}.downsample.conv.{m6.group(2)}"
        else:
            nk = k.replace("coder.conv_norm_out.", "coder.norm_out.")
        out["first_stage_model." + nk.replace(".conv_shortcut.", ".nin_shortcut.")] = v
    return out


def test_synthetic_decoder_weights_do_not_depend_on_the_encoder_flag():
    dec, full = model_util.load_vae("synthetic:tiny"), model_util.load_vae("synthetic:tiny", encoder=True)
    sd, sf = dec.state_dict(), full.state_dict()
    assert list(sf)[:len(sd)] == list(sd)
    for k in sd:
        assert torch.equal(sd[k], sf[k]), k
    extra = list(sf)[len(sd):]
    assert extra and all(k.startswith(("encoder.", "quant_conv.")) for k in extra)
    for want in ("encoder.conv_in.weight", "encoder.down_blocks.0.resnets.0.conv1.weight", "encoder.down_blocks.0.downsamplers.0.conv.weight",
                 "encoder.down_blocks.2.resnets.0.conv_shortcut.weight", "encoder.mid_block.attentions.0.to_out.0.bias",
                 "encoder.mid_block.resnets.1.norm2.weight", "encoder.conv_norm_out.bias", "encoder.conv_out.weight", "quant_conv.bias"):
        assert want in sf, want
    assert "encoder.down_blocks.3.downsamplers.0.conv.weight" not in sf
    assert sf["encoder.conv_out.weight"].shape == (8, 128, 3, 3) and sf["quant_conv.weight"].shape == (8, 8, 1, 1)
    assert sf["encoder.down_blocks.0.downsamplers.0.conv.weight"].abs().sum() > 0


def test_load_vae_encoder_diffusers_folder_both_attention_spellings(tmp_path):
    vae = model_util.load_vae("synthetic:tiny", encoder=True)
    sd = vae.state_dict()
    _write_folder(str(tmp_path / "pipe" / "vae"), vae, sd)
    _same(model_util.load_vae(str(tmp_path / "pipe"), encoder=True), vae)
    # without the flag: the decoder-only model of today, encoder keys ignored
    plain = model_util.load_vae(str(tmp_path / "pipe"))
    assert list(plain.state_dict()) == list(model_util.load_vae("synthetic:tiny").state_dict())
    assert plain.encoder is None
    old = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}
    sd_old = {}
    for k, v in sd.items():
        for new, o in old.items():
            k = k.replace(f"attentions.0.{new}.", f"attentions.0.{o}.")
        sd_old[k] = v
    assert "encoder.mid_block.attentions.0.query.weight" in sd_old
    _write_folder(str(tmp_path / "old"), vae, sd_old)
    _same(model_util.load_vae(str(tmp_path / "old"), encoder=True), vae)
    sd_short = {k: v for k, v in sd.items() if k != "encoder.down_blocks.1.downsamplers.0.conv.bias"}
    _write_folder(str(tmp_path / "short"), vae, sd_short)
    with pytest.raises(KeyError, match=r"encoder\.down_blocks\.1\.downsamplers\.0\.conv\.bias"):
        model_util.load_vae(str(tmp_path / "short"), encoder=True)
    model_util.load_vae(str(tmp_path / "short"))                       # ... which the decoder-only load does not miss
    sd_extra = dict(sd)
    sd_extra["encoder.down_blocks.3.downsamplers.0.conv.weight"] = torch.zeros(1)
    _write_folder(str(tmp_path / "extra"), vae, sd_extra)
    with pytest.raises(KeyError, match=r"encoder\.down_blocks\.3\.downsamplers\.0\.conv\.weight"):
        model_util.load_vae(str(tmp_path / "extra"), encoder=True)


def test_load_vae_encoder_single_file_ldm_layout(tmp_path):
    """The key list (names and shapes only) is tests/golden/ldm_vae_encoder_keys.json: the LDM encoder + quant_conv layout
    of the tiny synthetic encoder as this repository understands it -- pinned to nothing outside this repository."""
    from safetensors.torch import save_file
    vae = model_util.load_vae("synthetic:tiny", encoder=True)
    ldm = _to_ldm(vae.state_dict(), len(vae.cfg.block_out_channels))
    with open(os.path.join(ROOT, "tests", "golden", "ldm_vae_encoder_keys.json")) as f:
        golden = json.load(f)
    enc = {k: list(v.shape) for k, v in ldm.items() if k.startswith(("first_stage_model.encoder.", "first_stage_model.quant_conv."))}
    assert enc == golden
    assert golden["first_stage_model.encoder.mid.attn_1.q.weight"] == [128, 128, 1, 1]
    assert golden["first_stage_model.encoder.down.2.block.0.nin_shortcut.weight"] == [128, 64, 1, 1]
    assert "first_stage_model.encoder.down.2.downsample.conv.weight" in golden
    assert "first_stage_model.encoder.down.3.downsample.conv.weight" not in golden
    full = dict(ldm)
    full["model.diffusion_model.out.2.bias"] = torch.zeros(4)
    path = str(tmp_path / "model.safetensors")
    save_file({k: v.contiguous() for k, v in full.items()}, path)
    _same(model_util.load_vae(path, encoder=True), vae)
    assert list(model_util.load_vae(path).state_dict()) == list(model_util.load_vae("synthetic:tiny").state_dict())
    short = {k: v.contiguous() for k, v in full.items() if k != "first_stage_model.encoder.norm_out.weight"}
    save_file(short, str(tmp_path / "short.safetensors"))
    with pytest.raises(KeyError, match=r"encoder\.conv_norm_out\.weight"):
        model_util.load_vae(str(tmp_path / "short.safetensors"), encoder=True)
    extra = {k: v.contiguous() for k, v in full.items()}
    extra["first_stage_model.encoder.mid.attn_2.q.weight"] = torch.zeros(1)
    save_file(extra, str(tmp_path / "extra.safetensors"))
    with pytest.raises(KeyError, match=r"encoder\.mid\.attn_2\.q\.weight"):
        model_util.load_vae(str(tmp_path / "extra.safetensors"), encoder=True)


# ---- PNG reader ----------------------------------------------------------------------------------------------------------------
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def _png(path, w, h, colour, lines, depth=8, interlace=0):
    """`lines`: per scanline (filter type, filtered bytes)."""
    raw = b"".join(bytes([ft]) + bytes(b) for ft, b in lines)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace))
                + _chunk(b"tEXt", b"Comment\x00x") + _chunk(b"IDAT", zlib.compress(raw)[:7]) + _chunk(b"IDAT", zlib.compress(raw)[7:])
                + _chunk(b"IEND", b""))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def _filter(ft, cur, prev, bpp):
    """PNG filter `ft` of scanline `cur` (lists of ints) given the previous unfiltered line."""
    out = []
    for i, x in enumerate(cur):
        a = cur[i - bpp] if i >= bpp else 0
        b = prev[i]
        c = prev[i - bpp] if i >= bpp else 0
        pred = {0: 0, 1: a, 2: b, 3: (a + b) // 2, 4: _paeth(a, b, c)}[ft]
        out.append((x - pred) & 255)
    return out


def test_load_png_round_trip_and_every_filter(tmp_path):
    img = torch.randint(0, 256, (6, 7, 3), generator=torch.Generator().manual_seed(96), dtype=torch.uint8)
    p = str(tmp_path / "a.png")
    V.save_png(img, p)
    assert torch.equal(V.load_png(p), img)
    with open(str(tmp_path / "own.png"), "wb") as f:
        f.write(V._png_bytes(img.numpy()))
    assert torch.equal(V.load_png(str(tmp_path / "own.png")), img)
    rows = [img[y].flatten().tolist() for y in range(6)]
    for ft in (1, 2, 3, 4):                               # every line with filter ft (the first line sees a zero line above)
        lines = [(ft, _filter(ft, rows[y], rows[y - 1] if y else [0] * 21, 3)) for y in range(6)]
        q = str(tmp_path / f"f{ft}.png")
        _png(q, 7, 6, 2, lines)
        got = V.load_png(q)
        assert got.dtype == torch.uint8 and got.shape == (6, 7, 3)
        assert torch.equal(got, img), ft
    mixed = [(y % 5, _filter(y % 5, rows[y], rows[y - 1] if y else [0] * 21, 3)) for y in range(6)]
    _png(str(tmp_path / "mixed.png"), 7, 6, 2, mixed)
    assert torch.equal(V.load_png(str(tmp_path / "mixed.png")), img)


def test_load_png_rgba_grey_and_refusals(tmp_path):
    g = torch.Generator().manual_seed(97)
    rgba = torch.randint(0, 256, (4, 5, 4), generator=g, dtype=torch.uint8)
    rows = [rgba[y].flatten().tolist() for y in range(4)]
    _png(str(tmp_path / "rgba.png"), 5, 4, 6, [(4, _filter(4, rows[y], rows[y - 1] if y else [0] * 20, 4)) for y in range(4)])
    assert torch.equal(V.load_png(str(tmp_path / "rgba.png")), rgba[:, :, :3])          # alpha dropped
    grey = torch.randint(0, 256, (4, 5), generator=g, dtype=torch.uint8)
    rows = [grey[y].tolist() for y in range(4)]
    _png(str(tmp_path / "grey.png"), 5, 4, 0, [(1, _filter(1, rows[y], rows[y - 1] if y else [0] * 5, 1)) for y in range(4)])
    assert torch.equal(V.load_png(str(tmp_path / "grey.png")), grey[:, :, None].expand(4, 5, 3))
    _png(str(tmp_path / "deep.png"), 5, 4, 2, [(0, [0] * 30)] * 4, depth=16)
    with pytest.raises(ValueError, match="16"):
        V.load_png(str(tmp_path / "deep.png"))
    _png(str(tmp_path / "adam7.png"), 5, 4, 2, [(0, [0] * 15)] * 4, interlace=1)
    with pytest.raises(ValueError, match="interlace"):
        V.load_png(str(tmp_path / "adam7.png"))
    _png(str(tmp_path / "pal.png"), 5, 4, 3, [(0, [0] * 5)] * 4)
    with pytest.raises(ValueError, match="colour type 3"):
        V.load_png(str(tmp_path / "pal.png"))
    with open(str(tmp_path / "not.png"), "wb") as f:
        f.write(b"GIF89a" + bytes(20))
    with pytest.raises(ValueError, match="not a PNG"):
        V.load_png(str(tmp_path / "not.png"))


# ---- add_noise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ddim", "ddpm", "lms", "euler_a"])
def test_add_noise_closed_forms(name):
    """alpha-based: sqrt(abar_t) x + sqrt(1 - abar_t) n; sigma-based: x + sigma_t n -- first, a middle and the last timestep."""
    s = scheduler.create_noise_scheduler(name)
    s.set_timesteps(10)
    g = torch.Generator().manual_seed(98)
    x = torch.randn(2, 4, 8, 8, generator=g); n = torch.randn(2, 4, 8, 8, generator=g)
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2      # diffusers' table is fp32
    abar = torch.cumprod(1 - betas, 0).double()
    for i in (0, 5, 9):
        t = s.timesteps[i]
        got = s.add_noise(x, n, t)
        assert got.shape == x.shape and got.dtype == x.dtype
        if name in ("ddim", "ddpm"):
            a = abar[int(t)]
            want = a.sqrt() * x.double() + (1 - a).sqrt() * n.double()
        else:
            sig = float(s.sigmas[i])
            lo = int(math.floor(float(t)))
            all_sig = ((1 - abar) / abar).sqrt()
            frac = float(t) - lo
            interp = float(all_sig[lo] * (1 - frac) + all_sig[min(lo + 1, 999)] * frac)
            assert abs(sig - interp) <= 1e-5 * interp
            want = x.double() + interp * n.double()
        assert rel_err(got, want.float()) < TOL32, (name, i)
    # a batch of timesteps: one per sample
    tt = torch.stack([s.timesteps[0], s.timesteps[9]])
    both = s.add_noise(x, n, tt)
    assert torch.equal(both[0], s.add_noise(x[:1], n[:1], s.timesteps[0])[0])
    assert torch.equal(both[1], s.add_noise(x[1:], n[1:], s.timesteps[9])[0])


# ---- the sampling scripts' img2img path ----------------------------------------------------------------------------------------
def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("script,model", [("infer_xl", "synthetic:tiny_xl"), ("infer", "synthetic:tiny")])
def test_infer_scripts_img2img(dev, tmp_path, script, model):
    mod = _script(script)
    img, _ = _image(1, 128, 128, 99)
    init = str(tmp_path / "init.png")
    V.save_png(img[0], init)
    png = str(tmp_path / "out.png")
    base = ["--model", model, "--height", "128", "--width", "128", "--steps", "4", "--no_graphs", "--device", str(dev),
            "--out", str(tmp_path / "latents.safetensors")]
    half = mod.main(base + ["--init_image", init, "--strength", "0.5", "--image", png]).float().cpu()
    with open(png, "rb") as f:
        b = f.read(33)
    assert struct.unpack(">IIBB", b[16:26]) == (128, 128, 8, 2)
    full = mod.main(base + ["--init_image", init, "--strength", "1.0"]).float().cpu()
    t2i = mod.main(base).float().cpu()
    assert half.shape == full.shape == t2i.shape == (1, 4, 16, 16)
    assert torch.isfinite(half).all()
    assert not torch.equal(half, full) and not torch.equal(half, t2i) and not torch.equal(full, t2i)
    with pytest.raises(ValueError, match="128"):
        mod.main(base[:2] + ["--height", "64", "--width", "128"] + base[6:] + ["--init_image", init])
    with pytest.raises(ValueError, match="strength"):
        mod.main(base + ["--init_image", init, "--strength", "0"])
