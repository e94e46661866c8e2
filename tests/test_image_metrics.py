"""`leco_amd.image_metrics` (`compare`, `overlay_change`) and `--image_diff` of the sampling scripts -- on the host emulator (CPU
tier) and on gfx950 (`-m gpu`).  The kernel itself is held against float64 in tests/test_image_metrics_kernels.py; here the
numbers only have to be the kernel's."""
import contextlib
import importlib.util
import io
import json
import math
import os
import struct

import pytest
import torch

from leco_amd import attn_maps, image_metrics, model_util
from leco_amd.lora import LoRANetwork
from leco_amd.vae import load_png, save_png

bf = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 128


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _png_size(path):
    with open(path, "rb") as fh:
        head = fh.read(33)
    return struct.unpack(">II", head[16:24])


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


# ---- compare / overlay_change -------------------------------------------------------------------------------------------------
def test_compare_takes_the_three_baseline_shapes(dev):
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (3, 20, 31, 3), generator=g, dtype=torch.uint8).to(dev)
    base = img[1]
    r3 = image_metrics.compare(img, base, change_map=True)
    r1 = image_metrics.compare(img, base[None], change_map=True)
    rb = image_metrics.compare(img, base[None].repeat(3, 1, 1, 1), change_map=True)
    for r in (r1, rb):
        assert torch.equal(r.ssim, r3.ssim) and torch.equal(r.sse, r3.sse) and torch.equal(r.change, r3.change)
        assert torch.equal(r.psnr, r3.psnr) and torch.equal(r.mse, r3.mse)
    assert r3.ssim.dtype == torch.float64 and r3.sse.dtype == torch.int64 and tuple(r3.ssim.shape) == (3,)
    assert r3.change.dtype == torch.float32 and tuple(r3.change.shape) == (3, 20, 31) and r3.change.device == img.device
    assert image_metrics.compare(img, base).change is None
    # the baseline against itself: exactly 1, an infinite PSNR; the others: the host's arithmetic on the exact SSE
    assert r3.ssim[1].item() == 1.0 and r3.sse[1].item() == 0 and math.isinf(r3.psnr[1].item()) and r3.mse[1].item() == 0.0
    d = img.cpu().long() - base.cpu().long()[None]
    assert torch.equal(r3.sse, (d * d).sum(dim=(1, 2, 3)))
    for i in (0, 2):
        assert r3.ssim[i].item() < 1.0
        assert r3.mse[i].item() == r3.sse[i].item() / (20 * 31 * 3)
        assert abs(r3.psnr[i].item() - 10 * math.log10(255 ** 2 / r3.mse[i].item())) < 1e-12
    # pairwise is not the one-baseline answer
    pw = image_metrics.compare(img, img.flip(0))
    assert pw.ssim[1].item() == 1.0 and torch.equal(pw.sse[[0, 2]], image_metrics.compare(img[[0, 2]], img[[2, 0]]).sse)


def test_compare_refuses_what_it_cannot_take(dev):
    img = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=dev)
    for bad_img, bad_ref, word in [(img.float(), img, "uint8"), (img, img.float(), "uint8"), (img[0], img[0], "[B][H][W][3]"),
                                   (img[..., :2], img[..., :2], "[B][H][W][3]"), (img, img[:, :15], "baseline"),
                                   (img, torch.zeros((3, 16, 16, 3), dtype=torch.uint8, device=dev), "baseline"),
                                   (img[:, :10], img[:, :10], "smaller"), (img[:, :, :10], img[:, :, :10], "smaller")]:
        with pytest.raises(ValueError, match=word.replace("[", r"\[").replace("]", r"\]")):
            image_metrics.compare(bad_img, bad_ref)
    if dev.type == "cuda":
        with pytest.raises(ValueError, match="are on"):
            image_metrics.compare(img, img.cpu())
    else:
        with pytest.raises(ValueError, match="are on"):
            image_metrics.compare(img, torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device="meta"))


def test_overlay_change_is_the_attention_overlay(dev):
    g = torch.Generator().manual_seed(2)
    img = torch.randint(0, 256, (2, 24, 24, 3), generator=g, dtype=torch.uint8).to(dev)
    ref = img[0].clone()
    ref[8:14, 8:14] = 255 - ref[8:14, 8:14]
    res = image_metrics.compare(img, ref, change_map=True)
    peak = res.change.amax().reshape(1, 1)
    assert peak.item() > 1e-3
    want = attn_maps.overlay(res.change[:, None], img, 0.6, peak=peak)[0]
    got = image_metrics.overlay_change(res.change, img)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 24, 24, 3) and torch.equal(got, want)
    assert torch.equal(image_metrics.overlay_change(res.change, img, full=0.5, alpha=0.3),
                       attn_maps.overlay(res.change[:, None], img, 0.3, peak=torch.full((1, 1), 0.5))[0])
    # identical pictures: no heat anywhere (full heat = 1e-3, not 0 / 0), the pictures come back
    same = image_metrics.compare(img, img, change_map=True)
    assert torch.equal(image_metrics.overlay_change(same.change, img), img)
    with pytest.raises(ValueError):
        image_metrics.overlay_change(res.change, img, full=0.0)


def test_gaussian_taps():
    t = image_metrics.gaussian_taps()
    assert t.dtype == torch.float64 and tuple(t.shape) == (11,) and abs(t.sum().item() - 1.0) < 1e-15
    assert torch.equal(t, t.flip(0)) and abs(t[5].item() / t[4].item() - math.exp(1 / (2 * 1.5 ** 2))) < 1e-14


# ---- the sampling scripts -----------------------------------------------------------------------------------------------------
def _lora_file(tmp_path, dev, xl):
    unet = (model_util.load_models_xl("synthetic:tiny_xl", "ddim") if xl else model_util.load_models("synthetic:tiny", "ddim"))[2]
    with _quiet():
        net = LoRANetwork(unet.to(dev, bf), rank=4, multiplier=1.0, alpha=1.0)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for l in net.unet_loras:
            l.lora_up.weight.copy_(torch.randn(l.lora_up.weight.shape, generator=g) * 0.3)
    f = str(tmp_path / "x_last.safetensors")
    net.save_weights(f, dtype=torch.float32)
    return f


def _base_args(xl, dev, tmp_path):
    return ["--model", "synthetic:tiny_xl" if xl else "synthetic:tiny", "--height", str(SIZE), "--width", str(SIZE), "--steps", "2",
            "--device", str(dev), "--no_graphs", "--out", str(tmp_path / "latents.safetensors")]


def _check_sweep(dev, tmp_path, stem):
    """The sweep -1, 0, 1 with the default baseline: what .diff.json and .diff.png must hold."""
    with open(str(tmp_path / (stem + ".diff.json"))) as fh:
        doc = json.load(fh)
    assert doc["strengths"] == [[-1.0], [0.0], [1.0]] and doc["baseline"] == {"cell": 1, "strengths": [0.0]}
    assert len(doc["ssim"]) == len(doc["psnr"]) == len(doc["mse"]) == 3
    assert doc["ssim"][1] == 1.0 and doc["psnr"][1] is None and doc["mse"][1] == 0.0
    sheet = load_png(str(tmp_path / (stem + ".png")))
    assert tuple(sheet.shape) == (SIZE, 3 * SIZE, 3)
    cells = torch.stack([sheet[:, i * SIZE:(i + 1) * SIZE] for i in range(3)]).to(dev)
    res = image_metrics.compare(cells, cells[1])
    for i in (0, 2):
        assert doc["ssim"][i] < 1.0 and doc["psnr"][i] is not None
        assert doc["ssim"][i] == res.ssim[i].item() and doc["psnr"][i] == res.psnr[i].item() and doc["mse"][i] == res.mse[i].item()
    assert _png_size(str(tmp_path / (stem + ".diff.png"))) == _png_size(str(tmp_path / (stem + ".png"))) == (3 * SIZE, SIZE)
    return cells


def test_infer_image_diff_with_the_other_hooks_and_a_png_baseline(dev, tmp_path):
    mod = _script("infer")
    f = _lora_file(tmp_path, dev, False)
    base = _base_args(False, dev, tmp_path)
    others = ["--lora", f, "--lora_scales", "-1,0,1", "--clip_score", "a photo", "--attn_map", "#2"]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        mod.main(base + others + ["--image", str(tmp_path / "s.png"), "--image_diff"])
    assert out.getvalue().count("image diff strengths") == 3 and "image diff strengths 0: ssim 1.0000 psnr inf" in out.getvalue()
    cells = _check_sweep(dev, tmp_path, "s")
    # all three outputs are there, and the other two are what they are without --image_diff
    with _quiet():
        mod.main(base + others + ["--image", str(tmp_path / "t.png")])
    assert not os.path.exists(str(tmp_path / "t.diff.json"))
    for ext in (".scores.json", ".attn.json", ".attn.png", ".png"):
        assert _read(str(tmp_path / ("s" + ext))) == _read(str(tmp_path / ("t" + ext))), ext

    # a PNG as the baseline, no sweep
    png = str(tmp_path / "cell.png")
    save_png(cells[2].cpu(), png)
    with _quiet():
        mod.main(base + ["--image", str(tmp_path / "one.png"), "--image_diff", png])
    with open(str(tmp_path / "one.diff.json")) as fh:
        doc = json.load(fh)
    assert doc["baseline"] == {"png": png} and doc["strengths"] == [None] and len(doc["ssim"]) == 1
    one = load_png(str(tmp_path / "one.png")).to(dev)
    assert doc["ssim"][0] == image_metrics.compare(one[None], cells[2]).ssim[0].item() < 1.0
    assert _png_size(str(tmp_path / "one.diff.png")) == (SIZE, SIZE)


def test_a_cell_named_by_its_strengths_is_the_baseline(dev, tmp_path):
    """`--image_diff -1` and, for a stack of two files, `--image_diff 0,1`: the flags and the hook on pictures of the test's own
    (no model is needed to resolve a cell or to compare it)."""
    import argparse
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import _image_diff
    import _lora_sweep
    g = torch.Generator().manual_seed(4)
    for scale_flags, named, cell, cols in [(["--lora", "a", "--lora_scales", "-1,0,1"], "-1", 0, 3),
                                           (["--lora", "a", "--lora", "b", "--lora_scales", "0,1", "--lora_scales", "-1,0,1"], "0,1", 2, 3),
                                           (["--lora", "a", "--lora", "b", "--lora_scales", "0,1", "--lora_scales", "-1,0,1"], None, 1, 3)]:
        ap = argparse.ArgumentParser()
        _lora_sweep.add_arguments(ap)
        _image_diff.add_arguments(ap)
        for flag in ("--image", "--height", "--width"):
            ap.add_argument(flag, type=str if flag == "--image" else int)
        image = str(tmp_path / ("n%d.png" % cell))
        argv = scale_flags + ["--image", image, "--height", "40", "--width", "24", "--image_diff"] + ([named] if named else [])
        args = ap.parse_args(_image_diff.join_base(_lora_sweep.join_scales(argv)))
        scales = _lora_sweep.parse_scales(ap, args)
        _image_diff.check(ap, args, scales)
        assert args.image_diff_base == ("cell", cell)
        n = len(scales)
        img = torch.randint(0, 256, (n, 40, 24, 3), generator=g, dtype=torch.uint8).to(dev)
        seen = []
        with _quiet():
            _image_diff.hook(args, scales, cols=args.sheet_cols, also=seen.append)(img)
        assert len(seen) == 1 and seen[0] is img                                     # the chained hook ran, on the same pictures
        with open(image[:-4] + ".diff.json") as fh:
            doc = json.load(fh)
        res = image_metrics.compare(img, img[cell], change_map=True)
        assert doc["baseline"]["cell"] == cell and doc["strengths"] == [list(s) if isinstance(s, tuple) else [s] for s in scales]
        assert doc["ssim"] == res.ssim.tolist() and doc["ssim"][cell] == 1.0 and doc["psnr"][cell] is None
        # the change maps over the pictures on ONE scale, laid out like the sheet
        over = image_metrics.overlay_change(res.change, img)
        want = torch.cat([torch.cat(list(over[i:i + cols]), dim=1) for i in range(0, n, cols)], dim=0)
        assert torch.equal(load_png(image[:-4] + ".diff.png"), want.cpu())


def test_infer_xl_image_diff(dev, tmp_path):
    mod = _script("infer_xl")
    f = _lora_file(tmp_path, dev, True)
    with _quiet():
        mod.main(_base_args(True, dev, tmp_path) + ["--lora", f, "--lora_scales", "-1,0,1", "--image", str(tmp_path / "s.png"),
                                                    "--image_diff"])
    _check_sweep(dev, tmp_path, "s")


@pytest.mark.parametrize("name", ["infer", "infer_xl"])
def test_flag_errors_come_before_any_model_is_loaded(name, tmp_path, monkeypatch):
    mod = _script(name)

    def no_model(*a, **k):
        raise AssertionError("a model was loaded before the flags were checked")
    monkeypatch.setattr(model_util, "load_models", no_model)
    monkeypatch.setattr(model_util, "load_models_xl", no_model)
    monkeypatch.setattr(model_util, "load_vae", no_model)
    base = ["--model", "synthetic:tiny_xl" if name == "infer_xl" else "synthetic:tiny", "--height", str(SIZE), "--width", str(SIZE),
            "--steps", "2", "--device", "cpu", "--out", str(tmp_path / "l.safetensors")]
    small = str(tmp_path / "small.png")
    save_png(torch.zeros((64, 64, 3), dtype=torch.uint8), small)
    img = ["--image", str(tmp_path / "x.png")]
    sweep = ["--lora", str(tmp_path / "none.safetensors"), "--lora_scales", "-1,1"]
    for argv, word in [(["--image_diff"], "needs --image"),
                       (img + sweep + ["--image_diff"], "no cell with strengths 0"),
                       (img + sweep + ["--image_diff", "0.5"], "no cell with strengths 0.5"),
                       (img + sweep + ["--image_diff", "0,1"], "2 strengths"),
                       (img + ["--image_diff"], "needs a baseline PNG"),
                       (img + ["--image_diff", "-1"], "needs a baseline PNG"),
                       (img + ["--image_diff", str(tmp_path / "missing.png")], "readable PNG"),
                       (img + ["--image_diff", small], "64x64")]:
        err = io.StringIO()
        with pytest.raises(SystemExit), contextlib.redirect_stderr(err):
            mod.main(base + argv)
        assert word in err.getvalue(), (argv, err.getvalue())
