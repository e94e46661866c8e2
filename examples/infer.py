#!/usr/bin/env python
"""Sampling script for SD1.x / SD2.x -- `examples/infer_xl.py` for the non-XL models.

`model_util.load_models` -> `train_util.encode_prompts` for the prompt and the negative prompt -> `concat_embeddings` ->
`get_initial_latents` -> `train_util.diffusion` (DDIM, classifier-free guidance) through the HIP UNet, optionally with a
trained LoRA applied (`--lora out/x_last.safetensors`, the file `train_lora.py` writes).  The latents go to a safetensors
file (`--out`); with `--image PATH` they are decoded by the HIP VAE decoder (`leco_amd/vae.py`) and saved as a PNG, as
the reference's `test/infer_xl.py:136-154` does for SDXL.  With `--init_image PNG --strength S` the run is img2img: the
image is encoded by the HIP VAE encoder, noised to the timestep `S` selects, and only the rest of the schedule is run.

    python examples/infer.py --model synthetic:tiny --height 128 --width 128 --steps 4 --image out.png
    python examples/infer.py --model synthetic:tiny --height 128 --width 128 --steps 4 --init_image out.png --strength 0.5 --image out2.png
    python examples/infer.py --model synthetic:tiny --height 128 --width 128 --steps 4 --lora x_last.safetensors --lora_scales -2,-1,0,1,2 --image sheet.png
    python examples/infer.py --model /models/sd21 --v2 --v_pred --height 768 --width 768 --lora output/x_last.safetensors --image x.png

`--lora FILE` reads rank, alpha and coverage from the file (`--rank` / `--alpha` override).  `--lora_scales` is the slider
sweep: one seed and one initial latent (or `--init_image`) at every strength, all strengths through each denoising step as one
batch (`LoRANetwork.set_strengths`, bf16 only); `--image` becomes a contact sheet, left to right, `--out` holds [n,4,h,w].
`--lora` may be repeated: the files are stacked (`LoRANetwork.from_files`), `--lora_multipliers a,b` sets one fixed multiplier
per file, and `--lora_scales`, given once per `--lora` in the same order, samples the cross product in one batched pass (first
file slowest; the contact sheet has the last file's strengths left to right, the other combinations top to bottom).

`--clip_score TEXT` (repeatable, needs `--image`) scores every decoded picture against TEXT with the native CLIP image tower
(`--clip_model`: a local transformers CLIPModel folder, or `synthetic:vit_tiny` -- the default for `synthetic:*` models): one
line per picture, with its strengths in a sweep, and the same table in `<image stem>.scores.json` (`_clip_score.py`).

`--attn_map WORD` (repeatable, needs `--image`) draws where in the picture WORD of the prompt acts: the cross-attention heat of
its tokens over every decoded picture (`<image stem>.attn.png`, the layout of `--image` once per word, top to bottom) and the
mean heat per cell in `<image stem>.attn.json`; `#3` / `#3-5` name raw token positions (`_attn_map.py`).

`--image_diff [BASE]` (needs `--image`) says what else changed: SSIM, PSNR and MSE of every decoded picture against a baseline
-- the all-zero cell of `--lora_scales` by default, another cell named by its strengths (`-1`, `0,1`), or a PNG of the same
size -- in `<image stem>.diff.json`, and the change maps 1 - ssim over the pictures in `<image stem>.diff.png` (`_image_diff.py`).
"""
import argparse
import contextlib
import importlib.util
import os
import sys

import torch
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from leco_amd import model_util, train_util  # noqa: E402
import _attn_map  # noqa: E402
import _clip_score  # noqa: E402
import _image_diff  # noqa: E402
import _lora_sweep  # noqa: E402
from _img2img import init_latents  # noqa: E402


def _infer_xl():
    spec = importlib.util.spec_from_file_location("infer_xl", os.path.join(HERE, "infer_xl.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_image(*a, **k):
    return _infer_xl().write_image(*a, **k)


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="synthetic:tiny")
    ap.add_argument("--v2", action="store_true")
    ap.add_argument("--v_pred", action="store_true")
    ap.add_argument("--prompt", default="a photo of lemonade")
    ap.add_argument("--negative_prompt", default="")
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--guidance_scale", type=float, default=7.5)
    _lora_sweep.add_arguments(ap)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--no_graphs", action="store_true", help="eager launches instead of one hipGraph per UNet pass")
    ap.add_argument("--out", default="latents.safetensors")
    ap.add_argument("--image", default=None, help="decode the latents with the VAE and write this PNG")
    ap.add_argument("--vae", default=None, help="VAE for --image (default: the model's vae/ folder, or its synthetic VAE)")
    ap.add_argument("--init_image", default=None, help="img2img: start from this PNG (its size must be --height x --width)")
    ap.add_argument("--strength", type=float, default=0.6, help="img2img: 0 < S <= 1, the share of the schedule that is run")
    ap.add_argument("--native_text_encoder", action="store_true",
                    help="encode the prompts with the native CLIP text encoder (leco_amd.clip, bf16 only) instead of transformers")
    _clip_score.add_arguments(ap)
    _attn_map.add_arguments(ap)
    _image_diff.add_arguments(ap)
    args = ap.parse_args(_image_diff.join_base(_lora_sweep.join_scales(argv)))
    scales = _lora_sweep.parse_scales(ap, args)
    _clip_score.check(ap, args)
    _attn_map.check(ap, args)
    _image_diff.check(ap, args, scales)
    n = 1 if scales is None else len(scales)
    dev = torch.device(args.device)
    dtype = torch.bfloat16
    if args.init_image and not 0.0 < args.strength <= 1.0:
        raise ValueError(f"--strength must be in (0, 1], got {args.strength}")
    tokenizer, text_encoder, unet, sched = model_util.load_models(args.model, scheduler_name="ddim", v2=args.v2, v_pred=args.v_pred,
                                                                  native_text_encoder=args.native_text_encoder)
    text_encoder.to(dev, dtype=dtype)
    text_encoder.eval()
    unet.to(dev, dtype=dtype)
    unet.enable_xformers_memory_efficient_attention()
    unet.requires_grad_(False)
    unet.eval()
    unet.use_graphs = dev.type == "cuda" and not args.no_graphs
    network = _lora_sweep.load_network(unet, args, scales)
    pos = train_util.encode_prompts(tokenizer, text_encoder, [args.prompt])
    neg = train_util.encode_prompts(tokenizer, text_encoder, [args.negative_prompt])
    text_embeds = train_util.concat_embeddings(neg, pos, n)
    amap = _attn_map.start(args, unet, tokenizer, args.prompt)
    sched.set_timesteps(args.steps, device=dev)
    torch.manual_seed(args.seed)
    t_start = 0
    if args.init_image:
        latents, t_start = init_latents(args, sched, dev, use_graphs=unet.use_graphs)
        latents = latents.to(dtype)
    else:
        latents = train_util.get_initial_latents(sched, 1, args.height, args.width, 1).to(dev, dtype=dtype)
    if scales is not None:      # one seed, one initial latent: the same start at every strength
        latents = latents.repeat(n, 1, 1, 1)
    with (network if network is not None else contextlib.nullcontext()):
        latents = train_util.diffusion(unet, sched, latents, text_embeds, total_timesteps=args.steps, start_timesteps=t_start,
                                       guidance_scale=args.guidance_scale)
    save_file({"latents": latents.float().cpu().contiguous()}, args.out,
              {"prompt": args.prompt, "steps": str(args.steps), "guidance_scale": str(args.guidance_scale)})
    print(f"Done. latents {tuple(latents.shape)} -> {args.out}")
    score = _clip_score.hook(args, scales, dev, use_graphs=unet.use_graphs)
    score = _attn_map.hook(args, scales, unet, amap, cols=args.sheet_cols, also=score)
    score = _image_diff.hook(args, scales, cols=args.sheet_cols, also=score)
    if args.image and scales is None:
        _write_image(latents, args.vae or args.model, args.image, dev, use_graphs=unet.use_graphs, on_pictures=score)
    elif args.image:
        _lora_sweep.write_sheet(latents, args.vae or args.model, args.image, dev, use_graphs=unet.use_graphs, cols=args.sheet_cols,
                                on_pictures=score)
    return latents


if __name__ == "__main__":
    main()
