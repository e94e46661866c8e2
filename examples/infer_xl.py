#!/usr/bin/env python
"""Sampling smoke script -- the counterpart of the reference's `test/infer_xl.py` (:40-154) on the MI355X path.

Same flow: `model_util.load_models_xl` -> `train_util.encode_prompts_xl` for the prompt and the negative prompt ->
`concat_embeddings` of the text / pooled embeddings and the `add_time_ids` -> `get_initial_latents` (+ the SDXL noise
offset) -> `train_util.diffusion_xl` (DDIM, classifier-free guidance 7) through the HIP UNet, optionally with a trained
LoRA applied (`--lora out/x_last.safetensors`, the file `train_lora_xl.py` writes).

The latents are written to a safetensors file (`--out`).  With `--image PATH` the script goes on as the reference does
(:136-154): `vae.decode(latents / scaling_factor)`, denormalise, save a PNG -- through the HIP VAE decoder
(`leco_amd/vae.py`; `--vae` names the VAE: a diffusers folder, a single-file checkpoint or `synthetic:...`; default: the
model's own `vae/` folder, or the synthetic VAE of a synthetic model).  Without `--image` nothing about the VAE is loaded.

With `--init_image PNG --strength S` (0 < S <= 1, default 0.6) the run is img2img: the PNG (its size must be `--height` x
`--width`) is encoded by the HIP VAE encoder (`encode_to_latents`, the same `--vae`), noised with `scheduler.add_noise` to
`timesteps[steps - min(int(steps * S), steps)]`, and the rest of the schedule is run -- with and without `--lora`, so one
can see what a trained LoRA does to a given picture.

    python examples/infer_xl.py --model synthetic:tiny_xl --height 128 --width 128 --steps 4 --image out.png
    python examples/infer_xl.py --model synthetic:tiny_xl --height 128 --width 128 --steps 4 --init_image out.png --strength 0.5 --image out2.png
    python examples/infer_xl.py --model synthetic:tiny_xl --height 128 --width 128 --steps 4 --lora x_last.safetensors --lora_scales -2,-1,0,1,2 --image sheet.png
    python examples/infer_xl.py --model /models/sdxl-base --lora output/x_last.safetensors --prompt "a photo of lemonade" --image lemonade.png

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

SDXL_NOISE_OFFSET = 0.0357      # test/infer_xl.py:27


@torch.no_grad()
def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="synthetic:tiny_xl")
    ap.add_argument("--prompt", default="a photo of lemonade")
    ap.add_argument("--negative_prompt", default="")
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--guidance_scale", type=float, default=7.0)
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
    tokenizers, text_encoders, unet, sched = model_util.load_models_xl(args.model, scheduler_name="ddim",
                                                                        native_text_encoder=args.native_text_encoder)
    for te in text_encoders:
        te.to(dev, dtype=dtype)
        te.eval()
    unet.to(dev, dtype=dtype)
    unet.enable_xformers_memory_efficient_attention()
    unet.requires_grad_(False)
    unet.eval()
    unet.use_graphs = dev.type == "cuda" and not args.no_graphs
    network = _lora_sweep.load_network(unet, args, scales)
    add_time_ids = train_util.get_add_time_ids(args.height, args.width, dynamic_crops=False).to(dev)
    pos, pos_pooled = train_util.encode_prompts_xl(tokenizers, text_encoders, [args.prompt], num_images_per_prompt=1)
    neg, neg_pooled = train_util.encode_prompts_xl(tokenizers, text_encoders, [args.negative_prompt], num_images_per_prompt=1)
    text_embeds = train_util.concat_embeddings(neg, pos, n)
    add_text_embeds = train_util.concat_embeddings(neg_pooled, pos_pooled, n)
    add_time_ids = train_util.concat_embeddings(add_time_ids, add_time_ids, n)
    amap = _attn_map.start(args, unet, tokenizers[0], args.prompt)
    sched.set_timesteps(args.steps, device=dev)
    torch.manual_seed(args.seed)
    t_start = 0
    if args.init_image:
        latents, t_start = init_latents(args, sched, dev, use_graphs=unet.use_graphs)
        latents = latents.to(dtype)
    else:
        latents = train_util.get_initial_latents(sched, 1, args.height, args.width, 1)
        latents = train_util.apply_noise_offset(latents * sched.init_noise_sigma, SDXL_NOISE_OFFSET).to(dev, dtype=dtype)
    if scales is not None:      # one seed, one initial latent: the same start at every strength
        latents = latents.repeat(n, 1, 1, 1)
    with (network if network is not None else contextlib.nullcontext()):
        latents = train_util.diffusion_xl(unet, sched, latents, text_embeddings=text_embeds,
                                          add_text_embeddings=add_text_embeds, add_time_ids=add_time_ids,
                                          total_timesteps=args.steps, start_timesteps=t_start, guidance_scale=args.guidance_scale)
    save_file({"latents": latents.float().cpu().contiguous()}, args.out,
              {"prompt": args.prompt, "steps": str(args.steps), "guidance_scale": str(args.guidance_scale)})
    print(f"Done. latents {tuple(latents.shape)} -> {args.out}")
    score = _clip_score.hook(args, scales, dev, use_graphs=unet.use_graphs)
    score = _attn_map.hook(args, scales, unet, amap, cols=args.sheet_cols, also=score)
    score = _image_diff.hook(args, scales, cols=args.sheet_cols, also=score)
    if args.image and scales is None:
        write_image(latents, args.vae or args.model, args.image, dev, use_graphs=unet.use_graphs, on_pictures=score)
    elif args.image:
        _lora_sweep.write_sheet(latents, args.vae or args.model, args.image, dev, use_graphs=unet.use_graphs, cols=args.sheet_cols,
                                on_pictures=score)
    return latents


def write_image(latents, vae_path, png_path, dev, use_graphs=False, on_pictures=None):
    """test/infer_xl.py:136-154: decode (the division by the scaling factor happens inside `decode_to_uint8`), denormalise,
    round to 8 bits (the output convolution's epilogue) and save the first image.  ``on_pictures``: called with the uint8
    [n][H][W][3] pictures where the decoder left them (`--clip_score`)."""
    from leco_amd.vae import save_png
    vae = model_util.load_vae(vae_path).to(dev)
    vae.use_graphs = use_graphs
    img = vae.decode_to_uint8(latents.float())
    if on_pictures is not None:
        on_pictures(img)
    save_png(img[0], png_path)
    vae.release()
    print(f"image {img.shape[2]}x{img.shape[1]} -> {png_path}")


if __name__ == "__main__":
    main()
