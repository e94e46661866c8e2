#!/usr/bin/env python
"""Measurement only: the native CLIP image tower (leco_amd/clip_vision.py, `synthetic:vit_l`: ViT-L/14, 257 tokens) from
512 x 512 uint8 pictures on the device -- preprocessing included -- replayed from its hipGraph and launched eagerly, beside
transformers' `CLIPVisionModelWithProjection` in torch-bf16 eager on the same weights and the same device (given pixels that
are already preprocessed: its own preprocessing runs on the CPU in PIL and is not timed).  With --per-op the plan is also
timed launch by launch, summed per kind of launch: the share of the attention launches at 257 tokens is what decides whether
a dedicated kernel is worth building.  There is no pass mark.

    python tools/bench_clip_vision.py [--batches 1 9] [--iters 20] [--per-op] > profiles/clip_vision.txt
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from leco_amd import model_util  # noqa: E402
from tools.timing import print_per_op, time_ms  # noqa: E402


def _transformers_model(model, dev):
    try:
        import transformers as tr
    except ImportError:
        return None
    c = model.cfg
    hf = tr.CLIPVisionModelWithProjection(tr.CLIPVisionConfig(
        hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
        num_attention_heads=c.num_attention_heads, image_size=c.image_size, patch_size=c.patch_size, hidden_act=c.hidden_act,
        projection_dim=c.projection_dim, layer_norm_eps=c.layer_norm_eps))
    sd = model.state_dict()
    if not any(k.startswith("vision_model.") for k in hf.state_dict()):
        sd = {(k if k.startswith("visual_projection.") else k[len("vision_model."):]): v for k, v in sd.items()}
    hf.load_state_dict(sd, strict=False)
    return hf.to(dev, torch.bfloat16).eval()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="synthetic:vit_l")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 9])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--per-op", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    model = model_util.load_clip_scorer(args.model).vision.to(dev)
    cfg = model.cfg
    hf = None if args.no_torch else _transformers_model(model, dev)
    print(f"# CLIP image tower {args.model} ({cfg.hidden_size} wide, {cfg.num_hidden_layers} layers, {cfg.num_patches + 1} tokens) "
          f"from {args.size}x{args.size} uint8 pictures, median (min .. max) of {args.iters} after two warm-ups, ms; device: "
          f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    for B in args.batches:
        img = torch.randint(0, 256, (B, args.size, args.size, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(B)).to(dev)
        line, plan = f"B={B}:", None
        for graphs in (True, False):
            model.release()
            model.use_graphs = graphs
            model.encode_images(img)                 # builds the plan (and captures)
            plan = model.engine().plan(B, (args.size, args.size))
            med, lo, hi = time_ms(lambda: model._run(plan), args.iters)
            line += f"  native {'graph' if graphs else 'eager'} {med:.3f} ({lo:.3f} .. {hi:.3f})"
        line += f"  launches {len(plan.ops)}"
        if hf is not None:
            px = torch.randn(B, 3, cfg.image_size, cfg.image_size, device=dev, dtype=torch.bfloat16)
            with torch.no_grad():
                med, lo, hi = time_ms(lambda: hf(pixel_values=px).image_embeds, args.iters)
            line += f"  transformers bf16 eager (preprocessed pixels) {med:.3f} ({lo:.3f} .. {hi:.3f})"
        print(line, flush=True)
        if args.per_op:
            print_per_op(plan)
    model.release()


if __name__ == "__main__":
    main()
