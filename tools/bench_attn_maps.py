#!/usr/bin/env python
"""Measurement only: what collecting cross-attention token maps costs one CFG-doubled UNet pass (batch 2) of `synthetic:sd15`
at 512^2 (64 x 64 latents), LoRA off, each route replayed from its hipGraph:

  * the plan `forward` runs by default (the sampling scripts' pass without `--attn_map`),
  * the forward-only plan with the row-stripe kernels,
  * the forward-only plan built with LECO_STRIPE=0 (every block per op: the route a maps plan takes),
  * the maps plan (`Engine.plan(attn_maps=M)`): the per-op route + one `leco_xattn_token_maps` launch per cross-attention,

and the token-map launches of that plan alone, as a graph of their own.

    python tools/bench_attn_maps.py [--maps 2] [--reps 20] > profiles/attn_maps.txt
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from leco_amd import graphs, model_util  # noqa: E402
from leco_amd.unet import UNet2DConditionModel, sd15_config  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_maps.py measures on the GPU; there is none")
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    cfg = sd15_config()
    unet = model_util.init_synthetic_(UNet2DConditionModel(cfg)).to(dev, bf)
    unet.requires_grad_(False)
    eng = unet.engine()
    h = args.size // 8
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, h, h, generator=g).to(dev, bf)
    ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).to(dev, bf)
    os.environ.pop("LECO_STRIPE", None)
    plans = [("forward's default plan", eng.plan(2, h, h)), ("forward-only, stripe kernels", eng.plan(2, h, h, need_bwd=False))]
    os.environ["LECO_STRIPE"] = "0"
    plans.append(("forward-only, LECO_STRIPE=0 (per op)", eng.plan(2, h, h, need_bwd=False, tag="nostripe")))
    del os.environ["LECO_STRIPE"]
    mp = eng.plan(2, h, h, need_bwd=False, attn_maps=args.maps)
    mp.tok_w[:, 1:1 + args.maps].fill_diagonal_(1.0)
    plans.append((f"maps plan, {args.maps} words", mp))
    us = {}
    for name, p in plans:
        p.x_in.copy_(x)
        p.set_ctx(ctx)
        p.t_table[:1].fill_(500.0)
        p.t_idx.zero_()
        us[name] = (graphs.replay_us(p.fwd[False], reps=args.reps), len(p.fwd[False]))
    only = [op for op in mp.fwd[False] if op.name == "leco_xattn_token_maps"]
    us_only = graphs.replay_us(only, reps=args.reps)
    names = [n for n, _ in plans]
    print(f"# cross-attention token maps: one CFG-doubled UNet pass (batch 2, the maps of the cond sample) of synthetic:sd15 at "
          f"{args.size}^2, LoRA off")
    print(f"# hipGraph replay, mean of {args.reps} replays after 3 warm-ups, us; launches = kernels in the list")
    for n in names:
        print(f"{n:<40s} {us[n][0]:10.1f} us  {us[n][1]:4d} launches")
    print(f"{'the ' + str(len(only)) + ' token-map launches alone':<40s} {us_only:10.1f} us")
    base, route, maps = us[names[1]][0], us[names[2]][0], us[names[3]][0]
    print(f"maps plan - forward-only stripe plan     {maps - base:10.1f} us  ({100 * (maps - base) / base:+.1f} %): "
          f"route {route - base:.1f} us, map launches {maps - route:.1f} us")
    print(f"maps plan - forward's default plan       {maps - us[names[0]][0]:10.1f} us  ({100 * (maps - us[names[0]][0]) / us[names[0]][0]:+.1f} %)")
    unet.release()


if __name__ == "__main__":
    main()
