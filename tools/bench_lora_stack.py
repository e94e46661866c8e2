#!/usr/bin/env python
"""Measurement only: a 3 x 3 slider grid of two stacked LoRA files (`LoRANetwork.from_files`: lierla rank 4 + c3lier rank 8,
seeded random weights) on the `synthetic:sd15` UNet at 512^2 (64 x 64 latents) -- ONE CFG-doubled UNet pass at batch 18
through the sweep plan (`set_strengths`, `leco_lora_rowscale_stack` at every LoRA site) against NINE CFG-doubled passes at
batch 2 through the ordinary plan with `set_multipliers` between them (each change re-packs the LoRA operands).  Both sides
are what one denoising step of the grid costs; hipGraph replay on both.

    python tools/bench_lora_stack.py [--iters 10] > profiles/lora_stack.txt
"""
import argparse
import contextlib
import io
import itertools
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from leco_amd import model_util  # noqa: E402
from leco_amd.lora import DEFAULT_TARGET_REPLACE, UNET_TARGET_REPLACE_MODULE_CONV, LoRANetwork  # noqa: E402
from leco_amd.unet import UNet2DConditionModel, sd15_config  # noqa: E402

FILES = ((4, 1.0, list(DEFAULT_TARGET_REPLACE)), (8, 4.0, list(DEFAULT_TARGET_REPLACE) + list(UNET_TARGET_REPLACE_MODULE_CONV)))
GRID = list(itertools.product((-1.0, 0.0, 1.0), (0.0, 1.0, 2.0)))


def _time(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora_stack.py measures on the GPU; there is none")
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    cfg = sd15_config()
    unet = model_util.init_synthetic_(UNet2DConditionModel(cfg)).to(dev, bf)
    unet.requires_grad_(False)
    g = torch.Generator().manual_seed(0)
    folder = tempfile.mkdtemp()
    paths = []
    for j, (rank, alpha, targets) in enumerate(FILES):
        with contextlib.redirect_stdout(io.StringIO()):
            net = LoRANetwork(unet, rank=rank, alpha=alpha, target_replace_modules=targets)
        with torch.no_grad():
            for l in net.unet_loras:
                l.lora_up.weight.copy_(torch.randn(l.lora_up.weight.shape, generator=g) * 0.02)
        paths.append(os.path.join(folder, f"file{j}.safetensors"))
        net.save_weights(paths[-1], dtype=torch.float32)
    stack = LoRANetwork.from_files(unet, paths)
    unet.use_graphs = True
    h = args.size // 8
    n = len(GRID)
    x = torch.randn(1, 4, h, h, generator=g).to(dev, bf)
    ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).to(dev, bf)
    t = torch.tensor(500)
    x2, xn, ctxn = x.repeat(2, 1, 1, 1), x.repeat(2 * n, 1, 1, 1), ctx.repeat_interleave(n, 0)

    def grid_pass():
        return unet(xn, t, encoder_hidden_states=ctxn).sample

    def nine_passes():
        out = []
        for pair in GRID:
            stack.set_multipliers(pair)
            out.append(unet(x2, t, encoder_hidden_states=ctx).sample)
        return out

    with torch.no_grad():
        stack.set_strengths(GRID)
        y_grid = grid_pass().float()
        t_grid = _time(grid_pass, args.iters)
        sites = sum(1 for op in unet.engine().plan(2 * n, h, h, need_bwd=False, strengths=True).lists["fwd_on"]
                    if op.name == "leco_lora_rowscale_stack")
        stack.set_strengths(None)
        y_nine = [y.float() for y in nine_passes()]
        t_nine = _time(nine_passes, args.iters)
    # the two sides compute the same grid (bf16 rounding apart): cell i of the batched pass against fixed pass i
    dev_max = max(((torch.stack([y_grid[i], y_grid[n + i]]) - y_nine[i]).norm() / y_nine[i].norm()).item() for i in range(n))
    print(f"# stacked LoRA files, 3 x 3 strength grid, synthetic:sd15 UNet at {args.size}^2, files: lierla rank 4 alpha 1 + c3lier "
          f"rank 8 alpha 4 (stacked rank {stack.lora_dim}, {len(stack.unet_loras)} modules, {sites} row-scale launches per pass)")
    print(f"# one denoising step of the grid, hipGraph replay, median (min .. max) of {args.iters} after two warm-ups, ms")
    print(f"one batched pass, UNet batch {2 * n} (set_strengths)             {t_grid[0]:9.3f}  ({t_grid[1]:.3f} .. {t_grid[2]:.3f})")
    print(f"nine passes, UNet batch 2 (set_multipliers + re-pack each)  {t_nine[0]:9.3f}  ({t_nine[1]:.3f} .. {t_nine[2]:.3f})")
    print(f"nine passes / one batched pass                               {t_nine[0] / t_grid[0]:9.2f} x")
    print(f"largest relative L2 between a grid cell and its fixed-multiplier pass: {dev_max:.3g}")
    unet.release()


if __name__ == "__main__":
    main()
