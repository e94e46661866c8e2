#!/usr/bin/env python
"""Measurement only: `leco_image_compare` (mean SSIM, SSE and the change map of a batch of 8-bit pictures against one baseline)
at 512^2 and 1024^2, batch 1 and 9, replayed from a hipGraph, beside a torch statement of the same SSIM on the same device:
fp32 `F.conv2d` of the five moment planes with the same 11 x 11 window (timed with HIP events around eager calls; the uint8
-> fp32 conversion is outside the timed region, and torch's statement gives no SSE).

    python tools/bench_image_metrics.py [--reps 20] > profiles/image_metrics.txt
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from leco_amd import graphs, image_metrics, ops  # noqa: E402


def torch_ssim(x, y, win):
    """x, y fp32 [B * 3][1][H][W]: per-pixel SSIM on the valid region"""
    mx, my = F.conv2d(x, win), F.conv2d(y, win)
    sxx, syy, sxy = F.conv2d(x * x, win) - mx * mx, F.conv2d(y * y, win) - my * my, F.conv2d(x * y, win) - mx * my
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    return ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_metrics.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    taps64 = image_metrics.gaussian_taps()
    taps = taps64.float().to(dev)
    win = torch.outer(taps64, taps64).float()[None, None].to(dev)
    print("# leco_image_compare (two launches: tiles, finish) against one baseline picture, with the change map")
    print(f"# hipGraph replay, mean of {args.reps} replays after 3 warm-ups, us; torch: eager fp32 F.conv2d statement of the same "
          f"SSIM, mean of {args.reps} calls after 3")
    print(f"{'shape':<16s} {'leco_image_compare':>20s} {'torch F.conv2d':>16s} {'max |ssim diff|':>16s}")
    for size in (512, 1024):
        for batch in (1, 9):
            img = torch.randint(0, 256, (batch, size, size, 3), generator=g, dtype=torch.uint8)
            img = ((img.float() + img.float().roll(1, 1) + img.float().roll(1, 2)) / 3).to(torch.uint8).to(dev)     # not pure noise
            ref = img[0].roll(3, 1).contiguous()
            stats = torch.empty((batch, 2), dtype=torch.float64, device=dev)
            change = torch.empty((batch, size, size), dtype=torch.float32, device=dev)
            op = ops.image_compare(img, ref, 0, batch, size, size, taps, change, stats)
            us = graphs.replay_us([op], reps=args.reps)
            x = img.float().permute(0, 3, 1, 2).reshape(batch * 3, 1, size, size).contiguous()
            y = ref.float().permute(2, 0, 1)[None].expand(batch, 3, size, size).reshape(batch * 3, 1, size, size).contiguous()
            for _ in range(3):
                s = torch_ssim(x, y, win)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                s = torch_ssim(x, y, win)
            e1.record()
            e1.synchronize()
            us_t = e0.elapsed_time(e1) / args.reps * 1e3
            s = s.reshape(batch, 3, size - 10, size - 10).mean(1)
            diff = (1.0 - change[:, 5:-5, 5:-5] - s).abs().max().item()
            print(f"{f'{batch} x {size}^2':<16s} {us:17.1f} us {us_t:13.1f} us {diff:16.3g}")


if __name__ == "__main__":
    main()
