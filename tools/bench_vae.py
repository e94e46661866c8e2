#!/usr/bin/env python
"""Measurement only: VAE decode time from the launch plan at 512^2 and 1024^2 (batch 1, `synthetic:sd15` decoder: the real
SD shape -- 64x64 latents -> 512^2 has S = 4096 in the mid-block attention), beside torch-bf16 running the plain PyTorch
decoder the tests use (tests/test_vae.py `decoder_ref`).  With --per-op the plan is also timed launch by launch.

    python tools/bench_vae.py [--sizes 512 1024] [--iters 5] [--per-op] > profiles/vae_decode.txt

With --encode the same for the encoder (`encode_to_latents` of an 8-bit image: one plan from leco_conv_in_rgb to the
moments epilogue), beside torch-bf16 running tests/test_vae_encoder.py `encoder_ref`:

    python tools/bench_vae.py --encode --per-op > profiles/vae_encode.txt
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from leco_amd import model_util, ops  # noqa: E402


def _time(fn, iters):
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--per-op", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--encode", action="store_true", help="time the encoder instead of the decoder")
    args = ap.parse_args(argv)
    if args.encode:
        return main_encode(args)
    from test_vae import decoder_ref
    dev = torch.device("cuda:0")
    vae = model_util.load_vae("synthetic:sd15").to(dev)
    sd = {k: v.detach().to(dev, torch.bfloat16) for k, v in vae.state_dict().items()}
    print(f"# VAE decode, synthetic:sd15 decoder, batch 1, median (min .. max) of {args.iters} after one warm-up, ms")
    for size in args.sizes:
        h = size // 8
        lat = (torch.randn(1, 4, h, h, generator=torch.Generator().manual_seed(1)) * 0.18215).to(dev)
        for graphs in (False, True):
            vae.release()
            vae.use_graphs = graphs
            vae.decode_to_uint8(lat)                 # builds the plan (and captures)
            plan = vae.engine().plan(1, h, h)
            med, lo, hi = _time(lambda: vae._run(plan), args.iters)
            print(f"{size}x{size} hip plan {'graph' if graphs else 'eager'}: {med:.3f} ({lo:.3f} .. {hi:.3f})  "
                  f"launches {len(plan.ops)}  activation pool {plan.pool.nbytes() / 2 ** 20:.0f} MiB")
        if args.per_op:
            rows = []
            for op in plan.ops:
                med, _, _ = _time(lambda: op.run(), 3)
                rows.append((med, op.name, ops._describe_op(op)))
            tot = sum(r[0] for r in rows)
            for med, name, desc in sorted(rows, reverse=True)[:12]:
                print(f"    {med:9.3f} ms {100 * med / tot:5.1f} %  {name} {desc}")
        if not args.no_torch:
            with torch.no_grad():
                med, lo, hi = _time(lambda: decoder_ref(sd, vae.cfg, lat, torch.bfloat16), args.iters)
            print(f"{size}x{size} torch bf16 (tests/test_vae.py decoder_ref): {med:.3f} ({lo:.3f} .. {hi:.3f})")
    vae.release()


def main_encode(args):
    from test_vae_encoder import encoder_ref
    dev = torch.device("cuda:0")
    vae = model_util.load_vae("synthetic:sd15", encoder=True).to(dev)
    sd = {k: v.detach().to(dev, torch.bfloat16) for k, v in vae.state_dict().items()}
    print(f"# VAE encode, synthetic:sd15 encoder, batch 1, median (min .. max) of {args.iters} after one warm-up, ms")
    for size in args.sizes:
        img = torch.randint(0, 256, (1, size, size, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(dev)
        x = (img.float() / 127.5 - 1).permute(0, 3, 1, 2).contiguous()
        for graphs in (False, True):
            vae.release()
            vae.use_graphs = graphs
            vae.encode_to_latents(img)                # builds the plan (and captures)
            plan = vae.engine().encoder_plan(1, size, size, True, "sample")
            med, lo, hi = _time(lambda: vae._run(plan), args.iters)
            print(f"{size}x{size} hip plan {'graph' if graphs else 'eager'}: {med:.3f} ({lo:.3f} .. {hi:.3f})  "
                  f"launches {len(plan.ops)}  activation pool {plan.pool.nbytes() / 2 ** 20:.0f} MiB")
        if args.per_op:
            rows = []
            for op in plan.ops:
                med, _, _ = _time(lambda: op.run(), 3)
                rows.append((med, op.name, ops._describe_op(op)))
            tot = sum(r[0] for r in rows)
            for med, name, desc in sorted(rows, reverse=True)[:12]:
                print(f"    {med:9.3f} ms {100 * med / tot:5.1f} %  {name} {desc}")
        if not args.no_torch:
            with torch.no_grad():
                med, lo, hi = _time(lambda: encoder_ref(sd, vae.cfg, x, torch.bfloat16), args.iters)
            print(f"{size}x{size} torch bf16 (tests/test_vae_encoder.py encoder_ref): {med:.3f} ({lo:.3f} .. {hi:.3f})")
    vae.release()


if __name__ == "__main__":
    main()
