#!/usr/bin/env python
"""Measurement only: the native CLIP text encoder (leco_amd/clip.py) replayed from its hipGraph, beside torch-bf16 eager
running the plain PyTorch restatement the tests use (tests/test_clip.py `clip_ref`) on the same weights, in the same run.
Shapes: CLIP-L (12 layers), OpenCLIP-H (23 layers, what SD2.x uses), OpenCLIP-bigG (32 layers, with the projection), 77
tokens, seeded random weights (vocabulary cut to 4096 rows so that initialisation stays cheap; no other shape changes).
With --per-op the plan is also timed launch by launch, summed per kind of launch.

    python tools/bench_clip.py [--models clip_l open_clip_h bigg] [--batches 1 2 8] [--iters 20] [--per-op] > profiles/clip_text_encoder.txt
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from leco_amd import clip as CL  # noqa: E402
from tools.timing import print_per_op, time_ms  # noqa: E402

MODELS = {"clip_l": (CL.clip_l_config, False), "open_clip_h": (CL.open_clip_h_config, False), "bigg": (CL.open_clip_bigg_config, True)}
VOCAB = 4096


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--per-op", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args(argv)
    from test_clip import clip_ref
    dev = torch.device("cuda:0")
    print(f"# CLIP text encoder, 77 tokens, median (min .. max) of {args.iters} after two warm-ups, ms; device: "
          f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    for name in args.models:
        mk, projection = MODELS[name]
        cfg = mk(vocab_size=VOCAB, eos_token_id=VOCAB - 1, bos_token_id=VOCAB - 2)
        model = CL.init_synthetic_clip_((CL.CLIPTextModelWithProjection if projection else CL.CLIPTextModel)(cfg)).to(dev, torch.bfloat16)
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        for B in args.batches:
            ids = torch.randint(3, VOCAB - 2, (B, 77), generator=torch.Generator().manual_seed(B))
            ids[:, 0], ids[:, 20] = VOCAB - 2, VOCAB - 1
            line = f"{name} ({cfg.hidden_size} wide, {cfg.num_hidden_layers} layers) B={B}:"
            plan = None
            for graphs in (True, False):
                model.release()
                model.use_graphs = graphs
                model(ids)                               # builds the plan (and captures)
                plan = model.engine().plan(B, 77)
                med, lo, hi = time_ms(lambda: model._run(plan), args.iters)
                line += f"  native {'graph' if graphs else 'eager'} {med:.3f} ({lo:.3f} .. {hi:.3f})"
            line += f"  launches {len(plan.ops)}"
            if not args.no_torch:
                idd = ids.to(dev)
                with torch.no_grad():
                    med, lo, hi = time_ms(lambda: clip_ref(sd, cfg, idd, torch.bfloat16), args.iters)
                line += f"  torch bf16 eager {med:.3f} ({lo:.3f} .. {hi:.3f})"
            print(line, flush=True)
            if args.per_op:
                print_per_op(plan)
        model.release()
        del model, sd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
