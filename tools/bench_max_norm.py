"""Times `leco_lora_max_norm` (max-norm regularisation of the LoRA weights, train.scale_weight_norms) as graph replays on
the slabs of three configurations -- SD1.5 rank-4 lierla, SDXL rank-16 c3lier, SDXL rank-128 c3lier (does one workgroup per
module leave a single workgroup running for milliseconds?) -- once measure-only and once with a bound at the median module
norm (about half the modules are scaled; the graph restores the slab first, and that copy is timed alone and subtracted),
beside `leco_adamw` and `leco_grad_clip` on the same slab and the eager torch statement of the same regularisation (a Python
loop over the modules: matmul, norm, host decision, two multiplies).  Measurement only.
    python tools/bench_max_norm.py"""
import contextlib
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from leco_amd import model_util, ops
from leco_amd.lora import DEFAULT_TARGET_REPLACE, UNET_TARGET_REPLACE_MODULE_CONV, LoRANetwork
from leco_amd.unet import UNet2DConditionModel

dev = torch.device("cuda:0")


def module_rows(kind, rank, c3lier):
    """Table rows (down_off, up_off, r, K, N, scale) of a BASELINE config's network, from a shape-only (meta) instance."""
    with torch.device("meta"), contextlib.redirect_stdout(io.StringIO()):
        net = LoRANetwork(UNet2DConditionModel(model_util.SYNTHETIC[kind]()), rank=rank,
                          target_replace_modules=list(DEFAULT_TARGET_REPLACE) + (UNET_TARGET_REPLACE_MODULE_CONV if c3lier else []))
    rows = []
    for l in net.unet_loras:
        dn, up = l.lora_down.weight, l.lora_up.weight
        rows.append((l.down_off, l.up_off, dn.shape[0], dn.numel() // dn.shape[0], up.shape[0], l.scale))
    return rows, net.numel + (-net.numel) % 64


def replay_us(fn, n=50):
    """us per replay of a graph that holds one call of `fn`."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def eager_torch_ms(slab, rows, bound):
    """The per-module loop a framework trainer runs: one host decision per module."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scaled = 0
    for off, up_off, r, K, N, scale in rows:
        D, U = slab[off:off + r * K].view(r, K), slab[up_off:up_off + N * r].view(N, r)
        norm = (scale * (U @ D)).norm()
        if norm.item() > bound:
            f = (bound / norm) ** 0.5
            D.mul_(f)
            U.mul_(f)
            scaled += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, scaled


def main():
    print("slab                      modules      floats | measure us | restore us  restore+scale us  -> scale us (scaled) | "
          "adamw us  grad_clip us | eager torch loop ms (scaled)")
    for label, kind, rank, c3 in (("sd15 r4 lierla", "sd15", 4, False), ("sdxl r16 c3lier", "sdxl", 16, True),
                                  ("sdxl r128 c3lier", "sdxl", 128, True)):
        rows, n = module_rows(kind, rank, c3)
        M = len(rows)
        slab0 = torch.randn(n, device=dev) * 0.05
        slab, shadow = slab0.clone(), slab0.to(torch.bfloat16)
        table = ops.lora_norm_table(rows, dev)
        norms, factors, stats = torch.zeros(M, device=dev), torch.ones(M, device=dev), torch.zeros(4, device=dev)
        measure = ops.lora_max_norm(slab, shadow, table, 0.0, norms, factors, stats)
        measure.run()
        torch.cuda.synchronize()
        bound = float(norms.median())
        scale = ops.lora_max_norm(slab, shadow, table, bound, norms, factors, stats)
        t_measure = replay_us(measure.run)
        t_restore = replay_us(lambda: slab.copy_(slab0))
        t_both = replay_us(lambda: (slab.copy_(slab0), scale.run()))
        k = int(stats[0].item())
        g = torch.randn(n, device=dev) * 1e-3
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        hyper, gstats = torch.tensor([1e-4, 0.1, 0.001, 1.0], device=dev), torch.zeros(4, device=dev)
        p = slab0.clone()
        t_adamw = replay_us(ops.adamw(p, g, m, v, shadow, hyper, 0.9, 0.999, 1e-8, 1e-2, n).run)
        t_clip = replay_us(ops.grad_clip(g, hyper, 0.0, gstats, n).run)
        eager = slab0.clone()
        eager_torch_ms(eager, rows[:8], bound)                     # warm-up of the matmul / norm kernels
        eager.copy_(slab0)
        t_eager, k_eager = eager_torch_ms(eager, rows, bound)
        print(f"{label:24s} {M:8d} {n:11d} | {t_measure:10.1f} | {t_restore:10.1f}  {t_both:16.1f}  -> {t_both - t_restore:8.1f} ({k:4d}) | "
              f"{t_adamw:8.1f}  {t_clip:12.1f} | {t_eager:8.1f} ({k_eager})", flush=True)


if __name__ == "__main__":
    main()
