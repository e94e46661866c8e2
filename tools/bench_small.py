"""Times a few small launches in isolation (HIP events over back-to-back repeats): conv_in / conv_out at the level-0 shape,
self-attention forward, the slab optimizers (leco_adamw / leco_prodigy from a replayed graph) and the gradient controls
(leco_grad_clip / leco_grad_accumulate beside leco_adamw).
    python tools/bench_small.py          (under `rocprofv3 --kernel-trace --stats` the kernel names show which path ran)
    python tools/bench_small.py optimizers          only that section (also: conv, attention, grad_controls)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from leco_amd import ops

dev = torch.device("cuda:0"); bf = torch.bfloat16


def timeit(op, n=200):
    for _ in range(20): op.run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): op.run()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def timeit_graph(op_list, inner, n=100):
    """us per pass over `op_list`, replayed from a captured graph that holds `inner` passes."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for op in op_list: op.run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            for op in op_list: op.run()
    for _ in range(5): graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): graph.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (n * inner)


def bench_conv():
    for B in (2, 4, 12):
        H = W = 64; C = 320
        x = torch.randn(B, H, W, C, device=dev).to(bf); w = (torch.randn(4, 3, 3, C, device=dev) * 0.05).to(bf); b4 = torch.randn(4, device=dev)
        y = torch.zeros(B, 4, H, W, device=dev)
        print(f"conv_out B={B}: {timeit(ops.conv_out(x, w, b4, y, B, H, W, C, 4)):.1f} us")
        xi = torch.randn(B, 4, H, W, device=dev).to(bf); wi = torch.randn(4, 3, 3, C, device=dev) * 0.2; bi = torch.randn(C, device=dev)
        yi = torch.zeros(B, H, W, C, device=dev, dtype=bf)
        print(f"conv_in  B={B}: {timeit(ops.conv_in(xi, wi, bi, yi, B, H, W, 4, C)):.1f} us")


def bench_attention():
    """self-attention forward: register-staged (LECO_ATTN_DMA=0) vs LDS-DMA staged kernels, q|k|v fused layout as the planner's"""
    print("attention fwd  B  H     S   d   staged us   dma us")
    for (B, H, S, D) in [(4, 8, 4096, 40), (2, 8, 4096, 40), (12, 8, 4096, 40), (4, 8, 1024, 80), (12, 8, 1024, 80), (4, 5, 9216, 64),
                         (4, 10, 2304, 64), (2, 10, 4096, 64), (2, 20, 1024, 64), (4, 20, 576, 64)]:
        C = H * D
        qkv = torch.randn(B, S, 3 * C, device=dev).to(bf)
        o = torch.zeros(B, S, C, device=dev, dtype=bf); lse = torch.zeros(B, H, S, device=dev)
        p0 = qkv.data_ptr()
        op = ops.attention_fwd(p0, 3 * C, S * 3 * C, p0 + 2 * C, 3 * C, S * 3 * C, p0 + 4 * C, 3 * C, S * 3 * C, o.data_ptr(), C, S * C, lse, B, H, S, S, D, D ** -0.5)
        ts = []
        for mode in ("0", "1"):
            os.environ["LECO_ATTN_DMA"] = mode
            ts.append(timeit(op, 50))
        fl = 4.0 * B * H * S * S * D
        print(f"              {B:2d} {H:2d} {S:5d} {D:3d}   {ts[0]:8.1f}  {ts[1]:8.1f}   ({fl / ts[0] / 1e6:.0f} -> {fl / ts[1] / 1e6:.0f} TFLOP/s)")


def bench_optimizers():
    """Slab optimizers at the SD1.5 rank-4 and SDXL rank-16 LoRA slab sizes, one step per graph replay and 8 steps per replay
    (the second divides the replay overhead by 8).  Bytes per element: AdamW reads p g m v, writes p m v + the bf16 shadow =
    30; Prodigy's first launch reads p g m v s p0 and writes m v s = 36, its second reads p m v and writes p + shadow = 18.
    (d_coef = 1e-30 pins d at d0: the same memory traffic, and a constant random gradient cannot run the estimate to inf.)"""
    print("optimizer       floats   us/step (graph of 1)   us/step (graph of 8)   bytes/elt   TB/s (graph of 8)   of 8 TB/s")
    for n in (1_695_744, 42_557_440):
        p = torch.randn(n, device=dev) * 0.05; g = torch.randn(n, device=dev) * 1e-3
        m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev); sh = torch.zeros(n, device=dev, dtype=bf)
        s_ = torch.zeros(n, device=dev); p0 = p.clone()
        hyper = torch.tensor([1e-4, 0.1, 0.001, 1.0], device=dev)
        hyper_p = torch.tensor([1.0, 0.0, 0.0, 1.0], device=dev)
        state = ops.prodigy_state(1e-6, dev)
        rows = (("leco_adamw", [ops.adamw(p, g, m, v, sh, hyper, 0.9, 0.999, 1e-8, 1e-2, n)], 30),
                ("leco_prodigy", [ops.prodigy(p, g, m, v, s_, p0, sh, hyper_p, state, 0.9, 0.999, 0.999 ** 0.5, 1e-8, 0.0, 1e-30,
                                              float("inf"), True, False, False, n)], 54))
        for name, op_list, bpe in rows:
            t1, t8 = timeit_graph(op_list, 1), timeit_graph(op_list, 8)
            tbs = n * bpe / t8 / 1e6
            print(f"{name:13s} {n:9d}   {t1:10.1f}             {t8:10.1f}             {bpe:3d}         {tbs:6.2f}             {tbs / 8 * 100:4.0f} %")
        assert torch.isfinite(p).all()


def slab_numel(kind, rank, c3lier):
    """Floats in the LoRA slab of a BASELINE config: `net.slab.numel()` of its network, from a shape-only (meta) instance."""
    import contextlib, io
    from leco_amd import model_util
    from leco_amd.lora import DEFAULT_TARGET_REPLACE, UNET_TARGET_REPLACE_MODULE_CONV, LoRANetwork
    from leco_amd.unet import UNet2DConditionModel
    with torch.device("meta"), contextlib.redirect_stdout(io.StringIO()):
        net = LoRANetwork(UNet2DConditionModel(model_util.SYNTHETIC[kind]()), rank=rank,
                          target_replace_modules=list(DEFAULT_TARGET_REPLACE) + (UNET_TARGET_REPLACE_MODULE_CONV if c3lier else []))
    return net.numel + (-net.numel) % 64          # the slab is padded to 64 floats (LoRANetwork._build_slab)


def bench_grad_controls():
    """leco_grad_clip (reads g: 4 B/element; max_norm = 1.0 against a norm of ~1.3 / ~7: it clips) and leco_grad_accumulate
    (first = 0: reads acc and g, writes acc = 12 B/element) beside leco_adamw (30 B/element) at the slab sizes of the SD1.5
    rank-4 lierla and the SDXL rank-16 c3lier configs, one launch and 8 launches per graph replay."""
    print("launch                  floats   us (graph of 1)   us (graph of 8)   bytes/elt   TB/s (graph of 8)")
    for kind, rank, c3 in (("sd15", 4, False), ("sdxl", 16, True)):
        n = slab_numel(kind, rank, c3)
        p = torch.randn(n, device=dev) * 0.05; g = torch.randn(n, device=dev) * 1e-3; acc = torch.zeros(n, device=dev)
        m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev); sh = torch.zeros(n, device=dev, dtype=bf)
        hyper = torch.tensor([1e-4, 0.1, 0.001, 1.0], device=dev); stats = torch.zeros(4, device=dev)
        # (every clipping launch multiplies hyper[3] once more; the traffic does not depend on it)
        rows = (("leco_adamw", [ops.adamw(p, g, m, v, sh, hyper, 0.9, 0.999, 1e-8, 1e-2, n)], 30),
                ("leco_grad_clip", [ops.grad_clip(g, hyper, 1.0, stats, n)], 4),
                ("leco_grad_accumulate", [ops.grad_accumulate(acc, g, n, False)], 12))
        for name, op_list, bpe in rows:
            t1, t8 = timeit_graph(op_list, 1), timeit_graph(op_list, 8)
            print(f"{name:21s} {n:9d}   {t1:10.1f}        {t8:10.1f}        {bpe:3d}         {n * bpe / t8 / 1e6:6.2f}")
        print(f"  grad_stats {dict(zip(ops.GRAD_STATS_FIELDS, stats.cpu().tolist()))}")


SECTIONS = {"conv": bench_conv, "attention": bench_attention, "optimizers": bench_optimizers, "grad_controls": bench_grad_controls}
for name in sys.argv[1:] or list(SECTIONS):
    SECTIONS[name]()
