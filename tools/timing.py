"""What the bench_clip*.py tools share: event timing of a callable and the per-kind sums of a plan's launches."""
import torch


def time_ms(fn, iters):
    """(median, min, max) milliseconds of ``iters`` calls, each between two events, after two warm-ups."""
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


def print_per_op(plan):
    """The plan launched one op at a time (median of 5), summed per label of ``plan.names``, largest first."""
    kinds = {}
    for label, op in zip(plan.names, plan.ops):
        med, _, _ = time_ms(op.run, 5)
        t, n = kinds.get(label, (0.0, 0))
        kinds[label] = (t + med, n + 1)
    tot = sum(t for t, _ in kinds.values())
    for label, (t, n) in sorted(kinds.items(), key=lambda kv: -kv[1][0]):
        print(f"    {t:8.3f} ms {100 * t / tot:5.1f} %  {label} x {n}  ({1e3 * t / n:.1f} us each, launched one at a time)")
