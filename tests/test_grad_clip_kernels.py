"""`leco_grad_clip` and `leco_grad_accumulate` (csrc/grad_clip.hip) on the host emulator (CPU tier) and on gfx950 (`-m gpu`).

Tolerance of the norm test, derived: the kernel accumulates exact double products (an fp32 times an fp32 is exact in
double, its square is rounded once) in double, so its error before the final rounding to fp32 is below n * 2^-53 relative,
far under half an fp32 ulp (2^-24).  `stats[0]`, `stats[1]` and the new `hyper[3]` must therefore each be within ONE fp32
ulp of the float64 value rounded to fp32."""
import math

import pytest
import torch

from leco_amd import hip, ops

GS = 0.5
SIZES = (1, 255, 100_003, 300_007)      # one thread, one partial block, 391 blocks (ticket path), 1 172 blocks


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


_GRADS = {}


def _grad(n, seed=41):
    """Seeded randn * 1e-3, computed once per (n, seed) and never modified."""
    key = (n, seed)
    if key not in _GRADS:
        _GRADS[key] = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 1e-3
    return _GRADS[key]


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def _reference(g, gs, max_norm):
    """float64: (norm, coef, new grad_scale) with clip_grad_norm_'s arithmetic; max_norm as the fp32 the ABI carries."""
    norm = torch.linalg.vector_norm(g.double() * gs).item()
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    return norm, coef, gs * coef


def _within_one_ulp(got: float, want64: float) -> bool:
    w = torch.tensor(want64, dtype=torch.float64).to(torch.float32)
    lo, hi = torch.nextafter(w, torch.tensor(-math.inf)), torch.nextafter(w, torch.tensor(math.inf))
    return lo.item() <= got <= hi.item()


def _run(dev, g, max_norm, gs=GS, hyper0=(1e-4, 0.1, 0.001)):
    hyper = torch.tensor([*hyper0, gs], dtype=torch.float32).to(dev)
    stats = torch.full((4,), -7.0).to(dev)
    ops.grad_clip(g.to(dev), hyper, max_norm, stats, g.numel()).run()
    _sync(dev)
    return hyper.cpu(), stats.cpu()


@pytest.mark.parametrize("n", SIZES)
def test_norm_and_coef_against_float64(dev, n):
    g = _grad(n)
    true_norm = torch.linalg.vector_norm(g.double() * GS).item()
    uploaded = torch.tensor([1e-4, 0.1, 0.001, GS], dtype=torch.float32)
    for what, max_norm in (("clips", _f32(0.5 * true_norm)), ("does not clip", _f32(2 * true_norm)), ("measure only", 0.0)):
        hyper, stats = _run(dev, g, max_norm)
        norm, coef, new_gs = _reference(g, GS, max_norm)
        print(f"grad_clip n={n} {what}: norm {stats[0].item():.9g} (float64 {norm:.12g}), coef {stats[1].item():.9g} "
              f"({coef:.12g}), hyper[3] {hyper[3].item():.9g} ({new_gs:.12g})")
        assert _within_one_ulp(stats[0].item(), norm), (what, stats[0].item(), norm)
        assert _within_one_ulp(stats[1].item(), coef), (what, stats[1].item(), coef)
        assert stats[2].item() == 0 and stats[3].item() == 0
        assert torch.equal(hyper[:3].view(torch.int32), uploaded[:3].view(torch.int32)), what
        if what == "clips":
            assert coef < 1 and _within_one_ulp(hyper[3].item(), new_gs), (hyper[3].item(), new_gs)
        else:
            assert stats[1].item() == 1.0
            assert torch.equal(hyper.view(torch.int32), uploaded.view(torch.int32)), what


def test_two_runs_are_bit_equal(dev):
    g = _grad(300_007)
    max_norm = _f32(0.5 * torch.linalg.vector_norm(g.double() * GS).item())
    (h1, s1), (h2, s2) = _run(dev, g, max_norm), _run(dev, g, max_norm)
    assert torch.equal(h1.view(torch.int32), h2.view(torch.int32)) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert s1[1].item() < 1


def test_back_to_back_launches_rearm_the_ticket(dev):
    """Three different slabs through the same per-device scratch in stream order, no host wait in between: each result is
    its single-launch result."""
    slabs = [_grad(100_003, seed=51), _grad(300_007, seed=52) * 3, _grad(255, seed=53)]
    max_norms = [_f32(0.25 * torch.linalg.vector_norm(s.double() * GS).item()) for s in slabs]
    alone = [_run(dev, s, mn) for s, mn in zip(slabs, max_norms)]
    on_dev = [s.to(dev) for s in slabs]
    hypers = [torch.tensor([1e-4, 0.1, 0.001, GS], dtype=torch.float32).to(dev) for _ in slabs]
    stats = [torch.full((4,), -7.0).to(dev) for _ in slabs]
    for s, h, st, mn in zip(on_dev, hypers, stats, max_norms):
        ops.grad_clip(s, h, mn, st, s.numel()).run()
    _sync(dev)
    for (h1, s1), h, st in zip(alone, hypers, stats):
        assert torch.equal(h1.view(torch.int32), h.cpu().view(torch.int32))
        assert torch.equal(s1.view(torch.int32), st.cpu().view(torch.int32))
        assert s1[1].item() < 1


def test_nonfinite_elements_are_counted_and_nothing_is_scaled(dev):
    g = _grad(100_003).clone()
    g[300] = float("nan")                 # block 1
    g[70_000] = float("inf")              # block 273
    uploaded = torch.tensor([1e-4, 0.1, 0.001, GS], dtype=torch.float32)
    for max_norm in (1e-3, 0.0):
        hyper, stats = _run(dev, g, max_norm)
        assert stats[2].item() == 2
        assert not math.isfinite(stats[0].item())
        assert torch.equal(hyper.view(torch.int32), uploaded.view(torch.int32))


@pytest.mark.parametrize("n", (1, 255, 100_003))
def test_accumulate(dev, n):
    G = 5
    a, b = _grad(n, seed=61), _grad(n, seed=62) * 7
    full = torch.full((n + 2 * G,), float("nan")).to(dev)       # the destination is NaN: `first` must not read it
    acc = full[G:G + n]
    ops.grad_accumulate(acc, a.to(dev), n, True).run()
    _sync(dev)
    got = full.cpu()
    assert torch.equal(got[G:G + n], a) and torch.isnan(got[:G]).all() and torch.isnan(got[G + n:]).all()
    ops.grad_accumulate(acc, b.to(dev), n, False).run()
    _sync(dev)
    got = full.cpu()
    assert torch.equal(got[G:G + n].view(torch.int32), (a + b).view(torch.int32))
    assert torch.isnan(got[:G]).all() and torch.isnan(got[G + n:]).all()


def test_bad_arguments_are_refused(dev):
    n = 64
    g = torch.ones(n).to(dev)
    hyper0, stats0 = torch.tensor([1e-4, 0.1, 0.001, GS]), torch.full((4,), -7.0)
    hyper, stats = hyper0.clone().to(dev), stats0.clone().to(dev)
    acc = torch.full((n,), 3.0).to(dev)
    bad = [lambda: ops.grad_clip(None, hyper, 1.0, stats, n), lambda: ops.grad_clip(g, hyper, 1.0, stats, 0),
           lambda: ops.grad_clip(g, hyper, -1.0, stats, n), lambda: ops.grad_clip(g, hyper, float("nan"), stats, n),
           lambda: ops.Op("leco_grad_clip", (ops.ptr(g), n, None, 1.0, ops.ptr(stats))),
           lambda: ops.Op("leco_grad_clip", (ops.ptr(g), n, ops.ptr(hyper), 1.0, None)),
           lambda: ops.grad_accumulate(None, g, n, True), lambda: ops.grad_accumulate(acc, None, n, False),
           lambda: ops.grad_accumulate(acc, g, 0, False)]
    for make in bad:
        with pytest.raises(hip.LecoError, match="leco_grad_"):
            make().run()
    _sync(dev)
    assert torch.equal(hyper.cpu(), hyper0) and torch.equal(stats.cpu(), stats0) and torch.equal(acc.cpu(), torch.full((n,), 3.0))
    with pytest.raises(ValueError, match="4 fp32"):
        ops.grad_clip(g, hyper[:2], 1.0, stats, n)
