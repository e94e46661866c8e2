"""`leco_lora_max_norm` (csrc/lora_norm.hip) on the host emulator (CPU tier) and on gfx950 (`-m gpu`).

Reference: float64 torch, `(scale * U.double() @ D.double().flatten(1)).norm()` per module, with `scale` the fp32 value the
table carries.

Tolerance, derived: the kernel forms |U D|_F^2 = sum_ij (U^T U)_ij (D D^T)_ij from exact double products of fp32 values, so
its error before the final rounding is about (K + N) * 2^-53 * kappa with kappa = sum|U^T U o D D^T| / |U D|_F^2.  The tests
compute kappa in float64 for every module and assert kappa < 1e4 on their inputs (seeded randn gives kappa of the order of
r): with K + N < 2^10 that leaves a relative error below 2^-29, far under half an fp32 ulp (2^-24).  `norms[m]`,
`factors[m]`, `stats[1]` and `stats[2]` must therefore each be within ONE fp32 ulp of the float64 value rounded to fp32."""
import math

import pytest
import torch

from leco_amd import hip, ops

G = 5                # guard words in front of and behind the slab and the shadow (odd: the slab itself is only 4-byte aligned)
MAX_NORM = 1.0
# (name, r, K, N): K = the row length of lora_down (in * kh * kw for the convolution), N = out.  After the second module every
# offset is odd.  `pad` floats of padding follow each module.
MIXED = (("linear", 4, 320, 320), ("rank1", 1, 5, 3), ("conv3x3", 4, 8 * 9, 12), ("rank64", 64, 64, 70), ("rank96", 96, 128, 96),
         ("up_zero", 4, 40, 24), ("rank8", 8, 33, 21), ("rank20", 20, 150, 37))
MANY = tuple((f"small{i}", 2, 16, 16) for i in range(300))         # cross-module statistics past one block's worth


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def _within_one_ulp(got: float, want64: float) -> bool:
    w = torch.tensor(want64, dtype=torch.float64).to(torch.float32)
    lo, hi = torch.nextafter(w, torch.tensor(-math.inf)), torch.nextafter(w, torch.tensor(math.inf))
    return lo.item() <= got <= hi.item()


def _norm64(scale, U, D):
    return (scale * U.double() @ D.double().flatten(1)).norm().item()


def _kappa(U, D):
    U, D = U.double(), D.double().flatten(1)
    return ((U.T @ U) * (D @ D.T)).abs().sum().item() / (U @ D).norm().item() ** 2


_CASES = {}


def _case(which, seed=71):
    """A hand-built slab and table, computed once per (case, seed) and never modified: dict(slab [n] fp32, shadow [n] bf16
    (NOT the image of the slab: a rewritten element shows), rows (table rows), mods [(scale, down slice, up slice, D shape, U
    shape)], norm64 [M]).  The norms alternate between about 2 MAX_NORM and MAX_NORM / 2; `up_zero` has norm 0."""
    key = (which, seed)
    if key in _CASES:
        return _CASES[key]
    gen = torch.Generator().manual_seed(seed)
    spec = MIXED if which == "mixed" else MANY
    parts, rows, mods, off = [], [], [], 0
    for idx, (name, r, K, N) in enumerate(spec):
        scale = _f32(1.0 / r)                                       # alpha = 1, as the fp32 the table carries
        D = torch.randn(r, K, generator=gen) * 0.05
        U = torch.randn(N, r, generator=gen) * 0.05
        if name == "up_zero":
            U.zero_()
        else:
            U *= (2.0 if idx % 2 == 0 else 0.5) * MAX_NORM / _norm64(scale, U, D)
            assert _kappa(U, D) < 1e4, (name, _kappa(U, D))
        pad = 3 if which == "mixed" else idx % 3
        rows.append((off, off + r * K, r, K, N, scale))
        mods.append((scale, slice(off, off + r * K), slice(off + r * K, off + r * K + N * r), (r, K), (N, r)))
        parts += [D.reshape(-1), U.reshape(-1), torch.randn(pad, generator=gen)]
        off += r * K + N * r + pad
    slab = torch.cat(parts + [torch.randn(7, generator=gen)])       # padding after the last module too
    shadow = torch.randn(slab.numel(), generator=gen).to(torch.bfloat16)
    norm64 = [_norm64(s, slab[us].view(ush), slab[ds].view(dsh)) for s, ds, us, dsh, ush in mods]
    for v in norm64:                                                # no decision hangs on the last bit
        assert abs(v - MAX_NORM) > 1e-3 * MAX_NORM, v
    assert any(v > MAX_NORM for v in norm64) and any(v < MAX_NORM for v in norm64)
    _CASES[key] = dict(slab=slab, shadow=shadow, rows=rows, mods=mods, norm64=norm64)
    return _CASES[key]


class _Dev:
    """The case's buffers on the device, each between two runs of G guard words."""

    def __init__(self, dev, case, slab=None):
        slab = case["slab"] if slab is None else slab
        n, M = slab.numel(), len(case["rows"])
        self.n, self.M = n, M
        self.slab_full = torch.cat([torch.full((G,), 7.25), slab, torch.full((G,), 7.25)]).to(dev)
        self.shadow_full = torch.cat([torch.full((G,), 3.5).to(torch.bfloat16), case["shadow"], torch.full((G,), 3.5).to(torch.bfloat16)]).to(dev)
        self.out_full = torch.full((2 * M + 4 + 4 * G,), -7.0).to(dev)          # norms | factors | stats, guards around each
        self.slab, self.shadow = self.slab_full[G:G + n], self.shadow_full[G:G + n]
        self.norms = self.out_full[G:G + M]
        self.factors = self.out_full[2 * G + M:2 * G + 2 * M]
        self.stats = self.out_full[3 * G + 2 * M:3 * G + 2 * M + 4]
        self.table = ops.lora_norm_table(case["rows"], dev)

    def op(self, max_norm):
        return ops.lora_max_norm(self.slab, self.shadow, self.table, max_norm, self.norms, self.factors, self.stats)

    def guards_intact(self):
        s, h, o, M, n = self.slab_full.cpu(), self.shadow_full.cpu().float(), self.out_full.cpu(), self.M, self.n
        return bool((s[:G] == 7.25).all() and (s[G + n:] == 7.25).all() and (h[:G] == 3.5).all() and (h[G + n:] == 3.5).all()
                    and (o[:G] == -7).all() and (o[G + M:2 * G + M] == -7).all() and (o[2 * G + 2 * M:3 * G + 2 * M] == -7).all()
                    and (o[3 * G + 2 * M + 4:] == -7).all())

    def results(self):
        return [t.cpu().clone() for t in (self.slab, self.shadow, self.norms, self.factors, self.stats)]


def _run(dev, case, max_norm, slab=None):
    d = _Dev(dev, case, slab)
    d.op(max_norm).run()
    _sync(dev)
    assert d.guards_intact()
    return d


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _expected(case, max_norm):
    """float64: (post-scaling norms, ratios) of the rule."""
    ratios = [1.0 if (max_norm == 0 or v <= max_norm) else max_norm / v for v in case["norm64"]]
    return [v * q for v, q in zip(case["norm64"], ratios)], ratios


@pytest.mark.parametrize("which", ["mixed", "many"])
def test_norms_factors_and_stats_against_float64(dev, which):
    case = _case(which)
    slab, shadow, norms, factors, stats = _run(dev, case, MAX_NORM).results()
    post, ratios = _expected(case, MAX_NORM)
    for m, (want, ratio) in enumerate(zip(case["norm64"], ratios)):
        if m < 8:
            print(f"lora_max_norm {which}[{m}]: norm {norms[m].item():.9g} (float64 {want:.12g}), factor {factors[m].item():.9g} "
                  f"({math.sqrt(ratio):.12g})")
        assert _within_one_ulp(norms[m].item(), want), (m, norms[m].item(), want)
        if ratio == 1.0:
            assert factors[m].item() == 1.0, m
        else:
            assert factors[m].item() < 1.0 and _within_one_ulp(factors[m].item(), math.sqrt(ratio)), (m, factors[m].item(), ratio)
    n_scaled = sum(q < 1 for q in ratios)
    print(f"lora_max_norm {which}: stats {stats.tolist()} (float64: {n_scaled} scaled, mean {sum(post) / len(post):.12g}, max {max(post):.12g})")
    assert 0 < n_scaled < len(ratios)
    assert stats[0].item() == n_scaled and stats[3].item() == 0
    assert _within_one_ulp(stats[1].item(), sum(post) / len(post)), (stats[1].item(), sum(post) / len(post))
    assert _within_one_ulp(stats[2].item(), max(post)), (stats[2].item(), max(post))
    if which == "mixed":
        assert norms[5].item() == 0.0 and factors[5].item() == 1.0          # lora_up = 0: norm 0, ratio 1


@pytest.mark.parametrize("which", ["mixed", "many"])
def test_scaled_modules_are_one_multiply_and_the_rest_is_untouched(dev, which):
    case = _case(which)
    slab, shadow, norms, factors, stats = _run(dev, case, MAX_NORM).results()
    old, old_shadow = case["slab"], case["shadow"]
    want, want_shadow = old.clone(), old_shadow.clone()
    for m, (scale, ds, us, _, _) in enumerate(case["mods"]):
        if case["norm64"][m] > MAX_NORM:
            for sl in (ds, us):
                want[sl] = old[sl] * factors[m]                    # one fp32 multiply by the factor the kernel reports
                want_shadow[sl] = want[sl].to(torch.bfloat16)
            assert not torch.equal(want[ds], old[ds])
    # everything else -- unscaled modules, the padding between and after the modules -- keeps its bits, in slab and shadow
    assert torch.equal(_bits(slab), _bits(want))
    assert torch.equal(_bits(shadow), _bits(want_shadow))


def test_a_second_launch_measures_every_norm_inside_the_bound(dev):
    case = _case("mixed")
    d = _run(dev, case, MAX_NORM)
    scaled_slab, scaled_shadow = d.slab.cpu().clone(), d.shadow.cpu().clone()
    d.op(0.0).run()
    _sync(dev)
    _, _, norms, factors, stats = d.results()
    bound = MAX_NORM * (1 + 4 * 2.0 ** -24)                        # two fp32 roundings of the factor, squared
    assert (norms <= bound).all(), norms.max().item()
    assert stats[0].item() == 0 and stats[3].item() == 0 and (factors == 1.0).all()
    assert stats[2].item() <= bound and stats[2].item() > 0.99 * MAX_NORM
    assert torch.equal(_bits(d.slab.cpu()), _bits(scaled_slab)) and torch.equal(_bits(d.shadow.cpu()), _bits(scaled_shadow))
    d.op(MAX_NORM * (1 + 8 * 2.0 ** -24)).run()                    # a bound just above: still nothing to scale
    _sync(dev)
    assert d.stats.cpu()[0].item() == 0 and torch.equal(_bits(d.slab.cpu()), _bits(scaled_slab))
    assert d.guards_intact()


def test_max_norm_zero_measures_only(dev):
    case = _case("mixed")
    slab, shadow, norms, factors, stats = _run(dev, case, 0.0).results()
    assert torch.equal(_bits(slab), _bits(case["slab"])) and torch.equal(_bits(shadow), _bits(case["shadow"]))
    assert (factors == 1.0).all() and stats[0].item() == 0 and stats[3].item() == 0
    for m, want in enumerate(case["norm64"]):
        assert _within_one_ulp(norms[m].item(), want)
    assert _within_one_ulp(stats[1].item(), sum(case["norm64"]) / len(case["norm64"]))
    assert _within_one_ulp(stats[2].item(), max(case["norm64"]))


def test_a_nan_module_is_left_alone_and_counted(dev):
    case = _case("mixed")
    clean = _run(dev, case, MAX_NORM).results()
    assert case["norm64"][0] > MAX_NORM                             # module 0 is scaled in the clean run
    bad = case["slab"].clone()
    ds, us = case["mods"][0][1], case["mods"][0][2]
    bad[ds.start + 17] = float("nan")
    slab, shadow, norms, factors, stats = _run(dev, case, MAX_NORM, slab=bad).results()
    assert math.isnan(norms[0].item()) and factors[0].item() == 1.0
    assert stats[3].item() == 1 and stats[0].item() == clean[4][0].item() - 1
    for sl in (ds, us):                                             # untouched, slab and shadow
        assert torch.equal(_bits(slab[sl]), _bits(bad[sl])) and torch.equal(_bits(shadow[sl]), _bits(case["shadow"][sl]))
    rest = slice(us.stop, None)                                     # every other module: as in the clean run
    assert torch.equal(_bits(slab[rest]), _bits(clean[0][rest])) and torch.equal(_bits(shadow[rest]), _bits(clean[1][rest]))
    assert torch.equal(_bits(norms[1:]), _bits(clean[2][1:])) and torch.equal(_bits(factors[1:]), _bits(clean[3][1:]))
    post, _ = _expected(case, MAX_NORM)                             # mean and maximum run over the finite modules
    assert _within_one_ulp(stats[1].item(), sum(post[1:]) / len(post[1:])) and _within_one_ulp(stats[2].item(), max(post[1:]))


def test_a_table_row_outside_the_slab_is_not_followed(dev):
    case = _case("mixed")
    rows = list(case["rows"])
    off, up, r, K, N, scale = rows[2]
    rows[2] = (off, case["slab"].numel() - 3, r, K, N, scale)      # lora_up would end past the slab
    wrong = dict(case, rows=rows)
    clean = _run(dev, case, MAX_NORM).results()
    slab, shadow, norms, factors, stats = _run(dev, wrong, MAX_NORM).results()
    assert math.isnan(norms[2].item()) and factors[2].item() == 1.0 and stats[3].item() == 1
    ds, us = case["mods"][2][1], case["mods"][2][2]
    assert torch.equal(_bits(slab[ds.start:us.stop]), _bits(case["slab"][ds.start:us.stop]))
    assert torch.equal(_bits(slab[us.stop:]), _bits(clean[0][us.stop:])) and torch.equal(_bits(slab[:ds.start]), _bits(clean[0][:ds.start]))


def test_two_runs_are_bit_equal(dev):
    case = _case("many")
    a, b = _run(dev, case, MAX_NORM).results(), _run(dev, case, MAX_NORM).results()
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))
    assert a[4][0].item() > 0


def test_back_to_back_launches_rearm_the_ticket(dev):
    """Three different slabs through the same per-device scratch in stream order, no host wait in between: each result is
    its single-launch result."""
    cases = [_case("many", seed=81), _case("mixed", seed=82), _case("many", seed=83)]
    bounds = [MAX_NORM, 0.0, MAX_NORM]
    alone = [_run(dev, c, mn).results() for c, mn in zip(cases, bounds)]
    devs = [_Dev(dev, c) for c in cases]
    for d, mn in zip(devs, bounds):
        d.op(mn).run()
    _sync(dev)
    for single, d in zip(alone, devs):
        for x, y in zip(single, d.results()):
            assert torch.equal(_bits(x), _bits(y))
        assert d.guards_intact()


def test_bad_arguments_are_refused(dev):
    case = _case("mixed")
    d = _Dev(dev, case)
    before = [t.clone() for t in (d.slab_full.cpu(), d.shadow_full.cpu(), d.out_full.cpu())]
    good = (ops.ptr(d.slab), ops.ptr(d.shadow), d.n, ops.ptr(d.table), d.M, 1.0, ops.ptr(d.norms), ops.ptr(d.factors), ops.ptr(d.stats))

    def having(i, v):
        return lambda: ops.Op("leco_lora_max_norm", good[:i] + (v,) + good[i + 1:])
    bad = [having(i, None) for i in (0, 1, 3, 6, 7, 8)] + [having(2, 0), having(4, 0), having(4, -3), having(4, 1 << 20),
                                                          having(5, -1.0), having(5, float("nan"))]
    for make in bad:
        with pytest.raises(hip.LecoError, match="leco_lora_max_norm"):
            make().run()
    _sync(dev)
    for b, t in zip(before, (d.slab_full.cpu(), d.shadow_full.cpu(), d.out_full.cpu())):
        assert torch.equal(b, t)
    with pytest.raises(ValueError, match="fp32"):
        ops.lora_max_norm(d.slab, d.shadow, d.table, 1.0, d.norms[:2], d.factors, d.stats)
    with pytest.raises(ValueError, match="bf16"):
        ops.lora_max_norm(d.slab, d.slab, d.table, 1.0, d.norms, d.factors, d.stats)
