"""The slab-native Prodigy optimizer (`leco_prodigy`, `FusedStep(optimizer="prodigy")`, `train.optimizer: prodigy`) on the
host emulator (CPU tier) and on gfx950 (`-m gpu`).

Reference: `prodigyopt.Prodigy` when it imports; otherwise `ProdigyRef` below, a `torch.optim.Optimizer` restatement of the
published algorithm (Mishchenko & Defazio 2023, prodigyopt 1.0) that runs in the dtype of its parameters.

Tolerance: nothing is invented.  The restatement is run twice on the same inputs, on float64 and on float32 tensors; the
distance between the two is what fp32 state costs, and the kernel (fp32 state too, other summation order) must stay within
4 x that distance of the float64 run -- per compared quantity, relative L2 (relative difference for the scalars)."""
import contextlib
import io
import math
import os

import pytest
import torch
from safetensors.torch import load_file

from leco_amd import model_util, ops, prompt_util
from leco_amd.lora import LoRANetwork
from leco_amd.scheduler import create_noise_scheduler
from leco_amd.train import FusedStep
from leco_amd.unet import UNet2DConditionModel

bf = torch.bfloat16
GOLD = load_file(os.path.join(os.path.dirname(__file__), "golden", "tiny_step.safetensors"))
N_STEPS = 10
MARGIN = 4.0                     # the issue's: summation order legitimately differs


class ProdigyRef(torch.optim.Optimizer):
    """Prodigy as released in prodigyopt 1.0 (one global d over all param groups' tensors; the scalars are Python floats)."""

    def __init__(self, params, lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True,
                 use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf")):
        super().__init__(params, dict(lr=lr, betas=betas, beta3=beta3, eps=eps, weight_decay=weight_decay, decouple=decouple,
                                      use_bias_correction=use_bias_correction, safeguard_warmup=safeguard_warmup, d=d0, d0=d0,
                                      d_max=d0, d_numerator=0.0, d_denom=0.0, d_hat=d0, d_coef=d_coef, growth_rate=growth_rate,
                                      k=0))

    @torch.no_grad()
    def step(self, closure=None):
        g0 = self.param_groups[0]
        beta1, beta2 = g0["betas"]
        beta3 = g0["beta3"] if g0["beta3"] is not None else math.sqrt(beta2)
        k, d, d0, d_max, lr = g0["k"], g0["d"], g0["d0"], g0["d_max"], g0["lr"]
        bc = (math.sqrt(1 - beta2 ** (k + 1)) / (1 - beta1 ** (k + 1))) if g0["use_bias_correction"] else 1.0
        dlr = d * lr * bc
        num, den = g0["d_numerator"], 0.0
        if lr > 0:
            num *= beta3
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if group["weight_decay"] != 0 and not group["decouple"]:
                    g = g + group["weight_decay"] * p
                st = self.state[p]
                if "s" not in st:
                    st["s"], st["p0"] = torch.zeros_like(p), p.detach().clone()
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                if lr > 0:
                    num += (d / d0) * dlr * torch.dot(g.flatten(), (st["p0"] - p).flatten()).item()
                    st["exp_avg"].mul_(beta1).add_(g, alpha=d * (1 - beta1))
                    st["exp_avg_sq"].mul_(beta2).addcmul_(g, g, value=d * d * (1 - beta2))
                    st["s"].mul_(beta3).add_(g, alpha=(d / d0) * (d if group["safeguard_warmup"] else dlr))
                    den += st["s"].abs().sum().item()
        for group in self.param_groups:
            group["d_numerator"], group["d_denom"], group["dlr"] = num, den, dlr
        if den == 0:
            return None
        if lr > 0:
            d_hat = g0["d_coef"] * num / den
            if d == d0:
                d = max(d, d_hat)
            d_max = max(d_max, d_hat)
            d = min(d_max, d * g0["growth_rate"])
            for group in self.param_groups:
                group["d_hat"] = d_hat
        for group in self.param_groups:
            group["d"], group["d_max"], group["k"] = d, d_max, k + 1
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if group["weight_decay"] != 0 and group["decouple"]:
                    p.mul_(1 - group["weight_decay"] * dlr)
                p.addcdiv_(st["exp_avg"], st["exp_avg_sq"].sqrt().add_(d * group["eps"]), value=-dlr)
        return None


def reference_cls():
    try:
        from prodigyopt import Prodigy
        return Prodigy
    except ImportError:
        return ProdigyRef


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def run_reference(dtype, p_init, grads, lrs, kw, gs=1.0):
    """The reference on ONE flat tensor of `dtype`; returns its tensors and scalars after the last step."""
    p = torch.nn.Parameter(p_init.to(dtype).clone())
    opt = reference_cls()([p], lr=1.0, **kw)
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        p.grad = g.to(dtype) * torch.tensor(gs, dtype=torch.float32).to(dtype)
        opt.step()
    st, grp = opt.state[p], opt.param_groups[0]
    out = {"p": p.detach().double(), "exp_avg": st["exp_avg"].double(), "exp_avg_sq": st["exp_avg_sq"].double(), "s": st["s"].double()}
    out.update({k: float(grp[k]) for k in ("d", "d_numerator", "d_denom", "k")})
    return out


class Kernel:
    """`leco_prodigy` on a flat slab with caller-owned buffers, as FusedStep drives it."""

    def __init__(self, dev, p_init, kw, gs=1.0):
        c = dict(betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True, use_bias_correction=False,
                 safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf"))
        c.update(kw)
        if c["beta3"] is None:
            c["beta3"] = math.sqrt(c["betas"][1])
        self.c, self.dev, self.n, self.gs = c, dev, p_init.numel(), gs
        self.p = p_init.clone().to(dev)
        self.p0 = self.p.clone()
        self.m, self.v, self.s = (torch.zeros_like(self.p) for _ in range(3))
        self.shadow = torch.zeros(self.n, dtype=bf, device=dev)
        self.hyper = torch.zeros(4, device=dev)
        self.state = ops.prodigy_state(c["d0"], dev)

    def step(self, g, lr):
        c = self.c
        self.hyper.copy_(torch.tensor([lr, 0.0, 0.0, self.gs]))
        ops.prodigy(self.p, g.to(self.dev), self.m, self.v, self.s, self.p0, self.shadow, self.hyper, self.state, c["betas"][0],
                    c["betas"][1], c["beta3"], c["eps"], c["weight_decay"], c["d_coef"], c["growth_rate"], c["decouple"],
                    c["use_bias_correction"], c["safeguard_warmup"], self.n).run()
        _sync(self.dev)

    def result(self):
        out = {"p": self.p.cpu().double(), "exp_avg": self.m.cpu().double(), "exp_avg_sq": self.v.cpu().double(), "s": self.s.cpu().double()}
        out.update(dict(zip(ops.PRODIGY_STATE_FIELDS, self.state.cpu().tolist())))
        return out


def dist(a, b):
    if isinstance(b, float):
        return abs(a - b) / max(abs(b), 1e-300)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def assert_within_fp32_distance(got, r32, r64, what=""):
    """|got - r64| <= MARGIN * |r32 - r64| for every compared quantity."""
    report, bad = [], []
    for k in ("p", "exp_avg", "exp_avg_sq", "s", "d", "d_numerator", "d_denom"):
        e, cal = dist(got[k], r64[k]), dist(r32[k], r64[k])
        bound = MARGIN * cal
        report.append(f"{k}: kernel {e:.3g} fp32-restatement {cal:.3g}")
        if not e <= bound:
            bad.append(k)
    print(f"prodigy {what} vs float64: " + "; ".join(report))
    assert not bad, f"{what}: {bad} beyond {MARGIN} x the fp32 restatement's own distance from float64 -- " + "; ".join(report)
    assert got["k"] == r64["k"]


def _inputs(n, steps, seed):
    gen = torch.Generator().manual_seed(seed)
    p_init = torch.randn(n, generator=gen) * 0.05
    # LoRA-like gradients: a common direction plus noise, so that the distance estimate actually grows
    base = torch.randn(n, generator=gen)
    grads = [(base + 0.5 * torch.randn(n, generator=gen)) * 1e-3 for _ in range(steps)]
    # a decaying schedule, as fp32 values (lr travels in the fp32 hyper block)
    lrs = [float(torch.tensor(2.0 - 0.05 * i, dtype=torch.float32)) for i in range(steps)]
    return p_init, grads, lrs


CASES = {
    "defaults": {},
    "bias_correction_safeguard": dict(use_bias_correction=True, safeguard_warmup=True),
    "decoupled_wd": dict(weight_decay=0.1),
    "coupled_wd": dict(weight_decay=0.1, decouple=False),
    "growth_1.02": dict(growth_rate=1.02),
    "d_coef_2": dict(d_coef=2.0),
}


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_matches_the_float64_reference(dev, case):
    """20 steps of seeded gradients with a changing lr on 100 003 elements (391 blocks: the ticket path), gradient scale
    0.5 through hyper[3].  p, exp_avg, exp_avg_sq, s, d, d_numerator, d_denom within 4 x the float32 restatement's distance
    from the float64 one; the shadow is p.to(bfloat16) exactly.
    Measured, kernel / fp32 restatement, relative to float64 (gfx950; the emulator tier gives the same kernel figures, the
    restatement's move by ~10 % with the host's summation order): defaults p 3.35e-6 / 3.30e-6, exp_avg 3.32e-6 / 3.34e-6,
    exp_avg_sq 6.65e-6 / 6.69e-6, s 6.62e-6 / 6.66e-6, d 3.36e-6 / 3.26e-6, d_numerator 9.98e-6 / 9.91e-6, d_denom 6.62e-6 /
    6.65e-6; the largest ratio of all cases is d under decoupled decay, 3.7e-7 / 3.0e-7 (emulator host: / 2.7e-7 = 1.4 x); the
    largest distances are coupled decay's (p 6.2e-3 both, d 6.6e-5 both).  fp32 state itself is what costs: p0 - p cancels
    while the first steps move a 5e-2 weight by 1e-6."""
    kw = CASES[case]
    n, steps, gs = 100_003, 20, 0.5
    p_init, grads, lrs = _inputs(n, steps, seed=31)
    r64 = run_reference(torch.float64, p_init, grads, lrs, kw, gs)
    r32 = run_reference(torch.float32, p_init, grads, lrs, kw, gs)
    kern = Kernel(dev, p_init, kw, gs)
    for g, lr in zip(grads, lrs):
        kern.step(g, lr)
    got = kern.result()
    print(f"prodigy {case}: d after {steps} steps {r64['d']:.4g}")
    assert r64["d"] > 1e-6, r64["d"]                     # the inputs exercise the estimate: d has left d0
    assert_within_fp32_distance(got, r32, r64, case)
    assert torch.equal(kern.shadow.cpu(), kern.p.cpu().to(bf))


def test_two_runs_are_bit_equal(dev):
    """Fixed grid + partials added in a fixed order: the same inputs give the same bits (p, moments, s, every scalar) --
    what keeps data-parallel replicas, which all see the same all-reduced gradient, on the same d."""
    kw = dict(use_bias_correction=True, growth_rate=1.5)
    p_init, grads, lrs = _inputs(300_007, 6, seed=32)      # 1 172 blocks: several partials per thread of the last block
    outs = []
    for _ in range(2):
        kern = Kernel(dev, p_init, kw)
        for g, lr in zip(grads, lrs):
            kern.step(g, lr)
        outs.append((kern.p.cpu(), kern.m.cpu(), kern.v.cpu(), kern.s.cpu(), kern.shadow.cpu(), kern.state.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert outs[0][5][0].item() > 1e-6
    assert_within_fp32_distance(kern.result(), run_reference(torch.float32, p_init, grads, lrs, kw),
                                run_reference(torch.float64, p_init, grads, lrs, kw), "300 007 elements")


def test_zero_gradient_step_changes_nothing(dev):
    """den == sum |s| == 0 (all gradients zero so far): p, d and k stay, and the next ordinary steps match the reference
    that saw the same sequence.  Also lr = 0: the step does not happen either (the package's d_denom stays 0)."""
    n = 5_003
    p_init, grads, lrs = _inputs(n, 4, seed=33)
    grads = [torch.zeros(n)] + grads
    lrs = [1.0] + lrs
    kern = Kernel(dev, p_init, {})
    kern.step(grads[0], lrs[0])
    got = kern.result()
    assert torch.equal(kern.p.cpu(), p_init) and got["d"] == 1e-6 and got["k"] == 0 and got["d_denom"] == 0
    assert torch.equal(kern.shadow.cpu(), p_init.to(bf))
    for g, lr in zip(grads[1:], lrs[1:]):
        kern.step(g, lr)
    r64 = run_reference(torch.float64, p_init, grads, lrs, {})
    r32 = run_reference(torch.float32, p_init, grads, lrs, {})
    assert r64["k"] == 4
    assert_within_fp32_distance(kern.result(), r32, r64, "after a zero-gradient step")
    before = kern.result()
    kern.step(grads[1], 0.0)
    after = kern.result()
    assert torch.equal(before["p"], after["p"]) and after["d"] == before["d"] and after["k"] == before["k"]


def test_bad_arguments_are_refused(dev):
    from leco_amd import hip
    kern = Kernel(dev, torch.zeros(64), {})
    kern.c["betas"] = (0.9, 1.5)
    with pytest.raises(hip.LecoError, match="betas"):
        kern.step(torch.zeros(64), 1.0)
    with pytest.raises(ValueError, match="leco_prodigy_state"):
        ops.prodigy(kern.p, kern.p, kern.m, kern.v, kern.s, kern.p0, kern.shadow, kern.hyper, kern.hyper, 0.9, 0.999, 0.99, 1e-8,
                    0.0, 1.0, 2.0, True, False, False, 64)


# ---- through FusedStep / train() on the tiny UNet ----------------------------------------------------------------------
def hip_unet(dev):
    from oracle import unet_ref as R
    u = R.init_synthetic_(R.UNet2DConditionModel(R.tiny_config()), seed=1234)
    with torch.no_grad():
        for p in u.parameters():
            p.copy_(p.to(bf).float())
    m = UNet2DConditionModel(model_util.tiny_config())
    m.load_state_dict(u.state_dict())
    m = m.to(dev, bf)
    m.requires_grad_(False)
    m.engine().deterministic = True             # LECO_DETERMINISTIC: LoRA wgrads without fp32 atomics
    return m


def fresh_net(m):
    with contextlib.redirect_stdout(io.StringIO()):
        net = LoRANetwork(m, rank=4, multiplier=1.0, alpha=1.0)
    with torch.no_grad():
        for l in net.unet_loras:
            l.lora_down.weight.copy_(GOLD["lora." + l.lora_name + ".down"].reshape(l.lora_down.weight.shape))
            l.lora_up.weight.copy_(GOLD["lora." + l.lora_name + ".up"].reshape(l.lora_up.weight.shape))
    net.mark_updated()
    return net


def _pair(res):
    emb = {n: GOLD["emb." + n] for n in ("target", "positive", "neutral", "unconditional")}
    settings = prompt_util.PromptSettings(target="t", positive="p", neutral="n", unconditional="u", guidance_scale=2.0,
                                          batch_size=1, resolution=res, action="erase")
    return prompt_util.PromptEmbedsPair(torch.nn.MSELoss(), emb["target"], emb["positive"], emb["unconditional"], emb["neutral"],
                                        settings)


PRODIGY_KW = dict(use_bias_correction=True, safeguard_warmup=True, d_coef=1.0)


def test_fused_step_matches_the_reference_optimizer_object(dev):
    """Three `FusedStep.step`s with optimizer="prodigy" against a second network driven on the generic path by the reference
    optimizer object (deterministic engine: both see the same gradients as long as their bf16 shadows agree).  The gradients
    of the generic run are replayed through the float64 / float32 restatement on the flat slab: the fused slab is within
    4 x the fp32 distance of the float64 replay (the tolerance of the kernel test), and within the same bound of the
    generic path's slab.  d has grown above d0.
    Measured: fused, generic and the fp32 restatement all 4.35e-8 from the float64 replay, fused vs generic 1.1e-9 (emulator
    tier) / 8.2e-10 (gfx950)."""
    from leco_amd import train_util
    res = 64 if dev.type == "cpu" else 128
    m_f, m_g = hip_unet(dev), hip_unet(dev)      # an engine drives the LoRA network attached last: one model per network
    pair, sched = _pair(res), create_noise_scheduler("ddim")
    net_f, net_g = fresh_net(m_f), fresh_net(m_g)
    p_init = net_f.slab.detach().cpu().clone()
    kw = dict(d_coef=2.0)
    fs_f = FusedStep(m_f, net_f, sched, N_STEPS, lr=1.0, weight_decay=0.0, optimizer="prodigy", prodigy=kw)
    opt = reference_cls()(net_g.prepare_optimizer_params(), lr=1.0, **kw)
    fs_g = FusedStep(m_g, net_g, sched, N_STEPS, lr=1.0, weight_decay=0.0, optimizer=opt)
    grads = []
    torch.manual_seed(5)
    latents = train_util.get_initial_latents(sched, 1, res, res, 1)      # the same sample every step: the estimate sees
    for fs in (fs_f, fs_g):                                                # consistent gradients and d leaves d0 within three
        for _ in range(3):
            fs.step(pair, 1, latents, lr=1.0)
            if fs is fs_g:
                grads.append(fs.net.grad.detach().cpu().clone())
    _sync(dev)
    st = fs_f.prodigy_state()
    assert st["k"] == 3 and st["d"] > st["d0"] == 1e-6 and st["dlr"] > 0
    r64 = run_reference(torch.float64, p_init, grads, [1.0] * 3, kw)
    r32 = run_reference(torch.float32, p_init, grads, [1.0] * 3, kw)
    fused, generic = net_f.slab.detach().cpu().double(), net_g.slab.detach().cpu().double()
    e_f, e_g, cal, direct = dist(fused, r64["p"]), dist(generic, r64["p"]), dist(r32["p"], r64["p"]), dist(fused, generic)
    print(f"prodigy FusedStep: fused vs float64 replay {e_f:.3g}, generic vs float64 replay {e_g:.3g}, fp32 restatement {cal:.3g}, "
          f"fused vs generic {direct:.3g}, d {st['d']:.4g}")
    assert (fused - p_init.double()).abs().max() > 0
    assert e_f <= MARGIN * cal and direct <= MARGIN * cal, (e_f, direct, cal)
    assert dist(st["d"], r64["d"]) <= MARGIN * dist(r32["d"], r64["d"]), (st["d"], r64["d"], r32["d"])
    assert torch.equal(net_f.shadow.cpu(), net_f.slab.detach().to(bf).cpu())


def _train_config(tmp_path, name, iterations, optimizer_args):
    from leco_amd import config_util
    cfg = dict(prompts_file="unused", pretrained_model=dict(name_or_path="synthetic:tiny"),
               network=dict(type="lierla", rank=4, alpha=1.0),
               train=dict(precision="bfloat16", noise_scheduler="ddim", iterations=iterations, lr=1.0, optimizer="prodigy",
                          optimizer_args=optimizer_args, lr_scheduler="constant", max_denoising_steps=3),
               save=dict(name=name, path=str(tmp_path / name), per_steps=100), logging={}, other={})
    return config_util.RootConfig(**cfg)


def _prompts():
    return [prompt_util.PromptSettings(target="van gogh", positive="van gogh", unconditional="", neutral="", action="erase",
                                       guidance_scale=1.0, resolution=128, batch_size=1)]


def test_train_with_optimizer_prodigy(dev, tmp_path):
    """`train.optimizer: prodigy`, `lr: 1.0` and the example's optimizer_args on synthetic:tiny: the fused path runs (no
    prodigyopt needed), the loss is finite, lora_up has left zero and the LoRA file is written."""
    from leco_amd import train as T
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        net, loss = T.train(_train_config(tmp_path, "pg", 4, "d_coef=1.0 use_bias_correction=True safeguard_warmup=True"),
                            _prompts(), device=dev, use_graphs=False, progress=False)
    assert loss is not None and math.isfinite(loss)
    assert all(l.lora_up.weight.detach().abs().max().item() > 0 for l in net.unet_loras)
    assert torch.isfinite(net.slab.detach()).all()
    f = tmp_path / "pg" / "pg_last.safetensors"
    assert f.exists() and any(k.endswith("lora_up.weight") for k in load_file(str(f)))


def test_train_with_an_unsupported_prodigy_keyword_takes_the_package(dev, tmp_path):
    """A keyword the kernel does not implement is never dropped: the run goes to `prodigyopt.Prodigy` like before -- which,
    where the package is missing, is the ImportError that names it."""
    from leco_amd import train as T
    cfg = _train_config(tmp_path, "pk", 1, "d_coef=1.0 slice_p=11")
    try:
        import prodigyopt  # noqa: F401
        have = True
    except ImportError:
        have = False
    with contextlib.redirect_stdout(io.StringIO()):
        if have:
            T.train(cfg, _prompts(), device=dev, use_graphs=False, progress=False)
        else:
            with pytest.raises(ImportError, match="prodigyopt"):
                T.train(cfg, _prompts(), device=dev, use_graphs=False, progress=False)


def test_training_state_resume_is_bit_exact_with_prodigy(dev, tmp_path):
    """`test_training_state_resume_is_bit_exact` with Prodigy: two steps in one go vs step, save, a fresh network + load,
    step -- bit-equal slabs (s, p0 and the scalar state travel in the file).  The file is refused by an AdamW FusedStep,
    and an AdamW file by a Prodigy one, with the live network untouched."""
    from leco_amd import train as T, train_util
    res = 64 if dev.type == "cpu" else 128
    m = hip_unet(dev)
    pair, sched = _pair(res), create_noise_scheduler("ddim")

    def fresh(optimizer="prodigy"):
        net = fresh_net(m)
        kw = dict(optimizer="prodigy", prodigy=PRODIGY_KW, weight_decay=0.0) if optimizer == "prodigy" else {}
        return net, FusedStep(m, net, sched, N_STEPS, lr=1.0, **kw)

    def one(fs):
        fs.step(pair, 1, train_util.get_initial_latents(sched, 1, res, res, 1), lr=1.0)

    torch.manual_seed(3)
    net_a, fs_a = fresh()
    one(fs_a); one(fs_a)
    torch.manual_seed(3)
    net_b, fs_b = fresh()
    one(fs_b)
    T.save_training_state(tmp_path / "s.pt", fs_b, 0)
    torch.manual_seed(12345)
    net_c, fs_c = fresh()
    with torch.no_grad():
        net_c.slab.detach().zero_()
    assert T.load_training_state(tmp_path / "s.pt", fs_c) == 1
    assert fs_c.prodigy_state() == fs_b.prodigy_state() and fs_c.prodigy_state()["k"] == 1
    one(fs_c)
    a, c = net_a.slab.detach()[:net_a.numel].cpu(), net_c.slab.detach()[:net_c.numel].cpu()
    assert torch.equal(a, c)
    assert fs_a.prodigy_state() == fs_c.prodigy_state()
    # the wrong optimizer on either side: refused before anything is touched
    net_w, fs_w = fresh("adamw")
    keep = {k: getattr(net_w, k).detach().cpu().clone() for k in T.STATE_KEYS}
    with pytest.raises(ValueError, match="Prodigy"):
        T.load_training_state(tmp_path / "s.pt", fs_w)
    assert all(torch.equal(getattr(net_w, k).detach().cpu(), v) for k, v in keep.items()) and fs_w.opt_step == 0
    one(fs_w)
    T.save_training_state(tmp_path / "w.pt", fs_w, 0)
    blob = torch.load(tmp_path / "w.pt", map_location="cpu", weights_only=True)
    assert blob["format"] == 2 and "prodigy" not in blob          # the other optimizers' files are what they were
    before = net_c.slab.detach().cpu().clone()
    with pytest.raises(ValueError, match="Prodigy"):
        T.load_training_state(tmp_path / "w.pt", fs_c)
    assert torch.equal(net_c.slab.detach().cpu(), before) and fs_c.opt_step == 2
