"""Gradient clipping (`FusedStep(max_grad_norm=...)`) and accumulation (`FusedStep(accumulate=...)`, `flush`) through the
fused step, the training state, the config and `train()`, on the tiny synthetic model of the existing step tests -- host
emulator (CPU tier) and gfx950 (`-m gpu`).  The engine runs in deterministic mode (LECO_DETERMINISTIC: LoRA wgrads without
fp32 atomics) so that two runs from the same weights see the same gradient bits.

Tolerances are those of the existing optimizer-kernel tests, read there: AdamW `rel_err < 1e-5` (tests/test_kernels.py
test_timestep_ddim_loss_adamw), Lion `allclose(atol=1e-7)` (test_lion_matches_the_published_update), Prodigy within
MARGIN x the fp32 restatement's own distance from the float64 one (tests/test_prodigy.py)."""
import contextlib
import io
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from safetensors.torch import load_file

from conftest import rel_err
from test_prodigy import GOLD, MARGIN, N_STEPS, dist as pdist, fresh_net, hip_unet, run_reference

from leco_amd import config_util, ops, prompt_util, train_util
from leco_amd.scheduler import create_noise_scheduler
from leco_amd.train import FusedStep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 1e-2


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _res(dev):
    return 64 if dev.type == "cpu" else 128      # the emulator tier keeps the shapes small


def _pair(res, which="P"):
    """Two different prompt pairs on the golden embeddings: Q swaps the roles of the four prompts and the guidance."""
    names = ("target", "positive", "neutral", "unconditional") if which == "P" else ("neutral", "target", "unconditional", "positive")
    t, p, n, u = (GOLD["emb." + k] for k in names)
    settings = prompt_util.PromptSettings(target="t", positive="p", neutral="n", unconditional="u",
                                          guidance_scale=2.0 if which == "P" else 3.0, batch_size=1, resolution=res, action="erase")
    return prompt_util.PromptEmbedsPair(torch.nn.MSELoss(), t, p, u, n, settings)


def _latents(res, seed):
    torch.manual_seed(seed)
    return train_util.get_initial_latents(create_noise_scheduler("ddim"), 1, res, res, 1)


def _slab(net):
    return net.slab.detach()[:net.numel].cpu().clone()


def _grad(net, which="grad"):
    return getattr(net, which)[:net.numel].cpu().clone()


def adamw64(p, m, v, g, step, lr=LR, wd=WD):
    """One torch.optim.AdamW step in float64 on flat tensors."""
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    p = p * (1 - lr * wd) - (lr / (1 - B1 ** step)) * m / (v.sqrt() / math.sqrt(1 - B2 ** step) + EPS)
    return p, m, v


def clip64(g, max_norm, scale=1.0):
    """clip_grad_norm_ in float64 on the flat gradient `scale * g`: (clipped gradient, norm, coef)."""
    g = g.double() * scale
    norm = torch.linalg.vector_norm(g).item()
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    return g * coef, norm, coef


def _measured_norm(dev, m, pair, lat):
    """The gradient norm at the golden weights, as a measure-only step (max_grad_norm=0, lr=0) reports it."""
    net = fresh_net(m)
    fs = FusedStep(m, net, create_noise_scheduler("ddim"), N_STEPS, lr=0.0, max_grad_norm=0.0)
    fs.step(pair, 1, lat)
    st = fs.grad_stats()
    assert st["coef"] == 1.0 and st["nonfinite"] == 0 and st["norm"] > 0
    assert torch.equal(_slab(net), _slab(fresh_net(m)))            # measure only, lr = 0: nothing moved
    want = torch.linalg.vector_norm(_grad(net).double()).item()
    assert abs(st["norm"] - want) <= 2.0 ** -23 * want, (st, want)
    return st["norm"]


@pytest.mark.parametrize("optimizer", ["adamw", "lion", "prodigy"])
def test_clipped_step_matches_the_restatement(dev, optimizer):
    """Two clipped steps (max_grad_norm = half the norm a measure-only step reports: the clip engages, and the second step's
    moments mix two differently scaled gradients) against clip + optimizer restated in float64 on the gradients the steps
    left in `network.grad`."""
    res = _res(dev)
    m = hip_unet(dev)
    pair, lat, sched = _pair(res), _latents(res, 5), create_noise_scheduler("ddim")
    max_norm = 0.5 * _measured_norm(dev, m, pair, lat)
    net = fresh_net(m)
    p_init = _slab(net)
    kw = dict(adamw=dict(lr=LR, weight_decay=WD), lion=dict(lr=LR, weight_decay=WD, betas=(0.9, 0.99)),
              prodigy=dict(lr=1.0, weight_decay=0.0, prodigy=dict(d_coef=2.0)))[optimizer]
    fs = FusedStep(m, net, sched, N_STEPS, optimizer=optimizer, max_grad_norm=max_norm, **kw)
    grads, stats = [], []
    for _ in range(2):
        fs.step(pair, 1, lat)
        grads.append(_grad(net))
        stats.append(fs.grad_stats())
    _sync(dev)
    clipped = []
    for g, st in zip(grads, stats):
        gc, norm, coef = clip64(g, max_norm)
        assert coef < 1 and st["nonfinite"] == 0
        assert abs(st["norm"] - norm) <= 2.0 ** -23 * norm and abs(st["coef"] - coef) <= 2.0 ** -23 * coef, (st, norm, coef)
        clipped.append(gc)
    assert abs(net.hyper[3].item() - clip64(grads[1], max_norm)[2]) <= 2.0 ** -23        # grad_scale = coef / (world 1)
    got = _slab(net).double()
    assert (got - p_init.double()).abs().max() > 0
    if optimizer == "adamw":
        p, mm, vv = p_init.double(), torch.zeros_like(got), torch.zeros_like(got)
        for i, g in enumerate(clipped):
            p, mm, vv = adamw64(p, mm, vv, g, i + 1)
        e = rel_err(got, p)
        # the unclipped restatement must NOT pass: the test sees the clip
        q, mm, vv = p_init.double(), torch.zeros_like(got), torch.zeros_like(got)
        for i, g in enumerate(grads):
            q, mm, vv = adamw64(q, mm, vv, g.double(), i + 1)
        print(f"clipped adamw: slab vs float64 restatement {e:.3g} (unclipped restatement {rel_err(got, q):.3g})")
        assert e < 1e-5
        assert rel_err(net.exp_avg[:net.numel].cpu().double(), (1 - B1) * (B1 * clipped[0] + clipped[1])) < 1e-5
    elif optimizer == "lion":
        b1, b2 = 0.9, 0.99
        p, mo = p_init.double(), torch.zeros_like(got)
        for g in clipped:
            p = p * (1 - LR * WD) - LR * torch.sign(b1 * mo + (1 - b1) * g)
            mo = b2 * mo + (1 - b2) * g
        assert torch.allclose(got, p, atol=1e-7) and torch.allclose(net.exp_avg[:net.numel].cpu().double(), mo, atol=1e-7)
    else:
        pk = dict(d_coef=2.0)
        g32 = [g.float() for g in clipped]          # the scaled gradient fed in (the kernel multiplies in fp32 as well)
        r64 = run_reference(torch.float64, p_init, clipped, [1.0] * 2, pk)
        r32 = run_reference(torch.float32, p_init, g32, [1.0] * 2, pk)
        e, cal = pdist(got, r64["p"]), pdist(r32["p"], r64["p"])
        st = fs.prodigy_state()
        print(f"clipped prodigy: slab vs float64 restatement {e:.3g}, fp32 restatement {cal:.3g}, d {st['d']:.4g}")
        assert e <= MARGIN * cal, (e, cal)
        assert pdist(st["d"], r64["d"]) <= MARGIN * max(pdist(r32["d"], r64["d"]), 2.0 ** -23), (st["d"], r64["d"], r32["d"])
    assert torch.equal(net.shadow[:net.numel].cpu(), net.slab.detach()[:net.numel].to(torch.bfloat16).cpu())


def _record_launches(monkeypatch):
    names = []
    run, run_plan = ops.Op.run, ops.run_plan

    def op_run(self, stream=None):
        names.append(self.name)
        return run(self, stream)

    def plan_run(plan, stream=None):
        names.extend(op.name for op in plan)
        return run_plan(plan, stream)
    monkeypatch.setattr(ops.Op, "run", op_run)
    monkeypatch.setattr(ops, "run_plan", plan_run)
    return names


def test_unclipped_step_is_bit_identical_to_the_plain_step(dev, monkeypatch):
    """max_grad_norm = 1e9 never clips: slab, shadow and moments equal the plain step's bit for bit after 3 steps (coef == 1
    leaves hyper[3] alone).  With both options unset the step makes exactly the launches it made before: no grad_clip, no
    grad_accumulate, no grad_acc slab."""
    res = _res(dev)
    m = hip_unet(dev)
    pair, lat, sched = _pair(res), _latents(res, 5), create_noise_scheduler("ddim")
    names = _record_launches(monkeypatch)
    outs, launches = [], []
    for kw in ({}, dict(max_grad_norm=None, accumulate=1), dict(max_grad_norm=1e9)):
        net = fresh_net(m)
        fs = FusedStep(m, net, sched, N_STEPS, lr=LR, **kw)
        del names[:]
        for _ in range(1 if "accumulate" in kw else 3):      # (the explicit defaults: one step shows the launches)
            fs.step(pair, 1, lat)
            if len(launches) == len(outs):
                launches.append(list(names))                 # the first step's launches
        _sync(dev)
        every = list(names)
        assert not hasattr(net, "grad_acc")
        outs.append([t[:net.numel].cpu().clone() for t in (net.slab.detach(), net.shadow, net.exp_avg, net.exp_avg_sq)])
        if "max_grad_norm" in kw and kw["max_grad_norm"]:
            assert fs.grad_stats()["coef"] == 1.0
    for a, c in zip(outs[0], outs[2]):
        assert torch.equal(a, c)
    assert launches[0] == launches[1] and len(launches[0]) > 100
    assert not any("grad_clip" in n or "grad_accumulate" in n for n in launches[0])
    assert [n for n in launches[2] if n != "leco_grad_clip"] == launches[0] and launches[2].count("leco_grad_clip") == 1
    assert every.count("leco_grad_clip") == 3


def _gradient_at_init(m, pair, lat):
    net = fresh_net(m)
    fs = FusedStep(m, net, create_noise_scheduler("ddim"), N_STEPS, lr=0.0)
    fs.step(pair, 1, lat)
    return _grad(net)


def test_accumulation_of_two_pairs(dev):
    res = _res(dev)
    m = hip_unet(dev)
    P, Q, lat_p, lat_q = _pair(res, "P"), _pair(res, "Q"), _latents(res, 5), _latents(res, 6)
    g_p, g_q = _gradient_at_init(m, P, lat_p), _gradient_at_init(m, Q, lat_q)
    assert not torch.equal(g_p, g_q)
    net = fresh_net(m)
    fs = FusedStep(m, net, create_noise_scheduler("ddim"), N_STEPS, lr=LR, accumulate=2)
    m.prepare((2, 4, res // 8, res // 8), lora_on=True)          # shadow and packed operands are refreshed lazily: do it now
    p_init, shadow, version, packed_version = _slab(net), net.shadow.cpu().clone(), net.version, net._packed_version
    fs.step(P, 1, lat_p)
    _sync(dev)
    assert torch.equal(_slab(net), p_init) and torch.equal(net.shadow.cpu(), shadow) and fs.opt_step == 0 and fs.pending == 1
    assert net.version == version and net._packed_version == packed_version       # the packed operands were not rebuilt
    assert torch.equal(_grad(net, "grad_acc"), g_p)
    assert net.exp_avg.abs().max().item() == 0
    fs.step(Q, 1, lat_q)
    _sync(dev)
    assert torch.equal(_grad(net, "grad_acc"), g_p + g_q) and fs.opt_step == 1 and fs.pending == 0
    want, _, _ = adamw64(p_init.double(), torch.zeros(net.numel, dtype=torch.float64), torch.zeros(net.numel, dtype=torch.float64),
                         (g_p + g_q).double() / 2, 1)
    e = rel_err(_slab(net).double(), want)
    print(f"accumulate=2: slab vs float64 AdamW on the mean gradient {e:.3g}")
    assert e < 1e-5
    assert rel_err(net.exp_avg[:net.numel].cpu().double(), (1 - B1) * (g_p + g_q).double() / 2) < 1e-5      # the MEAN, not the sum
    assert net.version > version


def test_flush_applies_a_partial_group(dev):
    res = _res(dev)
    m = hip_unet(dev)
    P, Q, lat_p, lat_q = _pair(res, "P"), _pair(res, "Q"), _latents(res, 5), _latents(res, 6)
    g1, g2 = _gradient_at_init(m, P, lat_p), _gradient_at_init(m, Q, lat_q)
    net = fresh_net(m)
    fs = FusedStep(m, net, create_noise_scheduler("ddim"), N_STEPS, lr=LR, accumulate=3)
    p_init = _slab(net)
    fs.flush()                                    # nothing pending: nothing happens
    assert fs.opt_step == 0 and torch.equal(_slab(net), p_init)
    fs.step(P, 1, lat_p)
    fs.step(Q, 1, lat_q)
    assert fs.opt_step == 0 and fs.pending == 2 and torch.equal(_slab(net), p_init)
    fs.flush()
    _sync(dev)
    assert fs.opt_step == 1 and fs.pending == 0
    zeros = torch.zeros(net.numel, dtype=torch.float64)
    want, _, _ = adamw64(p_init.double(), zeros, zeros, (g1 + g2).double() / 2, 1)
    assert rel_err(_slab(net).double(), want) < 1e-5
    assert rel_err(net.exp_avg[:net.numel].cpu().double(), (1 - B1) * (g1 + g2).double() / 2) < 1e-5
    after = [t.cpu().clone() for t in (net.slab.detach(), net.shadow, net.exp_avg, net.exp_avg_sq)]
    fs.flush()
    _sync(dev)
    assert fs.opt_step == 1
    assert all(torch.equal(a, t.cpu()) for a, t in zip(after, (net.slab.detach(), net.shadow, net.exp_avg, net.exp_avg_sq)))


# ---- train(), the training state, the config ----------------------------------------------------------------------------
def _prompts():
    return [prompt_util.PromptSettings(target=t, positive=t, unconditional="", neutral="", action="erase", guidance_scale=1.0,
                                       resolution=64, batch_size=1) for t in ("van gogh", "monet")]


def _config(tmp_path, name, iterations, **train_kw):
    cfg = dict(prompts_file="unused", pretrained_model=dict(name_or_path="synthetic:tiny"), network=dict(type="lierla", rank=4, alpha=1.0),
               train=dict(precision="bfloat16", noise_scheduler="ddim", iterations=iterations, lr=1e-3, optimizer="AdamW",
                          lr_scheduler="cosine", max_denoising_steps=3, **train_kw),
               save=dict(name=name, path=str(tmp_path / name), per_steps=100), logging={}, other={})
    return config_util.RootConfig(**cfg)


def _spy_fused(monkeypatch):
    from leco_amd import train as T
    made, init = [], T.FusedStep.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        made.append(self)
    monkeypatch.setattr(T.FusedStep, "__init__", spy)
    return made


def test_train_loop_with_both_options(dev, tmp_path, monkeypatch):
    """The example config cut to 5 iterations: two full groups of 2 and the flushed remainder = 3 optimizer steps."""
    from leco_amd import train as T
    cfg = config_util.load_config_from_yaml(os.path.join(ROOT, "examples", "config_synthetic_tiny_clip_accum.yaml"))
    assert cfg.train.max_grad_norm == 1.0 and cfg.train.gradient_accumulation_steps == 2
    cfg.train.iterations = 5
    cfg.save.path = str(tmp_path / "ca")
    prompts = prompt_util.load_prompts_from_yaml(os.path.join(ROOT, "examples", "prompts.yaml"))
    made = _spy_fused(monkeypatch)
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        net, loss = T.train(cfg, prompts, device=dev, use_graphs=False, progress=False)
    fs = made[-1]
    assert fs.opt_step == 3 and fs.pending == 0 and fs.accumulate == 2 and fs.max_grad_norm == 1.0
    st = fs.grad_stats()
    assert st["nonfinite"] == 0 and st["norm"] > 0 and 0 < st["coef"] <= 1
    assert loss is not None and math.isfinite(loss) and torch.isfinite(net.slab.detach()).all()
    f = tmp_path / "ca" / f"{cfg.save.name}_last.safetensors"
    assert f.exists() and any(k.endswith("lora_up.weight") for k in load_file(str(f)))


def test_resume_in_the_middle_of_a_group_is_bit_exact(dev, tmp_path, monkeypatch):
    """accumulate=2, 5 iterations: stopped after iteration 2 (one micro-step pending; the state carries grad_acc), resumed
    and finished -- the final file equals the uninterrupted run's bit for bit.  A resume with another group length is
    refused, naming both; a state saved on a group boundary is the format it always was."""
    from leco_amd import train as T
    monkeypatch.setenv("LECO_DETERMINISTIC", "1")
    kw = dict(device=dev, use_graphs=False, progress=False)
    accum = dict(gradient_accumulation_steps=2, max_grad_norm=0.05)

    def run(name, **more):
        with contextlib.redirect_stdout(io.StringIO()):
            T.train(_config(tmp_path, name, 5, **accum), _prompts(), **kw, **more)
        return load_file(str(tmp_path / name / f"{name}_last.safetensors"))
    torch.manual_seed(21)
    full = run("full")
    torch.manual_seed(21)
    run("part", save_state=True, stop_after=2)
    state = tmp_path / "part" / "part_state.pt"
    blob = torch.load(state, map_location="cpu", weights_only=True)
    assert blob["format"] == 4 and blob["pending"] == 1 and blob["accumulate"] == 2 and blob["opt_step"] == 1
    assert blob["grad_acc"].shape == (1, *blob["slab"].shape) and blob["grad_acc"].abs().max() > 0
    made = _spy_fused(monkeypatch)
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(ValueError, match=r"(?s)2.*3|3.*2") as err:
        T.train(_config(tmp_path, "other", 5, gradient_accumulation_steps=3, max_grad_norm=0.05), _prompts(), **kw, resume_from=str(state))
    assert "2" in str(err.value) and "3" in str(err.value) and made[-1].opt_step == 0 and made[-1].pending == 0
    torch.manual_seed(999)
    resumed = run("part", resume_from=str(state))
    assert made[-1].opt_step == 3
    assert full.keys() == resumed.keys() and all(torch.equal(full[k], resumed[k]) for k in full)
    assert any(v.abs().max() > 0 for k, v in full.items() if k.endswith("lora_up.weight"))
    # on a group boundary (after iteration 1) nothing is pending: the file is what a run without the feature writes and reads
    torch.manual_seed(21)
    run("edge", save_state=True, stop_after=1)
    edge = torch.load(tmp_path / "edge" / "edge_state.pt", map_location="cpu", weights_only=True)
    assert edge["format"] == 2 and not {"grad_acc", "pending", "accumulate"} & set(edge)


def test_train_raises_on_nonfinite_gradients(dev, tmp_path, monkeypatch):
    """Where the loop shows the loss (iteration 0 here) it fetches grad_stats once; a non-finite count there ends the run
    with a FloatingPointError that names the iteration and the count."""
    from leco_amd import train as T
    stats = T.FusedStep.grad_stats
    monkeypatch.setattr(T.FusedStep, "grad_stats", lambda self: dict(stats(self), nonfinite=7))
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(FloatingPointError, match=r"iteration 0: 7 non-finite"):
        T.train(_config(tmp_path, "nf", 2, max_grad_norm=0.0), _prompts(), device=dev, use_graphs=False, progress=True)


def test_config_keys(tmp_path):
    base = open(os.path.join(ROOT, "examples", "config_synthetic_tiny.yaml")).read()
    assert "max_grad_norm" not in base and "gradient_accumulation_steps" not in base
    (tmp_path / "plain.yaml").write_text(base)
    plain = config_util.load_config_from_yaml(str(tmp_path / "plain.yaml"))
    assert plain.train.max_grad_norm is None and plain.train.gradient_accumulation_steps == 1
    both = base.replace("  max_denoising_steps: 5\n", "  max_denoising_steps: 5\n  max_grad_norm: 0.5\n  gradient_accumulation_steps: 4\n")
    assert both != base
    (tmp_path / "both.yaml").write_text(both)
    cfg = config_util.load_config_from_yaml(str(tmp_path / "both.yaml"))
    assert cfg.train.max_grad_norm == 0.5 and cfg.train.gradient_accumulation_steps == 4
    assert config_util.TrainConfig(max_grad_norm=0).max_grad_norm == 0           # measure only
    # unset, the two keys stay out of the dump (and of a saved LoRA's metadata): such a config dumps what it always did
    assert not {"max_grad_norm", "gradient_accumulation_steps"} & set(plain.model_dump()["train"])
    assert cfg.model_dump()["train"]["max_grad_norm"] == 0.5 and cfg.model_dump()["train"]["gradient_accumulation_steps"] == 4
    assert '"max_grad_norm":0.5' in cfg.model_dump_json() and "max_grad_norm" not in plain.model_dump_json()
    for bad in (dict(gradient_accumulation_steps=0), dict(gradient_accumulation_steps=-2), dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            config_util.TrainConfig(**bad)


def test_fused_step_refuses_bad_options(dev):
    m = hip_unet(dev)
    net = fresh_net(m)
    sched = create_noise_scheduler("ddim")
    for bad in (dict(accumulate=0), dict(accumulate=1.5), dict(max_grad_norm=-1.0), dict(max_grad_norm=float("nan"))):
        with pytest.raises(ValueError):
            FusedStep(m, net, sched, N_STEPS, **bad)
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        FusedStep(m, net, sched, N_STEPS).grad_stats()


# ---- data parallel: 2 processes, gloo, the host emulator -----------------------------------------------------------------
def _dp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LECO_DETERMINISTIC="1")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_dist as D
    D._setup()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    all_reduce = dist.all_reduce

    def counting(t, *a, **kw):
        calls.append(t.numel())
        return all_reduce(t, *a, **kw)
    dist.all_reduce = counting
    fs, net, pair = D._make(world)
    fs = FusedStep(fs.unet, net, fs.sched, 10, lr=1e-3, world_size=world, accumulate=2, max_grad_norm=1e-3)
    for i in range(4):                                  # two groups of two micro-steps on this rank's own noise
        fs.step(pair, 1, D._lat(10 * i + rank))
    st = fs.grad_stats()
    q.put((rank, len(calls), fs.opt_step, net.slab.detach()[:net.numel].numpy().copy(), (st["norm"], st["coef"], st["nonfinite"]),
           net.grad_acc[:net.numel].numpy().copy(), float(net.hyper[3])))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_accumulate_and_clip_identically():
    """accumulate=2 and clipping under data parallelism: ONE all-reduce per group (of grad_acc), both ranks end with
    bit-equal slabs and bit-equal grad_stats (the fixed-order reduction), grad_scale = coef / (world * group length)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        got = q.get(timeout=900)
        res[got[0]] = got[1:]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for r in range(2):
        assert res[r][0] == 2 and res[r][1] == 2, "one all-reduce and one optimizer step per group of two micro-steps"
    assert (res[0][2] == res[1][2]).all(), "ranks diverged"
    assert res[0][3] == res[1][3] and res[0][3][2] == 0
    assert (res[0][4] == res[1][4]).all()
    norm, coef, _ = res[0][3]
    want = torch.linalg.vector_norm(torch.from_numpy(res[0][4]).double() / 4).item()     # mean over 2 ranks x 2 micro-steps
    assert abs(norm - want) <= 2.0 ** -23 * want and coef < 1
    assert abs(res[0][5] - coef / 4) <= 2.0 ** -23 * coef / 4 and res[0][5] == res[1][5]
