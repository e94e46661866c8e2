"""Max-norm regularisation of the LoRA weights (`FusedStep(scale_weight_norms=...)`, `LoRANetwork.weight_norms` /
`apply_max_norm`, `train.scale_weight_norms`) through the fused step, the network, the config and `train()`, on the tiny
synthetic model of the existing step tests -- host emulator (CPU tier) and gfx950 (`-m gpu`).  The engine runs in
deterministic mode (LECO_DETERMINISTIC: LoRA wgrads without fp32 atomics) so that two runs from the same weights see the same
gradient bits.

Bounds: a norm measured after the pull-back may exceed the bound by the two fp32 roundings of the factor, squared:
`norm <= max_norm * (1 + 4 * 2^-24)`.  `weight_norms()` against the float64 statement: one fp32 ulp, derived in
tests/test_lora_norm_kernels.py (the kernel sums exact double products; kappa < 1e4 is asserted on the inputs)."""
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

from test_lora_norm_kernels import _kappa, _within_one_ulp
from test_prodigy import GOLD, N_STEPS, fresh_net, hip_unet

from leco_amd import config_util, ops, prompt_util, train_util
from leco_amd.lora import DEFAULT_TARGET_REPLACE, UNET_TARGET_REPLACE_MODULE_CONV, LoRANetwork
from leco_amd.scheduler import create_noise_scheduler
from leco_amd.train import FusedStep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-3
SLACK = 1 + 4 * 2.0 ** -24
bf = torch.bfloat16


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _res(dev):
    return 64 if dev.type == "cpu" else 128      # the emulator tier keeps the shapes small


def _pair(res):
    t, p, n, u = (GOLD["emb." + k] for k in ("target", "positive", "neutral", "unconditional"))
    settings = prompt_util.PromptSettings(target="t", positive="p", neutral="n", unconditional="u", guidance_scale=2.0,
                                          batch_size=1, resolution=res, action="erase")
    return prompt_util.PromptEmbedsPair(torch.nn.MSELoss(), t, p, u, n, settings)


def _latents(res, seed=5):
    torch.manual_seed(seed)
    return train_util.get_initial_latents(create_noise_scheduler("ddim"), 1, res, res, 1)


def _slab(net):
    return net.slab.detach()[:net.numel].cpu().clone()


def _norms64(net):
    """{lora_name: float64 norm}, the statement of the issue, with the fp32 scale the table carries."""
    out = {}
    for l in net.unet_loras:
        U, D = l.lora_up.weight.detach().cpu().double().flatten(1), l.lora_down.weight.detach().cpu().double().flatten(1)
        out[l.lora_name] = (float(torch.tensor(l.scale, dtype=torch.float32)) * U @ D).norm().item()
    return out


def _bound(m):
    """Half the largest module norm of the golden LoRA weights: it bites from the first step on."""
    return 0.5 * max(fresh_net(m).weight_norms().values())


def _setup(dev, monkeypatch):
    monkeypatch.setenv("LECO_DETERMINISTIC", "1")
    m = hip_unet(dev)
    return m, _pair(_res(dev)), _latents(_res(dev)), create_noise_scheduler("ddim")


def test_bound_holds_after_every_optimizer_step(dev, monkeypatch):
    m, pair, lat, sched = _setup(dev, monkeypatch)
    bound = _bound(m)
    net = fresh_net(m)
    fs = FusedStep(m, net, sched, N_STEPS, lr=LR)
    fs.step(pair, 1, lat)
    assert max(net.weight_norms().values()) > bound, "the same run without the option exceeds the bound"
    net = fresh_net(m)
    fs = FusedStep(m, net, sched, N_STEPS, lr=LR, scale_weight_norms=bound)
    scaled = []
    for _ in range(2):
        fs.step(pair, 1, lat)
        st = fs.weight_norm_stats()                       # (before weight_norms(): that launch rewrites the stats)
        scaled.append(st["keys_scaled"])
        assert st["nonfinite"] == 0 and 0 < st["avg_norm"] <= st["max_norm"] <= bound * SLACK
        norms = net.weight_norms()
        print(f"max-norm step: scaled {st['keys_scaled']}, avg {st['avg_norm']:.6g}, max {st['max_norm']:.6g}, bound {bound:.6g}, "
              f"measured max {max(norms.values()):.9g}")
        assert len(norms) == len(net.unet_loras) and max(norms.values()) <= bound * SLACK
        assert torch.equal(net.shadow[:net.numel].cpu(), net.slab.detach()[:net.numel].to(bf).cpu())
    assert max(scaled) > 0 and fs.opt_step == 2


def test_a_loose_bound_and_zero_change_nothing(dev, monkeypatch):
    """A bound above every norm, and 0 (measure only): slab, shadow and moments equal the plain run's bit for bit."""
    m, pair, lat, sched = _setup(dev, monkeypatch)
    outs = []
    for kw in ({}, dict(scale_weight_norms=1e9), dict(scale_weight_norms=0.0)):
        net = fresh_net(m)
        fs = FusedStep(m, net, sched, N_STEPS, lr=LR, **kw)
        fs.step(pair, 1, lat)
        _sync(dev)
        outs.append([t[:net.numel].cpu().clone() for t in (net.slab.detach(), net.shadow, net.exp_avg, net.exp_avg_sq)])
        if kw:
            st = fs.weight_norm_stats()
            assert st["keys_scaled"] == 0 and st["max_norm"] > 0 and st["nonfinite"] == 0
        else:
            assert getattr(net, "_norm_buffers", None) is None          # unset: no allocation
            with pytest.raises(RuntimeError, match="scale_weight_norms"):
                fs.weight_norm_stats()
    for other in outs[1:]:
        for a, c in zip(outs[0], other):
            assert torch.equal(a, c)


def test_accumulation_runs_the_kernel_on_optimizer_steps_only(dev, monkeypatch):
    m, pair, lat, sched = _setup(dev, monkeypatch)
    bound = _bound(m)
    net = fresh_net(m)
    fs = FusedStep(m, net, sched, N_STEPS, lr=LR, accumulate=2, scale_weight_norms=bound)
    names, run = [], ops.Op.run

    def op_run(self, stream=None):
        names.append(self.name)
        return run(self, stream)
    monkeypatch.setattr(ops.Op, "run", op_run)
    stats0 = net.norm_buffers()[3].cpu().clone()
    fs.step(pair, 1, lat)
    _sync(dev)
    assert fs.opt_step == 0 and "leco_lora_max_norm" not in names
    assert torch.equal(net.norm_buffers()[3].cpu(), stats0)            # the stats object is unchanged after a micro-step
    fs.step(pair, 1, lat)
    _sync(dev)
    assert fs.opt_step == 1 and names.count("leco_lora_max_norm") == 1
    assert fs.weight_norm_stats()["keys_scaled"] > 0
    assert max(net.weight_norms().values()) <= bound * SLACK


@pytest.mark.parametrize("optimizer", ["adamw", "lion", "prodigy", "torch"])
def test_every_optimizer_branch_is_followed_by_the_pull_back(dev, monkeypatch, optimizer):
    m, pair, lat, sched = _setup(dev, monkeypatch)
    bound = _bound(m)
    net = fresh_net(m)
    kw = dict(adamw=dict(lr=LR, optimizer="adamw"), lion=dict(lr=LR, optimizer="lion", betas=(0.9, 0.99)),
              prodigy=dict(lr=1.0, weight_decay=0.0, optimizer="prodigy", prodigy=dict(d_coef=2.0)))
    if optimizer == "torch":
        kw["torch"] = dict(lr=1e-2, optimizer=torch.optim.SGD(net.prepare_optimizer_params(), lr=1e-2, momentum=0.9))
    fs = FusedStep(m, net, sched, N_STEPS, scale_weight_norms=bound, **kw[optimizer])
    p_init = _slab(net)
    fs.step(pair, 1, lat)
    st = fs.weight_norm_stats()
    assert st["nonfinite"] == 0 and st["max_norm"] <= bound * SLACK
    assert max(net.weight_norms().values()) <= bound * SLACK
    assert not torch.equal(_slab(net), p_init)
    assert torch.equal(net.shadow[:net.numel].cpu(), net.slab.detach()[:net.numel].to(bf).cpu())


def test_the_forward_sees_the_scaled_weights(dev, monkeypatch, tmp_path):
    """`predict_noise` with the network a regularised run trained equals, to the bit, `predict_noise` with a fresh network
    loaded from the file that run saved: the shadow the kernel rewrote is the image of the slab it scaled."""
    m, pair, lat, sched = _setup(dev, monkeypatch)
    bound = _bound(m)                                    # (before `net`: an engine drives the network attached last)
    net = fresh_net(m)
    fs = FusedStep(m, net, sched, N_STEPS, lr=LR, scale_weight_norms=bound)
    fs.step(pair, 1, lat)
    assert fs.weight_norm_stats()["keys_scaled"] > 0
    f = tmp_path / "trained.safetensors"
    net.save_weights(f, torch.float32)
    sched.set_timesteps(N_STEPS)
    emb = train_util.concat_embeddings(pair.unconditional, pair.target, 1).to(dev, bf)
    x, t = lat.to(dev, bf), sched.timesteps[2]
    with torch.no_grad():
        with net:
            a = train_util.predict_noise(m, sched, t, x, emb, guidance_scale=3.0).float().cpu()
        m2 = hip_unet(dev)                               # an engine drives the LoRA network attached last: one model per network
        net2 = LoRANetwork.from_file(m2, f)
        with net2:
            b = train_util.predict_noise(m2, sched, t, x, emb, guidance_scale=3.0).float().cpu()
        off = train_util.predict_noise(m, sched, t, x, emb, guidance_scale=3.0).float().cpu()     # outside `with`: LoRA off
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(a, off)                       # (the LoRA is visible in the prediction at all)


def test_apply_max_norm_on_a_loaded_network_then_save(dev, tmp_path):
    m = hip_unet(dev)
    src = tmp_path / "src.safetensors"
    fresh_net(m).save_weights(src, torch.float32)
    net = LoRANetwork.from_file(m, src)
    before = net.weight_norms()
    bound = 0.5 * max(before.values())
    above = sum(v > bound for v in before.values())
    assert 0 < above < len(before)
    version = net.version
    st = net.apply_max_norm(bound)
    assert st["keys_scaled"] == above and st["nonfinite"] == 0 and st["max_norm"] <= bound * SLACK
    assert net.version > version                          # mark_updated(): the packed operands follow
    dst = tmp_path / "dst.safetensors"
    net.save_weights(dst, torch.float32)
    a, b = load_file(str(src)), load_file(str(dst))
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype
        if k.endswith(".alpha"):
            assert torch.equal(a[k], b[k])
    after = LoRANetwork.from_file(m, dst).weight_norms()
    assert after.keys() == before.keys()
    for k, v in after.items():
        assert v <= bound * SLACK
        if before[k] <= bound:
            assert v == before[k]                         # modules inside the bound were not written
    version = net.version
    # (a pulled-back norm lies on the bound up to rounding, on either side: a bound just above scales nothing)
    assert net.apply_max_norm(bound * (1 + 8 * 2.0 ** -24))["keys_scaled"] == 0 and net.version == version
    with pytest.raises(ValueError):
        net.apply_max_norm(-1.0)


def test_c3lier_and_a_rank_above_64_against_float64(dev):
    m = hip_unet(dev)
    with contextlib.redirect_stdout(io.StringIO()):
        net = LoRANetwork(m, rank=80, multiplier=1.0, alpha=4.0,
                          target_replace_modules=list(DEFAULT_TARGET_REPLACE) + UNET_TARGET_REPLACE_MODULE_CONV)
    g = torch.Generator().manual_seed(91)
    with torch.no_grad():
        for l in net.unet_loras:
            l.lora_up.weight.copy_((torch.randn(l.lora_up.weight.shape, generator=g) * 0.05).to(l.lora_up.weight.device))
    ranks = {l.lora_dim for l in net.unet_loras}
    assert 80 in ranks and min(ranks) < 80                # clamped convolutions keep their own rank (and scale)
    assert any(l.lora_down.weight.ndim == 4 and l.lora_down.weight.shape[-1] == 3 for l in net.unet_loras)
    for l in net.unet_loras:
        assert _kappa(l.lora_up.weight.detach().cpu().flatten(1), l.lora_down.weight.detach().cpu()) < 1e4
    got, want = net.weight_norms(), _norms64(net)
    assert got.keys() == want.keys() and len(got) == len(net.unet_loras)
    for k in want:
        assert _within_one_ulp(got[k], want[k]), (k, got[k], want[k])


def _prompts():
    return [prompt_util.PromptSettings(target=t, positive=t, unconditional="", neutral="", action="erase", guidance_scale=1.0,
                                       resolution=64, batch_size=1) for t in ("van gogh", "monet")]


def test_train_with_the_example_config(dev, tmp_path, monkeypatch):
    """examples/config_synthetic_tiny_max_norm.yaml through `train()`: the bar shows |w|, modules are pulled back, and the
    saved LoRA's module norms obey the bound."""
    from leco_amd import train as T
    monkeypatch.setenv("LECO_DETERMINISTIC", "1")
    cfg = config_util.load_config_from_yaml(os.path.join(ROOT, "examples", "config_synthetic_tiny_max_norm.yaml"))
    bound = cfg.train.scale_weight_norms
    assert bound is not None and bound > 0
    cfg.save.path = str(tmp_path / "mn")
    cfg.save.per_steps = 100
    cfg.train.iterations, cfg.train.max_denoising_steps = 3, 3       # (the example cut short: the bound bites from step 2 on)
    made, init, shown = [], T.FusedStep.__init__, []

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        made.append(self)
    monkeypatch.setattr(T.FusedStep, "__init__", spy)
    import tqdm
    set_description = tqdm.tqdm.set_description
    monkeypatch.setattr(tqdm.tqdm, "set_description", lambda self, desc=None, refresh=True: (shown.append(desc), set_description(self, desc, refresh))[1])
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        net, loss = T.train(cfg, _prompts(), device=dev, use_graphs=False, progress=True)
    fs = made[-1]
    assert fs.scale_weight_norms == bound and fs.opt_step == cfg.train.iterations
    st = fs.weight_norm_stats()
    print(f"example config: {st}, bar {shown[-1]!r}")
    assert st["keys_scaled"] > 0 and st["max_norm"] <= bound * SLACK and st["nonfinite"] == 0
    assert any(" |w|: " in d for d in shown) and any("*" in d.split(" |w|: ")[1] for d in shown if " |w|: " in d)
    f = tmp_path / "mn" / f"{cfg.save.name}_last.safetensors"
    saved = load_file(str(f))
    # the file is written in train.precision (bf16, 2^-9 per element): a norm moves by at most (1 + 2^-9)^2 - 1 < 2^-7 relative
    for l in net.unet_loras:
        U, D = saved[l.lora_name + ".lora_up.weight"].double().flatten(1), saved[l.lora_name + ".lora_down.weight"].double().flatten(1)
        assert (l.scale * U @ D).norm().item() <= bound * (1 + 2.0 ** -7), l.lora_name
    assert max(net.weight_norms().values()) <= bound * SLACK


def test_config_key(tmp_path, monkeypatch):
    base = open(os.path.join(ROOT, "examples", "config_synthetic_tiny.yaml")).read()
    assert "scale_weight_norms" not in base
    (tmp_path / "plain.yaml").write_text(base)
    plain = config_util.load_config_from_yaml(str(tmp_path / "plain.yaml"))
    assert plain.train.scale_weight_norms is None
    assert "scale_weight_norms" not in plain.model_dump()["train"] and "scale_weight_norms" not in plain.model_dump_json()
    # unset, the dump has exactly the keys it had before the option existed
    assert set(plain.model_dump()["train"]) == set(config_util.TrainConfig.model_fields) - {"max_grad_norm", "gradient_accumulation_steps",
                                                                                           "scale_weight_norms"}
    cfg = config_util.load_config_from_yaml(os.path.join(ROOT, "examples", "config_synthetic_tiny_max_norm.yaml"))
    assert cfg.train.scale_weight_norms == 0.002 and cfg.model_dump()["train"]["scale_weight_norms"] == 0.002
    assert config_util.TrainConfig(scale_weight_norms=0).scale_weight_norms == 0           # measure only
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            config_util.TrainConfig(scale_weight_norms=bad)
    # --strict_reference with the key is refused before any model is loaded
    from leco_amd import model_util, train as T

    def no_models(*a, **kw):
        raise AssertionError("a model was loaded")
    monkeypatch.setattr(model_util, "load_models", no_models)
    monkeypatch.setattr(T, "init_distributed", no_models)
    with pytest.raises(ValueError, match="strict_reference"):
        T.train(cfg, _prompts(), device=torch.device("cpu"), strict_reference=True, progress=False)


def test_fused_step_refuses_bad_values(dev):
    m = hip_unet(dev)
    net = fresh_net(m)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="scale_weight_norms"):
            FusedStep(m, net, create_noise_scheduler("ddim"), N_STEPS, scale_weight_norms=bad)


# ---- data parallel: 2 processes, gloo, the host emulator -----------------------------------------------------------------
def _dp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LECO_DETERMINISTIC="1")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_dist as D
    D._setup()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    fs, net, pair = D._make(world)
    bound = 0.5 * max(net.weight_norms().values())
    fs = FusedStep(fs.unet, net, fs.sched, 10, lr=1e-3, world_size=world, scale_weight_norms=bound)
    scaled = 0
    for i in range(3):                                  # every rank on its own noise
        fs.step(pair, 1, D._lat(10 * i + rank))
        scaled += fs.weight_norm_stats()["keys_scaled"]
    st = fs.weight_norm_stats()
    q.put((rank, net.slab.detach()[:net.numel].numpy().copy(), net.shadow[:net.numel].float().numpy().copy(),
           (st["keys_scaled"], st["avg_norm"], st["max_norm"], st["nonfinite"]), scaled, bound,
           max(net.weight_norms().values())))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_stay_bit_equal_under_a_biting_bound():
    """Three data-parallel steps with a bound that bites: the ranks take the same decisions without communicating -- slabs,
    shadows and statistics are bit-equal."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37500 + (os.getpid() % 2000)
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
    assert (res[0][0] == res[1][0]).all() and (res[0][1] == res[1][1]).all(), "ranks diverged"
    assert res[0][2] == res[1][2] and res[0][2][3] == 0
    assert res[0][3] > 0 and res[0][3] == res[1][3]
    assert res[0][4] == res[1][4] and res[0][5] <= res[0][4] * SLACK and res[1][5] <= res[1][4] * SLACK
