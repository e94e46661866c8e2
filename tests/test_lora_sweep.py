"""Per-sample LoRA strengths: the forward-only SWEEP plans (`Engine.plan(strengths=True)`), `LoRANetwork.set_strengths` /
`from_file`, and `--lora_scales` of the two sampling scripts -- on the host emulator (CPU tier) and on gfx950 (`-m gpu`).

Plan parity, measured (relative L2 from the fp32 oracle, all three strengths; sweep / existing single-multiplier path):
see DESIGN.md section 7 "Per-sample strengths"."""
import contextlib
import importlib.util
import io
import os
import struct

import pytest
import torch
from safetensors.torch import load_file, save_file

from conftest import rel_err
from leco_amd import model_util
from leco_amd.lora import DEFAULT_TARGET_REPLACE, UNET_TARGET_REPLACE_MODULE_CONV, LoRANetwork
from leco_amd.unet import UNet2DConditionModel
from oracle import lora_ref
from oracle import unet_ref as R

bf = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRENGTHS = (-1.5, 0.0, 1.0)
C3LIER = list(DEFAULT_TARGET_REPLACE) + list(UNET_TARGET_REPLACE_MODULE_CONV)
# LoRA magnitude (std of lora_down and lora_up): large enough that, on the oracle alone, strengths -1.5 and 1 move the
# output by more than 10 x the parity tolerance (asserted below), small enough that the output stays in the range of the
# LoRA-off network
MAG = {4: 0.25, 72: 0.12}


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


def _pair(dev, xl: bool, rank: int, c3lier: bool, mag: float, seed: int = 11):
    """(oracle UNet, oracle LoRA, HIP UNet, HIP LoRA) on the same bf16-rounded weights; `up` and `down` random, non-zero."""
    ref = R.init_synthetic_(R.UNet2DConditionModel(R.tiny_config(xl=xl)), seed=1234 if not xl else 3)
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.to(bf).float())
    ref.requires_grad_(False)
    m = UNet2DConditionModel(model_util.tiny_xl_config() if xl else model_util.tiny_config())
    m.load_state_dict(ref.state_dict())
    m = m.to(dev, bf)
    m.requires_grad_(False)
    targets = C3LIER if c3lier else list(DEFAULT_TARGET_REPLACE)
    with _quiet():
        rnet = lora_ref.LoRANetworkRef(ref, rank=rank, targets=targets)
        net = LoRANetwork(m, rank=rank, target_replace_modules=targets)
    assert [l.lora_name for l in rnet.unet_loras] == [l.lora_name for l in net.unet_loras]
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for rl, l in zip(rnet.unet_loras, net.unet_loras):
            d = (torch.randn(rl.lora_down.weight.shape, generator=g) * mag).to(bf).float()
            u = (torch.randn(rl.lora_up.weight.shape, generator=g) * mag).to(bf).float()
            rl.lora_down.weight.copy_(d); rl.lora_up.weight.copy_(u)
            l.lora_down.weight.copy_(d.reshape(l.lora_down.weight.shape)); l.lora_up.weight.copy_(u.reshape(l.lora_up.weight.shape))
    net.mark_updated()
    return ref, rnet, m, net


def _inputs(xl: bool, seed: int = 5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 4, 16, 16, generator=g).to(bf)
    ctx = torch.randn(2, 77, 64, generator=g).to(bf)                 # [uncond; cond]
    extra = None
    if xl:
        extra = {"text_embeds": torch.randn(2, 64, generator=g).to(bf), "time_ids": torch.tensor([[128., 128, 0, 0, 128, 128]] * 2)}
    return x, ctx, extra


def _call(m, dev, x, ctx, extra, n):
    """One CFG-doubled pass over n copies of the sample: batch [uncond x n; cond x n] (train_util.predict_noise)."""
    kw = {}
    if extra is not None:
        kw["added_cond_kwargs"] = {k: v.repeat_interleave(n, 0).to(dev) for k, v in extra.items()}
    with torch.no_grad():
        y = m(x.repeat(2 * n, 1, 1, 1).to(dev), torch.tensor(500), encoder_hidden_states=ctx.repeat_interleave(n, 0).to(dev), **kw).sample
    return y.float().cpu()


def _oracle(ref, rnet, x, ctx, extra, s):
    for l in rnet.unet_loras:
        l.multiplier = s
    kw = {} if extra is None else {"added_cond_kwargs": {k: v.float() for k, v in extra.items()}}
    with torch.no_grad():
        return ref(x.repeat(2, 1, 1, 1).float(), torch.tensor(500), encoder_hidden_states=ctx.float(), **kw).sample


@pytest.mark.parametrize("xl", [False, True], ids=["sd", "xl"])
@pytest.mark.parametrize("rank,c3lier", [(4, False), (72, True)], ids=["lierla4", "c3lier72"])
def test_sweep_plan_matches_single_strength_passes_and_the_oracle(dev, xl, rank, c3lier):
    """One CFG-doubled batch at strengths (-1.5, 0, 1) == three single-strength passes through the existing path
    (`network.multiplier = s`) == the fp32 oracle, sample by sample.  Tolerance: 1.5 x the relative L2 of the EXISTING
    single-multiplier path from the oracle, measured here (the margin covers the one extra bf16 rounding of T . s)."""
    ref, rnet, m, net = _pair(dev, xl, rank, c3lier, MAG[rank])
    x, ctx, extra = _inputs(xl)
    n = len(STRENGTHS)
    gold = [_oracle(ref, rnet, x, ctx, extra, s) for s in STRENGTHS]          # each [2 = uncond, cond][4][16][16]
    single = []
    for s in STRENGTHS:
        net.multiplier = s
        single.append(_call(m, dev, x, ctx, extra, 1))
    net.multiplier = 0
    off = _call(m, dev, x, ctx, extra, 1)
    net.multiplier = 1.0
    net.set_strengths(STRENGTHS)
    y = _call(m, dev, x, ctx, extra, n)                                        # rows [u(-1.5) u(0) u(1) c(-1.5) c(0) c(1)]
    sweep = [torch.stack([y[i], y[n + i]]) for i in range(n)]
    assert any(k[-1] == "sweep" for k in m.engine().plans), list(m.engine().plans)
    e_single = [rel_err(a, g) for a, g in zip(single, gold)]
    e_sweep = [rel_err(a, g) for a, g in zip(sweep, gold)]
    d_pair = [rel_err(a, b) for a, b in zip(sweep, single)]
    tol = [1.5 * e for e in e_single]
    moved = [rel_err(gold[i], gold[1]) for i in (0, 2)]
    print(f"sweep parity {'xl' if xl else 'sd'} rank {rank}{' c3lier' if c3lier else ''} [{dev.type}]: "
          f"single vs oracle {['%.4g' % e for e in e_single]}, sweep vs oracle {['%.4g' % e for e in e_sweep]}, "
          f"sweep vs single {['%.4g' % e for e in d_pair]}, strength 0 vs LoRA-off {rel_err(sweep[1], off):.4g}, "
          f"oracle moved by {['%.4g' % e for e in moved]}")
    # not vacuous: on the oracle alone the two non-zero strengths move the output by >= 10 x the tolerance
    assert min(moved) >= 10 * max(tol), (moved, tol)
    for i in range(n):
        assert e_sweep[i] <= tol[i], (STRENGTHS[i], e_sweep[i], tol[i])
        assert d_pair[i] <= tol[i], (STRENGTHS[i], d_pair[i], tol[i])
    assert rel_err(sweep[1], off) <= tol[1]


def test_strengths_change_between_graph_replays_without_a_repack(dev):
    """Capture once, replay at (1, 1), write (-1, 2) into the strength buffer, replay: equals an eager run at (-1, 2); the
    packed operand images and the captured graph are the same objects throughout.  On the GPU the capture runs in an
    interpreter of its own (`python tests/test_lora_sweep.py graph_replay`), like the cases of tests/test_fullsize.py: a
    hipGraph capture in the shared test process can be followed by a segfault inside `hipStreamBeginCapture` of a LATER
    test's full-size model, and the other graph tests of the suite avoid it in the same ways."""
    if dev.type == "cuda":
        import subprocess
        import sys
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "graph_replay"], capture_output=True, text=True, timeout=300,
                           cwd=ROOT)
        assert r.returncode == 0 and "graph replay ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        return
    _check_graph_replay(dev)


def _check_graph_replay(dev):
    _, _, m, net = _pair(dev, False, 4, False, MAG[4])
    x, ctx, _ = _inputs(False)
    m.use_graphs = True

    def run():
        with torch.no_grad():
            return m(x.repeat(2, 1, 1, 1).to(dev), torch.tensor(500), encoder_hidden_states=ctx.to(dev)).sample.float().cpu()
    net.set_strengths((1.0, 1.0))
    y11 = run()
    plan = next(p for k, p in m.engine().plans.items() if k[-1] == "sweep")
    packed, graph = net._packed_version, plan.graphs.get("fwd_on")
    if dev.type == "cuda":
        assert graph is not None
    net.set_strengths((-1.0, 2.0))
    y_replay = run()
    assert net._packed_version == packed and plan.graphs.get("fwd_on") is graph
    assert torch.equal(plan.strengths.cpu(), torch.tensor([-1.0, 2.0]))
    m.use_graphs = False
    y_eager = run()
    assert torch.equal(y_replay, y_eager)
    assert rel_err(y_replay, y11) > 1e-2
    m.release()


def test_from_file_rebuilds_the_network(dev, tmp_path):
    m = UNet2DConditionModel(model_util.tiny_config()).to(dev, bf)
    g = torch.Generator().manual_seed(2)
    for rank, alpha, targets in ((4, 1.0, None), (8, 4.0, C3LIER)):
        with _quiet():
            net = LoRANetwork(m, rank=rank, alpha=alpha, target_replace_modules=targets)
        with torch.no_grad():
            for l in net.unet_loras:
                l.lora_up.weight.copy_(torch.randn(l.lora_up.weight.shape, generator=g) * 0.1)
        f = str(tmp_path / f"r{rank}.safetensors")
        net.save_weights(f, dtype=torch.float32)
        saved = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
        again = LoRANetwork.from_file(m, f)
        assert again.lora_dim == rank and again.alpha == alpha and len(again.unet_loras) == len(net.unet_loras)
        sd = again.state_dict()
        assert list(sd) == list(saved)
        for k in saved:
            assert torch.equal(sd[k].cpu(), saved[k]), k
        assert abs(again.unet_loras[0].scale - alpha / rank) < 1e-12
    # a file with the reference's keys (tests/golden/tiny_lora_keys.txt: written by the reference's own lora.py), fp16 as
    # the reference saves it
    gold = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "tiny_lora_keys.txt")):
        key, shape = line.split(" ", 1)
        shape = tuple(int(v) for v in shape.strip().strip("()").split(",") if v.strip())
        gold[key] = torch.tensor(1.0) if key.endswith(".alpha") else (torch.randn(shape, generator=g) * 0.1).half()
    f = str(tmp_path / "reference.safetensors")
    save_file(gold, f)
    theirs = LoRANetwork.from_file(m, f)
    sd = theirs.state_dict()
    assert set(sd) == set(gold) and theirs.lora_dim == 4
    for k, v in gold.items():
        assert torch.equal(sd[k].cpu().float().reshape(v.shape), v.float()), k
    # mixed ranks
    mixed = dict(load_file(str(tmp_path / "r4.safetensors")))
    names = sorted(k[:-len(".lora_down.weight")] for k in mixed if k.endswith(".lora_down.weight"))
    k = names[3] + ".lora_down.weight"
    mixed[k] = torch.cat([mixed[k], mixed[k]], 0)
    mixed[names[3] + ".lora_up.weight"] = torch.cat([mixed[names[3] + ".lora_up.weight"]] * 2, 1)
    f = str(tmp_path / "mixed.safetensors")
    save_file({k: v.contiguous() for k, v in mixed.items()}, f)
    with pytest.raises(ValueError, match="not uniform") as ei:
        LoRANetwork.from_file(m, f)
    assert names[3] in str(ei.value) and names[0] in str(ei.value)


def test_set_strengths_interface(dev):
    _, _, m, net = _pair(dev, False, 4, False, MAG[4])
    x, ctx, _ = _inputs(False)

    def run(batch):
        with torch.no_grad():
            return m(x.repeat(batch, 1, 1, 1).to(dev), torch.tensor(500),
                     encoder_hidden_states=ctx[:1].repeat(batch, 1, 1).to(dev)).sample.float().cpu()
    before = run(4)
    plans = set(m.engine().plans)
    net.set_strengths((1.0, 0.5, 2.0))
    with pytest.raises(ValueError, match="multiple"):
        run(4)
    net.set_strengths((1.0, 0.5))
    swept = run(4)
    # rows 0 and 2 run at strength 1, rows 1 and 3 at 0.5
    assert rel_err(swept[0], before[0]) < rel_err(swept[1], before[1]) and rel_err(swept[1], before[1]) > 1e-2
    net.multiplier = 0                       # `multiplier` stays the on / off switch
    off = run(4)
    net.multiplier = 1.0
    assert rel_err(off[1], before[1]) > 1e-2
    net.set_strengths(None)
    after = run(4)
    assert torch.equal(after, before)        # the same bits as before the feature was used
    assert plans <= set(m.engine().plans)
    with pytest.raises(ValueError):
        net.set_strengths(())


def test_sweep_on_a_float32_model_is_refused():
    """The fp32 compute mode has no sweep variant: the request raises before anything is built."""
    from conftest import _bind_emu
    _bind_emu()
    m = UNet2DConditionModel(model_util.tiny_config()).float()
    m.requires_grad_(False)
    with _quiet():
        net = LoRANetwork(m, rank=4)
    net.set_strengths((0.0, 1.0))
    g = torch.Generator().manual_seed(1)
    with pytest.raises(NotImplementedError, match="float32"):
        with torch.no_grad():
            m(torch.randn(2, 4, 16, 16, generator=g), torch.tensor(10), encoder_hidden_states=torch.randn(2, 77, 64, generator=g))
    with pytest.raises(NotImplementedError, match="float32"):
        m.engine().plan(2, 16, 16, need_bwd=False, strengths=True)


# ---- the sampling scripts -----------------------------------------------------------------------------------------------------
def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("script,model", [("infer", "synthetic:tiny"), ("infer_xl", "synthetic:tiny_xl")])
def test_infer_scripts_lora_scales(dev, tmp_path, script, model):
    from leco_amd.vae import load_png, save_png
    mod = _script(script)
    unet = (model_util.load_models_xl if script == "infer_xl" else model_util.load_models)(model, "ddim")[2]
    with _quiet():
        net = LoRANetwork(unet.to(dev, bf), rank=4, multiplier=1.0, alpha=1.0)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for l in net.unet_loras:
            l.lora_up.weight.copy_(torch.randn(l.lora_up.weight.shape, generator=g) * 0.3)
    f = str(tmp_path / "x_last.safetensors")
    net.save_weights(f, dtype=torch.float32)
    sheet, out = str(tmp_path / "sheet.png"), str(tmp_path / "latents.safetensors")
    base = ["--model", model, "--height", "128", "--width", "128", "--steps", "2", "--device", str(dev), "--no_graphs", "--out", out]
    with _quiet():
        lat = mod.main(base + ["--lora", f, "--lora_scales", "-1,0,1", "--image", sheet]).float().cpu()
    with open(sheet, "rb") as fh:
        head = fh.read(33)
    assert struct.unpack(">IIBB", head[16:26]) == (384, 128, 8, 2)              # width n * W, height H, 8-bit RGB
    img = load_png(sheet)
    panels = [img[:, 128 * i:128 * (i + 1)] for i in range(3)]
    assert not torch.equal(panels[0], panels[1]) and not torch.equal(panels[1], panels[2]) and not torch.equal(panels[0], panels[2])
    assert tuple(load_file(out)["latents"].shape) == (3, 4, 16, 16) and lat.shape == (3, 4, 16, 16)
    assert not torch.equal(lat[0], lat[1]) and not torch.equal(lat[1], lat[2])
    with _quiet():
        plain = mod.main(base + ["--lora", f]).float().cpu()
        typed = mod.main(base + ["--lora", f, "--rank", "4", "--alpha", "1"]).float().cpu()
    assert plain.shape == (1, 4, 16, 16) and torch.equal(plain, typed)
    # the sweep's strength-1 panel is the plain LoRA run (another launch plan: bf16 rounding apart, cf. the plan parity test)
    assert rel_err(lat[2], plain[0]) < rel_err(lat[1], plain[0]) and rel_err(lat[2], plain[0]) < rel_err(lat[0], plain[0])
    # img2img composes with the sweep
    init = str(tmp_path / "init.png")
    save_png(panels[1].contiguous(), init)
    with _quiet():
        i2i = mod.main(base + ["--lora", f, "--lora_scales", "-1,1", "--init_image", init, "--strength", "0.5"]).float().cpu()
    assert i2i.shape == (2, 4, 16, 16) and torch.isfinite(i2i).all() and not torch.equal(i2i[0], i2i[1])
    with pytest.raises(SystemExit):
        with contextlib.redirect_stderr(io.StringIO()):
            mod.main(base + ["--lora_scales", "-1,1"])


if __name__ == "__main__":
    import sys
    assert sys.argv[1:] == ["graph_replay"], sys.argv
    from conftest import _bind_hip
    _bind_hip()
    _check_graph_replay(torch.device("cuda:0"))
    torch.cuda.synchronize()
    print("graph replay ok")
