"""Cross-attention token heatmaps at the model level: the MAPS plans (`Engine.plan(attn_maps=M)`), `set_attention_maps` /
`reset_attention_maps` / `attention_maps`, `attn_maps.token_weights` and `--attn_map` of the sampling scripts -- on the host
emulator (CPU tier) and on gfx950 (`-m gpu`).  `synthetic:tiny` / `tiny_xl` shapes at 8 x 8 latents (64 x 64 pixels)."""
import contextlib
import importlib.util
import io
import json
import os
import struct

import pytest
import torch

from conftest import rel_err
from leco_amd import attn_maps, model_util, ops
from leco_amd.lora import LoRANetwork
from leco_amd.unet import UNet2DConditionModel

bf = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = 8
# kernel bound of tests/test_attn_maps_kernels.py (relative L2 of one launch from a float64 softmax on the same bf16 operands)
BOUND = 1e-4


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


def _model(dev, xl=False, lora=False, mag=0.25):
    m = model_util.init_synthetic_(UNet2DConditionModel(model_util.tiny_xl_config() if xl else model_util.tiny_config()), 3 if xl else 1234)
    m = m.to(dev, bf)
    m.requires_grad_(False)
    net = None
    if lora:
        with _quiet():
            net = LoRANetwork(m, rank=4)
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            for l in net.unet_loras:
                l.lora_down.weight.copy_((torch.randn(l.lora_down.weight.shape, generator=g) * mag).to(l.lora_down.weight.device))
                l.lora_up.weight.copy_((torch.randn(l.lora_up.weight.shape, generator=g) * mag).to(l.lora_up.weight.device))
        net.mark_updated()
    return m, net


def _inputs(xl, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 4, HW, HW, generator=g).to(bf)
    ctx = torch.randn(2, 77, 64, generator=g).to(bf)                 # [uncond; cond]
    extra = None
    if xl:
        extra = {"text_embeds": torch.randn(2, 64, generator=g).to(bf), "time_ids": torch.tensor([[64., 64, 0, 0, 64, 64]] * 2)}
    return x, ctx, extra


def _call(m, dev, x, ctx, extra, n=1, t=500):
    """One CFG-doubled pass over n copies of the sample: batch [uncond x n; cond x n] (train_util.predict_noise)."""
    kw = {}
    if extra is not None:
        kw["added_cond_kwargs"] = {k: v.repeat_interleave(n, 0).to(dev) for k, v in extra.items()}
    with torch.no_grad():
        y = m(x.repeat(2 * n, 1, 1, 1).to(dev), torch.tensor(t), encoder_hidden_states=ctx.repeat_interleave(n, 0).to(dev), **kw).sample
    return y.float().cpu()


def _tok_w():
    tw = torch.zeros(2, 77)
    tw[0, 2] = 1.0
    tw[1, 4:7] = 1.0
    return tw


def _maps_plan(m):
    return m._attn_plan


def _restate(plan, m, tw):
    """float64, from the plan's own `q2` / `kv` buffers: per layer [Bc][M][hw] = mean over heads of the token columns of the
    softmax, the LAST Bc samples of the batch only."""
    out = []
    B = plan.x_in.shape[0]
    for name, buf, hw in plan.attn_layers:
        heads = m.engine().named[name].attn2.heads
        q = plan.bufs[name + ".q2"].double().cpu()
        kv = plan.bufs[name + ".kv"].double().cpu()
        C = q.shape[1]
        d = C // heads
        Bc = buf.shape[0]
        q = q.reshape(B, hw, heads, d)[B - Bc:]
        k = kv[:, :C].reshape(B, 77, heads, d)[B - Bc:]
        p = torch.softmax(torch.einsum("bihd,bjhd->bhij", q, k) * d ** -0.5, dim=-1)
        out.append(torch.einsum("mj,bhij->bmi", tw.double(), p) / heads)
    return out


@pytest.mark.parametrize("xl", [False, True], ids=["sd", "xl"])
def test_layer_maps_accumulate_the_cond_rows_of_every_cross_attention(dev, xl):
    m, _ = _model(dev, xl)
    x, ctx, extra = _inputs(xl)
    tw = _tok_w()
    m.set_attention_maps(tw)
    _call(m, dev, x, ctx, extra, t=500)
    plan = _maps_plan(m)
    n_blocks = sum(1 for n, mod in m.named_modules() if n.endswith(".attn2"))
    assert len(plan.attn_layers) == n_blocks and n_blocks >= 5
    assert not any(op.name in ("leco_xblock_tail", "leco_xblock_head") for op in plan.fwd[False])
    r1 = _restate(plan, m, tw)
    x2, _, _ = _inputs(xl, seed=9)
    _call(m, dev, x2, ctx, extra, t=200)
    assert _maps_plan(m) is plan
    r2 = _restate(plan, m, tw)
    worst = 0.0
    for (name, buf, hw), a, b in zip(plan.attn_layers, r1, r2):
        assert tuple(buf.shape) == (1, 2, hw)
        e = ((buf.double().cpu() - (a + b)).norm() / (a + b).norm()).item()
        worst = max(worst, e)
        assert e <= BOUND, (name, e)
    print(f"layer maps {'xl' if xl else 'sd'} [{dev.type}]: {len(plan.attn_layers)} layers, worst rel L2 {worst:.3g}")
    heat = m.attention_maps((64, 64))
    assert tuple(heat.shape) == (1, 2, 64, 64) and torch.isfinite(heat).all() and heat.min() >= 0
    # the probabilities of a row sum to one: the mean heat of a 3-token word at most 3 x 2 passes
    assert 0 < heat[0, 1].mean().item() <= 6.0
    m.reset_attention_maps()
    assert all(float(buf.abs().max()) == 0.0 for _, buf, _ in plan.attn_layers)
    m.release()


def test_maps_use_the_cond_rows_only(dev):
    """Swapping [uncond; cond] changes the maps; they follow the second half."""
    m, _ = _model(dev)
    x, ctx, extra = _inputs(False)
    m.set_attention_maps(_tok_w())
    _call(m, dev, x, ctx, extra)
    plan = _maps_plan(m)
    a = [buf.cpu().clone() for _, buf, _ in plan.attn_layers]
    m.reset_attention_maps()
    _call(m, dev, x, ctx.flip(0), extra)
    b = [buf.cpu().clone() for _, buf, _ in plan.attn_layers]
    assert all(rel_err(u, v) > 100 * BOUND for u, v in zip(a, b))
    # explicit cond_rows = the whole batch: twice the rows
    m.set_attention_maps(_tok_w(), cond_rows=2)
    _call(m, dev, x, ctx, extra)
    full = _maps_plan(m)
    assert full is not plan and full.attn_layers[0][1].shape[0] == 2
    for (_, buf, _), u in zip(full.attn_layers, a):
        assert torch.equal(buf[1].cpu(), u[0])           # the same pass, the same rows, the same bits
    m.release()


def test_pred_equals_the_per_op_forward_only_plan_bit_for_bit(dev, monkeypatch):
    """The map launches only read: in LECO_DETERMINISTIC=1 the noise prediction of a maps plan equals, bit for bit, that of
    the forward-only plan of the same shape built with LECO_STRIPE=0."""
    monkeypatch.setenv("LECO_DETERMINISTIC", "1")
    m, _ = _model(dev)
    assert m.engine().deterministic
    x, ctx, extra = _inputs(False)
    before = _call(m, dev, x, ctx, extra)
    plans = set(m.engine().plans)
    m.set_attention_maps(_tok_w())
    y = _call(m, dev, x, ctx, extra)
    monkeypatch.setenv("LECO_STRIPE", "0")
    eng = m.engine()
    p0 = eng.plan(2, HW, HW, need_bwd=False, tag="nostripe")
    monkeypatch.delenv("LECO_STRIPE")
    p0.x_in.copy_(x.repeat(2, 1, 1, 1).to(dev))
    p0.set_ctx(ctx.to(dev))
    p0.t_table[:1].fill_(500.0)
    p0.t_idx.zero_()
    ops.run_plan(p0.fwd[False])
    assert torch.equal(p0.pred.to(bf).float().cpu(), y)
    # off again: the previous plans, the same bits as before the feature was used
    m.set_attention_maps(None)
    after = _call(m, dev, x, ctx, extra)
    assert torch.equal(after, before) and plans <= set(eng.plans)
    m.release()


def test_a_strength_sweep_gets_one_map_per_cell(dev):
    """`set_strengths([-1, 0, 1])`: the three cells' maps differ, and the strength-0 cell's maps are the LoRA-off run's.  Bound
    for "are": the two runs go through different launch plans (sweep at batch 6, plain at batch 2), so their bf16 activations
    differ by rounding noise, as the existing sweep-plan parity test allows for the prediction (1.5 x the 1.1e-2 of the
    single-multiplier path from the oracle = 1.65e-2); the maps are smooth in q and k (scores of O(1)), so the same 1.65e-2
    holds for them.  "Differ": by more than 5 x that."""
    tol = 1.65e-2
    m, net = _model(dev, lora=True, mag=0.3)
    x, ctx, extra = _inputs(False)
    m.set_attention_maps(_tok_w())
    net.multiplier = 0
    _call(m, dev, x, ctx, extra)
    off = [buf.cpu().clone() for _, buf, _ in _maps_plan(m).attn_layers]
    net.multiplier = 1.0
    net.set_strengths((-1.0, 0.0, 1.0))
    _call(m, dev, x, ctx, extra, n=3)
    plan = _maps_plan(m)
    assert plan.key[-1].endswith("sweep") and "maps2x3" in plan.key[-1]
    cells = [buf.cpu().clone() for _, buf, _ in plan.attn_layers]
    assert tuple(cells[0].shape[:2]) == (3, 2)
    e0 = max(rel_err(c[1], o[0]) for c, o in zip(cells, off))
    lo = max(rel_err(c[0], c[1]) for c in cells)
    hi = max(rel_err(c[2], c[1]) for c in cells)
    print(f"sweep maps [{dev.type}]: strength 0 vs LoRA-off {e0:.3g}; -1 vs 0 {lo:.3g}, +1 vs 0 {hi:.3g}")
    assert e0 <= tol, e0
    assert lo >= 5 * tol and hi >= 5 * tol and max(rel_err(c[0], c[2]) for c in cells) >= 5 * tol
    heat = m.attention_maps((32, 32))
    assert tuple(heat.shape) == (3, 2, 32, 32)
    m.release()


def test_graph_replay_equals_eager(dev):
    """On the GPU the capture runs in an interpreter of its own, like the other graph tests of the suite."""
    if dev.type == "cuda":
        import subprocess
        import sys
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "graph_replay"], capture_output=True, text=True, timeout=300,
                           cwd=ROOT)
        assert r.returncode == 0 and "graph replay ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        return
    _check_graph_replay(dev)


def _check_graph_replay(dev):
    m, _ = _model(dev)
    x, ctx, extra = _inputs(False)
    m.set_attention_maps(_tok_w())
    m.use_graphs = True
    y1 = _call(m, dev, x, ctx, extra)
    y2 = _call(m, dev, x, ctx, extra)             # the second pass replays the captured graph
    plan = _maps_plan(m)
    if dev.type == "cuda":
        assert plan.graphs.get("fwd_off") is not None
    replay = [buf.cpu().clone() for _, buf, _ in plan.attn_layers]
    m.set_attention_step_weight(0.0)              # read on the device: the replayed graph is muted
    _call(m, dev, x, ctx, extra)
    assert all(torch.equal(buf.cpu(), r) for (_, buf, _), r in zip(plan.attn_layers, replay))
    m.set_attention_step_weight(1.0)
    m.use_graphs = False
    m.reset_attention_maps()
    e1 = _call(m, dev, x, ctx, extra)
    e2 = _call(m, dev, x, ctx, extra)
    assert torch.equal(y1, e1) and torch.equal(y2, e2)
    assert all(torch.equal(buf.cpu(), r) for (_, buf, _), r in zip(plan.attn_layers, replay))
    m.release()


def test_maps_on_a_float32_model_are_refused():
    from conftest import _bind_emu
    _bind_emu()
    m = UNet2DConditionModel(model_util.tiny_config()).float()
    m.requires_grad_(False)
    m.set_attention_maps(_tok_w())
    g = torch.Generator().manual_seed(1)
    with pytest.raises(NotImplementedError, match="float32"):
        with torch.no_grad():
            m(torch.randn(2, 4, HW, HW, generator=g), torch.tensor(10), encoder_hidden_states=torch.randn(2, 77, 64, generator=g))
    with pytest.raises(NotImplementedError, match="float32"):
        m.engine().plan(2, HW, HW, need_bwd=False, attn_maps=2)


def test_maps_plan_refusals():
    from conftest import _bind_emu
    _bind_emu()
    m = UNet2DConditionModel(model_util.tiny_config()).to(bf)
    eng = m.engine()
    with pytest.raises(ValueError):
        eng.plan(2, HW, HW, need_bwd=True, attn_maps=2)
    with pytest.raises(ValueError):
        eng.plan(2, HW, HW, need_bwd=False, share=2, attn_maps=2)
    with pytest.raises(ValueError):
        eng.plan(2, HW, HW, need_bwd=False, attn_maps=9)
    with pytest.raises(ValueError):
        eng.plan(3, HW, HW, need_bwd=False, attn_maps=2)
    with pytest.raises(ValueError):
        m.set_attention_maps(torch.zeros(2, 76))


def test_token_weights(tmp_path):
    """A multi-token word, `#i-j`, a missing word -- with a synthetic BPE vocabulary (single letters: a word of n letters is n
    tokens), as the front-end test of tests/test_unet.py builds it."""
    from test_host import _write_synthetic_clip
    from transformers import CLIPTokenizer
    folder = str(tmp_path / "model")
    _write_synthetic_clip(folder)
    tok = CLIPTokenizer.from_pretrained(os.path.join(folder, "tokenizer"))
    tw, where = attn_maps.token_weights(tok, "a cat on a mat", ["cat", "a", "#3-5", "#76"])
    # row: <start> a | c a t | o n | a | m a t <end>...
    assert where[0] == [2, 3, 4] and where[1] == [1, 7] and where[2] == [3, 4, 5] and where[3] == [76]
    assert tuple(tw.shape) == (4, 77) and tw[0].sum() == 3 and tw[1].sum() == 2 and tw[0, 2:5].tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="dog"):
        attn_maps.token_weights(tok, "a cat on a mat", ["dog"])
    with pytest.raises(ValueError):
        attn_maps.token_weights(tok, "a cat", ["#77"])
    # synthetic:* models have no token ids: raw positions work, words say what to do
    stw, swhere = attn_maps.token_weights(model_util.SyntheticTokenizer(), "a cat", ["#2"])
    assert swhere == [[2]] and stw[0, 2] == 1
    with pytest.raises(ValueError, match="#3"):
        attn_maps.token_weights(model_util.SyntheticTokenizer(), "a cat", ["cat"])


# ---- the sampling scripts -----------------------------------------------------------------------------------------------------
def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _png_size(path):
    with open(path, "rb") as fh:
        head = fh.read(33)
    return struct.unpack(">IIBB", head[16:26])


def test_infer_attn_map_writes_the_sheet_and_the_json(dev, tmp_path):
    mod = _script("infer")
    unet = model_util.load_models("synthetic:tiny", "ddim")[2]
    with _quiet():
        net = LoRANetwork(unet.to(dev, bf), rank=4, multiplier=1.0, alpha=1.0)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for l in net.unet_loras:
            l.lora_up.weight.copy_(torch.randn(l.lora_up.weight.shape, generator=g) * 0.3)
    f = str(tmp_path / "x_last.safetensors")
    net.save_weights(f, dtype=torch.float32)
    sheet, out = str(tmp_path / "s.png"), str(tmp_path / "latents.safetensors")
    base = ["--model", "synthetic:tiny", "--height", "64", "--width", "64", "--steps", "2", "--device", str(dev), "--no_graphs", "--out", out]
    with _quiet():
        mod.main(base + ["--lora", f, "--lora_scales", "-1,0,1", "--image", sheet, "--attn_map", "#2", "--attn_map", "#3-4",
                         "--clip_score", "a photo"])
    assert _png_size(sheet) == (192, 64, 8, 2)
    # the sheet layout once per word, top to bottom
    assert _png_size(str(tmp_path / "s.attn.png")) == (192, 128, 8, 2)
    with open(str(tmp_path / "s.attn.json")) as fh:
        doc = json.load(fh)
    with open(str(tmp_path / "s.scores.json")) as fh:
        scores = json.load(fh)
    assert doc["words"] == ["#2", "#3-4"] and doc["token_positions"] == [[2], [3, 4]]
    assert doc["strengths"] == scores["strengths"] == [[-1.0], [0.0], [1.0]]              # the same cell order
    mh = torch.tensor(doc["mean_heat"])
    assert tuple(mh.shape) == (3, 2) and bool((mh > 0).all()) and not torch.equal(mh[0], mh[2])
    # without a sweep: one picture per word
    one = str(tmp_path / "one.png")
    with _quiet():
        mod.main(base + ["--image", one, "--attn_map", "#2"])
    assert _png_size(str(tmp_path / "one.attn.png")) == (64, 64, 8, 2)
    with open(str(tmp_path / "one.attn.json")) as fh:
        assert json.load(fh)["strengths"] == [None]
    with pytest.raises(SystemExit):
        with contextlib.redirect_stderr(io.StringIO()):
            mod.main(base + ["--attn_map", "#2"])             # needs --image


def test_infer_xl_attn_map(dev, tmp_path):
    mod = _script("infer_xl")
    img = str(tmp_path / "x.png")
    with _quiet():
        mod.main(["--model", "synthetic:tiny_xl", "--height", "64", "--width", "64", "--steps", "2", "--device", str(dev), "--no_graphs",
                  "--out", str(tmp_path / "l.safetensors"), "--image", img, "--attn_map", "#1"])
    assert _png_size(str(tmp_path / "x.attn.png")) == (64, 64, 8, 2)
    with open(str(tmp_path / "x.attn.json")) as fh:
        doc = json.load(fh)
    assert doc["token_positions"] == [[1]] and doc["mean_heat"][0][0] > 0


if __name__ == "__main__":
    import sys
    assert sys.argv[1:] == ["graph_replay"], sys.argv
    from conftest import _bind_hip
    _bind_hip()
    _check_graph_replay(torch.device("cuda:0"))
    torch.cuda.synchronize()
    print("graph replay ok")
