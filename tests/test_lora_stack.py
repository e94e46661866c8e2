"""Stacked LoRA files: `LoRANetwork.from_files` / `LoRAStack` (fixed per-file multipliers, per-sample strength rows, merged
export), the sweep plans of a stack (`leco_lora_rowscale_stack` at every LoRA site) and the repeated `--lora` /
`--lora_scales` / `--lora_multipliers` of the two sampling scripts -- on the host emulator (CPU tier) and on gfx950 (`-m gpu`).

The oracle is oracle/lora_ref.py as it is: two `LoRANetworkRef` built one after the other on the same oracle UNet (each wraps
the forward it finds -- the reference's own way of applying two LoRAs).  File A: lierla, rank 4, alpha 1; file B: c3lier, rank
8, alpha 4.  Tolerance: nothing fixed in advance -- 1.5 x the larger relative L2 of the EXISTING single-file path
(`LoRANetwork.from_file`, fixed `multiplier`, each file alone) from the oracle, measured in the same process; the margin covers
the two extra bf16 roundings of a stack (the scaled `up` block, T . s).  Measured values: DESIGN.md section 7 "Stacked LoRA
files"."""
import contextlib
import importlib.util
import io
import itertools
import os
import struct

import pytest
import torch
from safetensors.torch import load_file, save_file

from conftest import rel_err
from leco_amd import model_util
from leco_amd.lora import DEFAULT_TARGET_REPLACE, UNET_TARGET_REPLACE_MODULE_CONV, LoRANetwork, LoRAStack
from leco_amd.unet import UNet2DConditionModel
from oracle import lora_ref
from oracle import unet_ref as R

bf = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3LIER = list(DEFAULT_TARGET_REPLACE) + list(UNET_TARGET_REPLACE_MODULE_CONV)
FILES = ((4, 1.0, list(DEFAULT_TARGET_REPLACE)), (8, 4.0, C3LIER))       # (rank, alpha, targets) of file A and file B
# LoRA magnitude (std of lora_down and lora_up) per file: large enough that, on the oracle alone, every non-vacuity
# comparison below exceeds 10 x the tolerance, small enough that the output stays in the range of the LoRA-off network
MAG = (0.2, 0.04)
AB = (-1.5, 2.0)                                       # the fixed multipliers (a, b): a != b, both non-zero
GRID = tuple(itertools.product((-1.5, 1.0), (0.0, 2.0)))  # the strength rows of the grid test, first file slowest


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


class _World:
    """One oracle UNet with its two reference LoRAs, the HIP UNet on the same bf16-rounded weights, the two files, and the
    oracle outputs computed so far.  Built once per (device, model) and shared by the tests; the gold values never change."""

    def __init__(self, dev, xl, folder):
        self.dev, self.xl = dev, xl
        ref = R.init_synthetic_(R.UNet2DConditionModel(R.tiny_config(xl=xl)), seed=1234 if not xl else 3)
        with torch.no_grad():
            for p in ref.parameters():
                p.copy_(p.to(bf).float())
        ref.requires_grad_(False)
        m = UNet2DConditionModel(model_util.tiny_xl_config() if xl else model_util.tiny_config())
        m.load_state_dict(ref.state_dict())
        self.ref, self.m = ref, m.to(dev, bf)
        self.m.requires_grad_(False)
        self.rnets, self.paths = [], []
        g = torch.Generator().manual_seed(11)
        for j, ((rank, alpha, targets), mag) in enumerate(zip(FILES, MAG)):
            with _quiet():
                rnet = lora_ref.LoRANetworkRef(ref, rank=rank, alpha=alpha, targets=targets)
                net = LoRANetwork(self.m, rank=rank, alpha=alpha, target_replace_modules=targets)
            assert [l.lora_name for l in rnet.unet_loras] == [l.lora_name for l in net.unet_loras]
            with torch.no_grad():
                for rl, l in zip(rnet.unet_loras, net.unet_loras):
                    d = (torch.randn(rl.lora_down.weight.shape, generator=g) * mag).to(bf).float()
                    u = (torch.randn(rl.lora_up.weight.shape, generator=g) * mag).to(bf).float()
                    rl.lora_down.weight.copy_(d); rl.lora_up.weight.copy_(u)
                    l.lora_down.weight.copy_(d.reshape(l.lora_down.weight.shape)); l.lora_up.weight.copy_(u.reshape(l.lora_up.weight.shape))
            path = os.path.join(str(folder), f"file{'ab'[j]}{'_xl' if xl else ''}.safetensors")
            net.save_weights(path, dtype=torch.float32)
            self.rnets.append(rnet)
            self.paths.append(path)
        gi = torch.Generator().manual_seed(5)
        self.x = torch.randn(1, 4, 16, 16, generator=gi).to(bf)
        self.ctx = torch.randn(2, 77, 64, generator=gi).to(bf)                 # [uncond; cond]
        self.extra = None
        if xl:
            self.extra = {"text_embeds": torch.randn(2, 64, generator=gi).to(bf), "time_ids": torch.tensor([[128., 128, 0, 0, 128, 128]] * 2)}
        self._gold = {}
        self._tol = None

    def gold(self, a, b):
        """The oracle at multipliers (a, b): [2 = uncond, cond][4][16][16]."""
        if (a, b) not in self._gold:
            for rnet, s in zip(self.rnets, (a, b)):
                for l in rnet.unet_loras:
                    l.multiplier = s
            kw = {} if self.extra is None else {"added_cond_kwargs": {k: v.float() for k, v in self.extra.items()}}
            with torch.no_grad():
                self._gold[(a, b)] = self.ref(self.x.repeat(2, 1, 1, 1).float(), torch.tensor(500), encoder_hidden_states=self.ctx.float(),
                                              **kw).sample
        return self._gold[(a, b)]

    def call(self, n):
        """One CFG-doubled pass over n copies of the sample: batch [uncond x n; cond x n] (train_util.predict_noise)."""
        dev, kw = self.dev, {}
        if self.extra is not None:
            kw["added_cond_kwargs"] = {k: v.repeat_interleave(n, 0).to(dev) for k, v in self.extra.items()}
        with torch.no_grad():
            y = self.m(self.x.repeat(2 * n, 1, 1, 1).to(dev), torch.tensor(500),
                       encoder_hidden_states=self.ctx.repeat_interleave(n, 0).to(dev), **kw).sample
        return y.float().cpu()

    def tol(self):
        """1.5 x the larger relative L2 of the existing single-file path from the oracle: file A alone at multiplier a, file
        B alone at multiplier b."""
        if self._tol is None:
            errs = []
            for j, s in enumerate(AB):
                net = LoRANetwork.from_file(self.m, self.paths[j], multiplier=s)
                pair = (s, 0.0) if j == 0 else (0.0, s)
                errs.append(rel_err(self.call(1), self.gold(*pair)))
                del net
            self.single = errs
            self._tol = 1.5 * max(errs)
            print(f"stack parity {'xl' if self.xl else 'sd'} [{self.dev.type}]: single file vs oracle A@{AB[0]} {errs[0]:.4g}, "
                  f"B@{AB[1]} {errs[1]:.4g} -> tolerance {self._tol:.4g}")
        return self._tol


_worlds = {}


def _world(dev, xl, tmp_path) -> _World:
    key = (dev.type, xl)
    if key not in _worlds:
        _worlds[key] = _World(dev, xl, tmp_path)
    return _worlds[key]


def _samples(y, n):
    return [torch.stack([y[i], y[n + i]]) for i in range(n)]


XL = pytest.mark.parametrize("xl", [False, True], ids=["sd", "xl"])


@XL
def test_fixed_multipliers_match_the_oracle(dev, tmp_path, xl):
    """The stack at `set_multipliers((a, b))` == two reference LoRAs at (a, b); on the oracle alone a dropped file, swapped
    strengths or a wrong scale move the output by >= 10 x the tolerance."""
    w = _world(dev, xl, tmp_path)
    a, b = AB
    tol = w.tol()
    stack = LoRANetwork.from_files(w.m, w.paths)
    assert isinstance(stack, LoRAStack) and stack.lora_dim == 12 and stack.alpha == 12.0
    assert stack.col_file == [0] * 4 + [1] * 8
    stack.set_multipliers((a, b))
    y = w.call(1)
    assert not any(k[-1] == "sweep" for k in w.m.engine().plans)
    err = rel_err(y, w.gold(a, b))
    moved = {"(a,b) vs (0,0)": rel_err(w.gold(a, b), w.gold(0.0, 0.0)), "(a,0) vs (0,b)": rel_err(w.gold(a, 0.0), w.gold(0.0, b)),
             "(a,b) vs (b,a)": rel_err(w.gold(a, b), w.gold(b, a))}
    print(f"stack fixed multipliers {'xl' if xl else 'sd'} [{dev.type}]: stack vs oracle {err:.4g}, tolerance {tol:.4g}, oracle moved by "
          + ", ".join(f"{k} {v:.4g}" for k, v in moved.items()))
    for k, v in moved.items():
        assert v >= 10 * tol, (k, v, tol)
    assert err <= tol, (err, tol)
    # a constructor argument is the same as the setter; the default is all 1
    again = LoRANetwork.from_files(w.m, w.paths, multipliers=(a, b))
    assert torch.equal(again.slab.detach().cpu(), stack.slab.detach().cpu())
    ones = LoRANetwork.from_files(w.m, w.paths)
    assert rel_err(w.call(1), w.gold(1.0, 1.0)) <= tol
    with ones:                               # `with stack:` / `multiplier` keep their on / off meaning
        pass
    assert rel_err(w.call(1), w.gold(0.0, 0.0)) <= tol


@XL
def test_grid_in_one_batch_matches_the_oracle_and_the_fixed_passes(dev, tmp_path, xl):
    """(-1.5, 1) x (0, 2): n = 4 in one CFG-doubled batch of 8 == the oracle at each pair == the stack's own
    fixed-multiplier pass at that pair, through a plan keyed with the sweep tag."""
    w = _world(dev, xl, tmp_path)
    tol = w.tol()
    stack = LoRANetwork.from_files(w.m, w.paths)
    fixed = []
    for pair in GRID:
        stack.set_multipliers(pair)
        fixed.append(w.call(1))
    assert not any(k[-1] == "sweep" for k in w.m.engine().plans)
    stack.set_multipliers((0.5, 0.25))      # (ignored while strengths are set)
    stack.set_strengths(GRID)
    n = len(GRID)
    sweep = _samples(w.call(n), n)
    keys = [k for k in w.m.engine().plans if k[-1] == "sweep"]
    assert keys and w.m.engine().plans[keys[0]].strengths.shape == (2 * n, 2), list(w.m.engine().plans)
    e_gold = [rel_err(s, w.gold(*pair)) for s, pair in zip(sweep, GRID)]
    e_fixed = [rel_err(s, f) for s, f in zip(sweep, fixed)]
    print(f"stack grid {'xl' if xl else 'sd'} [{dev.type}]: sweep vs oracle {['%.4g' % e for e in e_gold]}, sweep vs fixed passes "
          f"{['%.4g' % e for e in e_fixed]}, tolerance {tol:.4g}")
    for i, pair in enumerate(GRID):
        assert e_gold[i] <= tol, (pair, e_gold[i], tol)
        assert e_fixed[i] <= tol, (pair, e_fixed[i], tol)
    # the cells differ on the oracle by far more than the tolerance: a strength of the wrong cell or file would show
    assert min(rel_err(w.gold(*p), w.gold(*q)) for p, q in itertools.combinations(GRID, 2)) >= 10 * tol
    stack.set_strengths(None)               # back to the multipliers set above
    assert rel_err(w.call(1), w.gold(0.5, 0.25)) <= tol


def test_strength_rows_change_between_graph_replays_without_a_repack(dev, tmp_path):
    """Capture once, replay at one strength matrix, write another into the buffer, replay: equals an eager run at the second
    matrix; no re-pack, no new plan, no new graph.  On the GPU the capture runs in an interpreter of its own, like
    tests/test_lora_sweep.py's replay test and for its reason."""
    if dev.type == "cuda":
        import subprocess
        import sys
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "graph_replay", str(tmp_path)], capture_output=True, text=True,
                           timeout=300, cwd=ROOT)
        assert r.returncode == 0 and "graph replay ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        return
    _check_graph_replay(_world(dev, False, tmp_path))


def _check_graph_replay(w):
    m = w.m
    stack = LoRANetwork.from_files(m, w.paths)
    first, second = ((1.0, 1.0), (1.0, 1.0)), ((-1.0, 2.0), (0.5, -1.5))
    m.use_graphs = True
    try:
        stack.set_strengths(first)
        y1 = w.call(2)
        plans = dict(m.engine().plans)
        plan = next(p for k, p in plans.items() if k[-1] == "sweep")
        packed, graph = stack._packed_version, plan.graphs.get("fwd_on")
        if w.dev.type == "cuda":
            assert graph is not None
        stack.set_strengths(second)
        assert not stack.needs_repack()
        y_replay = w.call(2)
        assert not stack.needs_repack() and stack._packed_version == packed
        assert m.engine().plans == plans and plan.graphs.get("fwd_on") is graph and len(plan.graphs) <= 1
        assert torch.equal(plan.strengths.cpu(), torch.tensor(second * 2))
    finally:
        m.use_graphs = False
    y_eager = w.call(2)
    assert torch.equal(y_replay, y_eager)
    assert rel_err(y_replay, y1) > 1e-2
    m.release()


def test_from_files_interface(dev, tmp_path):
    w = _world(dev, False, tmp_path)
    m, (fa, fb) = w.m, w.paths
    # one file == from_file
    for f, (rank, alpha, _) in zip((fa, fb), FILES):
        one, ref = LoRANetwork.from_files(m, [f]), None
        slab = one.slab.detach().cpu().clone()
        assert (one.lora_dim, one.alpha, one.col_file, one.multipliers) == (rank, alpha, [0] * rank, (1.0,))
        ref = LoRANetwork.from_file(m, f)
        assert torch.equal(slab, ref.slab.detach().cpu()) and (ref.lora_dim, ref.alpha) == (rank, alpha)
        assert [l.lora_name for l in one.unet_loras] == [l.lora_name for l in ref.unet_loras]
    # lierla + c3lier -> the c3lier coverage, whatever the order; the column blocks follow the order of the files
    with _quiet():
        c3 = [l.lora_name for l in LoRANetwork(m, rank=4, target_replace_modules=C3LIER).unet_loras]
    ba = LoRANetwork.from_files(m, [fb, fa])
    assert [l.lora_name for l in ba.unet_loras] == c3 and ba.col_file == [0] * 8 + [1] * 4
    ab = LoRANetwork.from_files(m, [fa, fb])
    assert [l.lora_name for l in ab.unet_loras] == c3 and (ab.lora_dim, ab.alpha) == (12, 12.0)
    sa, sb = load_file(fa), load_file(fb)
    conv_only = next(l for l in ab.unet_loras if l.lora_name + ".alpha" not in sa)
    both = next(l for l in ab.unet_loras if l.lora_name + ".alpha" in sa)
    assert conv_only.lora_down.weight[:4].abs().max() == 0 and conv_only.lora_up.weight[:, :4].abs().max() == 0
    n = both.lora_name
    assert torch.equal(both.lora_down.weight[:4].cpu(), sa[n + ".lora_down.weight"])
    assert torch.equal(both.lora_down.weight[4:].cpu(), sb[n + ".lora_down.weight"])
    assert torch.equal(both.lora_up.weight[:, :4].cpu(), sa[n + ".lora_up.weight"] * (1.0 / 4))          # alpha_j / r_j, in fp32
    assert torch.equal(both.lora_up.weight[:, 4:].cpu(), sb[n + ".lora_up.weight"] * (4.0 / 8))
    assert abs(both.scale - 1.0) < 1e-12
    # errors
    with pytest.raises(ValueError, match="no files"):
        LoRANetwork.from_files(m, [])
    mixed = dict(sa)
    names = sorted(k[:-len(".lora_down.weight")] for k in mixed if k.endswith(".lora_down.weight"))
    mixed[names[3] + ".lora_down.weight"] = torch.cat([mixed[names[3] + ".lora_down.weight"]] * 2, 0)
    mixed[names[3] + ".lora_up.weight"] = torch.cat([mixed[names[3] + ".lora_up.weight"]] * 2, 1)
    f = str(tmp_path / "mixed.safetensors")
    save_file({k: v.contiguous() for k, v in mixed.items()}, f)
    with pytest.raises(ValueError, match="not uniform"):
        LoRANetwork.from_files(m, [fb, f])
    # 8 + 60 columns are wider than the 64-channel modules of the tiny UNet
    with _quiet():
        wide = LoRANetwork(m, rank=60, alpha=1.0)
    f = str(tmp_path / "wide.safetensors")
    wide.save_weights(f, dtype=torch.float32)
    with pytest.raises(ValueError, match="wider than lora_unet_") as ei:
        LoRANetwork.from_files(m, [fb, f])
    assert "68" in str(ei.value)
    stack = LoRANetwork.from_files(m, [fa, fb])
    for bad in ((1.0,), (1.0, 2.0, 3.0), (1.0, float("nan"))):
        with pytest.raises(ValueError, match="set_multipliers"):
            stack.set_multipliers(bad)
    with pytest.raises(ValueError, match="2 strengths per sample"):
        stack.set_strengths([(1.0, 2.0), (1.0,)])
    with pytest.raises(ValueError, match="plain number"):
        stack.set_strengths([0.0, 1.0])
    with pytest.raises(ValueError):
        stack.set_strengths([])
    with pytest.raises(ValueError):
        stack.set_strengths([(1.0, float("inf"))])
    assert stack.strengths is None
    LoRANetwork.from_files(m, [fa]).set_strengths([0.0, 1.0])          # one file: plain floats are accepted
    stack = LoRANetwork.from_files(m, [fa, fb])
    stack.set_strengths([(1.0, 0.0), (0.0, 1.0), (1.0, 1.0)])
    with pytest.raises(ValueError, match="multiple"):
        w.call(2)                                                        # a batch of 4 at 3 rows


def test_stack_strengths_on_a_float32_model_are_refused(tmp_path):
    """The fp32 compute mode has no sweep variant; fixed multipliers work there, because a stack is an ordinary network."""
    from conftest import _bind_emu
    _bind_emu()
    w = _world(torch.device("cpu"), False, tmp_path)
    m = UNet2DConditionModel(model_util.tiny_config())
    m.load_state_dict(w.ref.state_dict())
    m = m.float()
    m.requires_grad_(False)
    stack = LoRANetwork.from_files(m, w.paths, multipliers=AB)
    with torch.no_grad():
        y = m(w.x.repeat(2, 1, 1, 1).float(), torch.tensor(500), encoder_hidden_states=w.ctx.float()).sample
    assert rel_err(y, w.gold(*AB)) < 1e-4          # fp32 against fp32: only the summation order differs
    stack.set_strengths(GRID)
    with pytest.raises(NotImplementedError, match="float32"):
        with torch.no_grad():
            m(w.x.repeat(8, 1, 1, 1).float(), torch.tensor(500), encoder_hidden_states=w.ctx.repeat_interleave(4, 0).float())


def test_merged_export_is_a_normal_lora_file(dev, tmp_path):
    w = _world(dev, False, tmp_path)
    tol = w.tol()
    stack = LoRANetwork.from_files(w.m, w.paths, multipliers=AB)
    y_stack = w.call(1)
    slab = stack.slab.detach().cpu().clone()
    stack.set_strengths(GRID)                 # (the export folds the MULTIPLIERS in, also while strengths are set)
    f = str(tmp_path / "merged.safetensors")
    stack.save_weights(f, dtype=torch.float32)
    sd = load_file(f)
    assert all(float(v) == 12.0 for k, v in sd.items() if k.endswith(".alpha"))
    merged = LoRANetwork.from_file(w.m, f)
    assert type(merged) is LoRANetwork and (merged.lora_dim, merged.alpha) == (12, 12.0)
    assert torch.equal(merged.slab.detach().cpu(), slab)
    y = w.call(1)
    print(f"merged export [{dev.type}]: merged file vs stack {rel_err(y, y_stack):.4g}, vs oracle {rel_err(y, w.gold(*AB)):.4g}, "
          f"tolerance {tol:.4g}")
    assert rel_err(y, y_stack) <= tol and rel_err(y, w.gold(*AB)) <= tol


# ---- the sampling scripts -----------------------------------------------------------------------------------------------------
def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("script,model", [("infer", "synthetic:tiny"), ("infer_xl", "synthetic:tiny_xl")])
def test_infer_scripts_stack_two_files(dev, tmp_path, script, model):
    mod = _script(script)
    unet = (model_util.load_models_xl if script == "infer_xl" else model_util.load_models)(model, "ddim")[2].to(dev, bf)
    g = torch.Generator().manual_seed(3)
    files = []
    for j, (rank, alpha, targets) in enumerate(FILES):
        with _quiet():
            net = LoRANetwork(unet, rank=rank, multiplier=1.0, alpha=alpha, target_replace_modules=targets)
        with torch.no_grad():
            for l in net.unet_loras:
                l.lora_up.weight.copy_(torch.randn(l.lora_up.weight.shape, generator=g) * 0.3)
        files.append(str(tmp_path / f"file{j}.safetensors"))
        net.save_weights(files[-1], dtype=torch.float32)
    sheet, out = str(tmp_path / "sheet.png"), str(tmp_path / "latents.safetensors")
    base = ["--model", model, "--height", "128", "--width", "128", "--steps", "2", "--device", str(dev), "--no_graphs", "--out", out]
    two = ["--lora", files[0], "--lora", files[1]]
    sa, sb = (-1.0, 1.0), (0.0, 1.0, 2.0)
    with _quiet():
        lat = mod.main(base + two + ["--lora_scales", "-1,1", "--lora_scales", "0,1,2", "--image", sheet]).float().cpu()
    with open(sheet, "rb") as fh:
        head = fh.read(33)
    assert struct.unpack(">IIBB", head[16:26]) == (3 * 128, 2 * 128, 8, 2)     # n_2 pictures wide, n_1 high, 8-bit RGB
    assert tuple(load_file(out)["latents"].shape) == (6, 4, 16, 16) and lat.shape == (6, 4, 16, 16)
    # cell (i, j) is the run at fixed multipliers (a_i, b_j): nearer to it than any other cell is (another launch plan: bf16
    # rounding apart -- the comparison tests/test_lora_sweep.py makes for its strength-1 panel)
    for (i, a), (j, b) in itertools.product(enumerate(sa), enumerate(sb)):
        with _quiet():
            fixed = mod.main(base + two + ["--lora_multipliers", f"{a},{b}"]).float().cpu()
        assert fixed.shape == (1, 4, 16, 16)
        d = [rel_err(lat[c], fixed[0]) for c in range(6)]
        assert min(range(6), key=d.__getitem__) == 3 * i + j, ((a, b), d)
    # one --lora with one --lora_scales behaves as before: [n, 4, h, w] from the single-file network
    with _quiet():
        one = mod.main(base + ["--lora", files[0], "--lora_scales", "-1,0,1"]).float().cpu()
        plain = mod.main(base + ["--lora", files[0]]).float().cpu()
    assert one.shape == (3, 4, 16, 16) and plain.shape == (1, 4, 16, 16)
    assert rel_err(one[2], plain[0]) < rel_err(one[1], plain[0]) and rel_err(one[2], plain[0]) < rel_err(one[0], plain[0])
    for bad in (two + ["--lora_scales", "-1,1"], ["--lora", files[0], "--lora_scales", "-1,1", "--lora_scales", "0,1"],
                two + ["--lora_multipliers", "1"], two + ["--rank", "4"]):
        with pytest.raises(SystemExit):
            with contextlib.redirect_stderr(io.StringIO()):
                mod.main(base + bad)


if __name__ == "__main__":
    import sys
    assert sys.argv[1] == "graph_replay" and len(sys.argv) == 3, sys.argv
    from conftest import _bind_hip
    _bind_hip()
    _check_graph_replay(_World(torch.device("cuda:0"), False, sys.argv[2]))
    torch.cuda.synchronize()
    print("graph replay ok")
