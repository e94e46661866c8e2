"""LoRA adapter network for the MI355X UNet engine.

Mirrors the reference's ``lora.py`` interface -- ``LoRANetwork(unet, rank, multiplier, alpha,
train_method)``, ``prepare_optimizer_params()``, ``save_weights(file, dtype, metadata)``, the
``with network:`` on/off switch (lora.py:110-237) -- and reproduces its module discovery, key
names, tensor shapes and init (lora.py:49-95,158-199) so the emitted ``.safetensors`` drop into
the reference tooling / webui unchanged.

What is different is the storage: instead of monkey-patching ``org_module.forward``
(lora.py:97-106) with five tiny kernels per module, all LoRA matrices live in ONE flat fp32
slab (plus a bf16 shadow the MFMA kernels read and a flat fp32 gradient slab), and the UNet
engine fuses ``up(down(x)) * multiplier * scale`` into the base GEMM as an extra K tile.  The
per-module ``lora_down.weight`` / ``lora_up.weight`` Parameters are views into the slab, so
``torch.optim`` optimizers, ``state_dict()`` and the fused AdamW kernel all see the same memory,
and the data-parallel gradient exchange is a single all-reduce of the gradient slab.
"""
from __future__ import annotations

import math
import os
from typing import List, Literal, Optional

import torch
import torch.nn as nn
from safetensors.torch import save_file

from . import ops

UNET_TARGET_REPLACE_MODULE_TRANSFORMER = ["Transformer2DModel"]
UNET_TARGET_REPLACE_MODULE_CONV = ["ResnetBlock2D", "Downsample2D", "Upsample2D"]  # locon / c3lier
LORA_PREFIX_UNET = "lora_unet"
DEFAULT_TARGET_REPLACE = UNET_TARGET_REPLACE_MODULE_TRANSFORMER

TRAINING_METHODS = Literal["noxattn", "innoxattn", "selfattn", "xattn", "full"]


class LoRAModule(nn.Module):
    """Holds one (lora_down, lora_up, alpha) triple.  Shapes follow lora.py:62-88."""

    def __init__(self, lora_name: str, leaf_name: str, org_module: nn.Module, multiplier=1.0, lora_dim=4, alpha=1):
        super().__init__()
        self.lora_name = lora_name
        self.leaf_name = leaf_name
        self.lora_dim = lora_dim
        cls = org_module.__class__.__name__
        if cls == "Linear":
            in_dim, out_dim = org_module.in_features, org_module.out_features
            self.lora_down = nn.Linear(in_dim, lora_dim, bias=False)
            self.lora_up = nn.Linear(lora_dim, out_dim, bias=False)
        elif cls == "Conv2d":
            in_dim, out_dim = org_module.in_channels, org_module.out_channels
            self.lora_dim = min(self.lora_dim, in_dim, out_dim)
            if self.lora_dim != lora_dim:
                print(f"{lora_name} dim (rank) is changed to: {self.lora_dim}")
            self.lora_down = nn.Conv2d(in_dim, self.lora_dim, org_module.kernel_size, org_module.stride,
                                       org_module.padding, bias=False)
            self.lora_up = nn.Conv2d(self.lora_dim, out_dim, (1, 1), (1, 1), bias=False)
        else:
            raise ValueError(f"unsupported LoRA target class {cls}")
        if isinstance(alpha, torch.Tensor):
            alpha = alpha.detach().float().item()
        alpha = lora_dim if alpha is None or alpha == 0 else alpha
        self.scale = alpha / self.lora_dim
        self.register_buffer("alpha", torch.tensor(alpha))
        nn.init.kaiming_uniform_(self.lora_down.weight, a=math.sqrt(5))
        nn.init.zeros_(self.lora_up.weight)
        self.multiplier = multiplier
        self.down_off = self.up_off = -1  # element offsets into the network slab


def _discover(prefix, root_module, target_replace_modules, train_method):
    """Module discovery of the reference (lora.py:158-199, including its name-filter semantics): yields
    (leaf qualified name, lora name, leaf module) in network order."""
    for name, module in root_module.named_modules():
        if train_method == "noxattn":
            if "attn2" in name or "time_embed" in name:
                continue
        elif train_method == "innoxattn":
            if "attn2" in name:
                continue
        elif train_method == "selfattn":
            if "attn1" not in name:
                continue
        elif train_method == "xattn":
            if "attn2" not in name:
                continue
        elif train_method == "full":
            pass
        else:
            raise NotImplementedError(f"train_method: {train_method} is not implemented.")
        if module.__class__.__name__ in target_replace_modules:
            for child_name, child_module in module.named_modules():
                if child_module.__class__.__name__ in ["Linear", "Conv2d"]:
                    leaf = name + "." + child_name
                    yield leaf, (prefix + "." + leaf).replace(".", "_"), child_module


def _read_lora_file(file) -> dict:
    if os.path.splitext(str(file))[1] == ".safetensors":
        from safetensors.torch import load_file
        return load_file(str(file))
    return torch.load(file, map_location="cpu", weights_only=True)


class LoRANetwork(nn.Module):
    # per-sample strengths of the sampling path (`set_strengths`); None = the single `multiplier`
    strengths = None
    _strengths_version = 0

    def __init__(self, unet, rank: int = 4, multiplier: float = 1.0, alpha: float = 1.0,
                 train_method: TRAINING_METHODS = "full", target_replace_modules: Optional[List[str]] = None,
                 strict_reference: bool = False, strict_dtype: torch.dtype = torch.bfloat16) -> None:
        super().__init__()
        self.multiplier = multiplier
        self.lora_dim = rank
        self.alpha = alpha
        self.strict_reference = strict_reference
        self.strict_dtype = strict_dtype          # the precision `--strict_reference` rounds the parameters to (train.precision)
        targets = list(DEFAULT_TARGET_REPLACE if target_replace_modules is None else target_replace_modules)
        self.unet_loras: List[LoRAModule] = self.create_modules(LORA_PREFIX_UNET, unet, targets, rank, multiplier,
                                                               train_method)
        print(f"create LoRA for U-Net: {len(self.unet_loras)} modules.")
        names = set()
        for lora in self.unet_loras:
            assert lora.lora_name not in names, f"duplicated lora name: {lora.lora_name}. {names}"
            names.add(lora.lora_name)
        for lora in self.unet_loras:
            self.add_module(lora.lora_name, lora)
        self.version = 0
        self._packed_version = -1
        self._unet = [unet]  # not registered as a submodule
        self._build_slab(torch.device("cpu"))
        if hasattr(unet, "engine") and next(unet.parameters()).device.type != "meta":
            if unet.device != self.slab.device:
                self._adopt(self.slab.detach().to(unet.device))
            unet.engine().attach_lora(self)

    # ---- discovery (lora.py:158-199, including its name-filter semantics) ---------------------------
    def create_modules(self, prefix, root_module, target_replace_modules, rank, multiplier, train_method) -> list:
        return [LoRAModule(lora_name, leaf, child, multiplier, rank, self.alpha)
                for leaf, lora_name, child in _discover(prefix, root_module, target_replace_modules, train_method)]

    # ---- flat storage ---------------------------------------------------------------------------------
    def _build_slab(self, device) -> None:
        off = 0
        for lora in self.unet_loras:
            lora.down_off = off
            off += lora.lora_down.weight.numel()
            lora.up_off = off
            off += lora.lora_up.weight.numel()
        self.numel = off
        if self.unet_loras and self.unet_loras[0].lora_down.weight.device.type == "meta":
            self.slab = None   # shape-only instance (built under torch.device("meta")): names / census only
            return
        pad = (-off) % 64
        slab = torch.zeros(off + pad, dtype=torch.float32, device=device)
        for lora in self.unet_loras:
            for w, o in ((lora.lora_down.weight, lora.down_off), (lora.lora_up.weight, lora.up_off)):
                slab[o:o + w.numel()].copy_(w.detach().reshape(-1).float())
        self._adopt(slab)

    def _adopt(self, slab: torch.Tensor) -> None:
        dev = slab.device
        if self.strict_reference:  # reference keeps the parameters and the AdamW state in train.precision (train_lora.py:78,89)
            slab = slab.to(getattr(self, "strict_dtype", torch.bfloat16)).float()
        self.slab = slab.requires_grad_(True)         # autograd anchor of the engine's Function
        self.grad = torch.zeros_like(slab)
        self.shadow = slab.detach().to(torch.bfloat16)
        self.exp_avg = torch.zeros_like(slab)
        self.exp_avg_sq = torch.zeros_like(slab)
        self.hyper = torch.zeros(4, dtype=torch.float32, device=dev)
        data = slab.detach()
        for lora in self.unet_loras:
            for mod, o in ((lora.lora_down, lora.down_off), (lora.lora_up, lora.up_off)):
                shape = mod.weight.shape
                mod.weight.data = data[o:o + mod.weight.numel()].view(shape)
                mod.weight.grad = None
            lora.alpha = lora.alpha.to(dev)
        self._norm_buffers = None      # the device table of `weight_norms` / `apply_max_norm` follows the slab
        self.version += 1

    # ---- max-norm regularisation (leco_lora_max_norm) --------------------------------------------------------------
    def norm_buffers(self):
        """(table, norms, factors, stats) of `leco_lora_max_norm` on the slab's device: the module table (offsets, each
        module's own rank, K = the row length of `lora_down`, N = out, scale = alpha / r) uploaded once, and the kernel's
        three fp32 outputs.  Built on first use and again when the slab is re-adopted (`to`)."""
        if getattr(self, "_norm_buffers", None) is None:
            dev = self.slab.device
            rows = []
            for lora in self.unet_loras:
                dn, up = lora.lora_down.weight, lora.lora_up.weight
                rows.append((lora.down_off, lora.up_off, dn.shape[0], dn.numel() // dn.shape[0], up.shape[0], lora.scale))
            M = len(rows)
            self._norm_buffers = (ops.lora_norm_table(rows, dev), torch.zeros(M, dtype=torch.float32, device=dev),
                                  torch.ones(M, dtype=torch.float32, device=dev), torch.zeros(4, dtype=torch.float32, device=dev))
        return self._norm_buffers

    def _max_norm_op(self, max_norm: float):
        if self.strict_reference:
            raise ValueError("max-norm regularisation is not defined for --strict_reference networks (bf16 master weights)")
        table, norms, factors, stats = self.norm_buffers()
        return ops.lora_max_norm(self.slab.detach(), self.shadow, table, max_norm, norms, factors, stats)

    def weight_norms(self) -> dict:
        """{lora_name: scale * |lora_up lora_down|_F}: the Frobenius norm of every module's effective update at multiplier 1
        (for a 3x3 `lora_down`: of the composed convolution).  One measure-only launch; waits for the device."""
        self._max_norm_op(0.0).run()
        norms = self.norm_buffers()[1].cpu().tolist()
        return {lora.lora_name: v for lora, v in zip(self.unet_loras, norms)}

    def apply_max_norm(self, max_norm: float) -> dict:
        """Max-norm regularisation ("scale_weight_norms"): every module whose norm (`weight_norms`) exceeds ``max_norm`` has
        `lora_down` and `lora_up` multiplied by sqrt(max_norm / norm) each, in the fp32 slab and its bf16 shadow.  Returns
        ``dict(keys_scaled, avg_norm, max_norm, nonfinite)`` -- mean and maximum AFTER scaling over the modules with a
        finite norm; modules with a non-finite norm are left alone and counted.  Waits for the device."""
        if not float(max_norm) >= 0.0:
            raise ValueError(f"apply_max_norm: max_norm must be >= 0 (0: measure only), got {max_norm!r}")
        self._max_norm_op(float(max_norm)).run()
        k, avg, top, bad = self.norm_buffers()[3].cpu().tolist()
        if k > 0:
            self.mark_updated()
        return dict(zip(ops.WEIGHT_NORM_STATS_FIELDS, (int(k), avg, top, int(bad))))

    def to(self, *args, **kwargs):
        """Moves the slab; the fp32 master stays fp32 (the requested dtype only selects the
        compute/saved precision, which is bf16 on the MFMA path).  The reference's
        ``network.to(DEVICE, dtype=weight_dtype)`` call (train_lora.py:72-78) therefore works."""
        device = kwargs.get("device")
        for a in args:
            if isinstance(a, (str, torch.device)):
                device = a
        if device is not None and torch.device(device) != self.slab.device:
            self._adopt(self.slab.detach().to(device))
            unet = self._unet[0]
            if hasattr(unet, "engine") and torch.device(device).type != "meta":
                unet.engine().attach_lora(self)
        return self

    def attach_grads(self) -> None:
        """Expose the flat gradient slab as the per-parameter ``.grad`` views torch optimizers expect."""
        g = self.grad
        for lora in self.unet_loras:
            for mod, o in ((lora.lora_down, lora.down_off), (lora.lora_up, lora.up_off)):
                if mod.weight.grad is None:
                    mod.weight.grad = g[o:o + mod.weight.numel()].view(mod.weight.shape)

    def grads_cleared(self) -> bool:
        return self.unet_loras[0].lora_down.weight.grad is None

    def mark_updated(self) -> None:
        """Call after the LoRA parameters changed (optimizer step): the bf16 shadow and the packed
        MFMA operands are refreshed lazily before the next LoRA-on pass."""
        self.version += 1

    def sync_shadow(self) -> None:
        ops.cast_f32_bf16(self.slab.detach(), self.shadow, self.slab.numel()).run()

    # ---- reference API ----------------------------------------------------------------------------------
    def prepare_optimizer_params(self):
        all_params = []
        if self.unet_loras:
            params = []
            [params.extend(lora.parameters()) for lora in self.unet_loras]
            all_params.append({"params": params})
        return all_params

    def save_weights(self, file, dtype=None, metadata: Optional[dict] = None):
        state_dict = self.state_dict()
        if dtype is not None:
            for key in list(state_dict.keys()):
                state_dict[key] = state_dict[key].detach().clone().to("cpu").to(dtype)
        for key in list(state_dict.keys()):
            if not key.startswith("lora"):
                del state_dict[key]
        if os.path.splitext(str(file))[1] == ".safetensors":
            save_file({k: v.contiguous() for k, v in state_dict.items()}, str(file), metadata)
        else:
            torch.save(state_dict, file)

    def load_weights(self, file, strict: bool = True) -> None:
        """Inverse of `save_weights` (the reference has none): fills `lora_down` / `lora_up` from a file written by
        this package or by the reference (same key names, Appendix E); `alpha` must agree with the construction."""
        sd = _read_lora_file(file)
        own = self.state_dict()
        missing = [k for k in own if k.startswith("lora") and k not in sd]
        unexpected = [k for k in sd if k not in own]
        if strict and (missing or unexpected):
            raise KeyError(f"{file}: LoRA keys differ (missing {missing[:3]}, unexpected {unexpected[:3]})")
        with torch.no_grad():
            for k, v in sd.items():
                if k not in own:
                    continue
                if k.endswith(".alpha"):
                    if strict and abs(float(v) - float(own[k])) > 1e-6:
                        raise ValueError(f"{file}: {k} = {float(v)} but the network was built with {float(own[k])}")
                    continue
                own[k].copy_(v.to(own[k].dtype).reshape(own[k].shape))
        self.mark_updated()
        self.sync_shadow()

    def needs_repack(self) -> bool:
        """True when the packed MFMA operand images are older than the parameters."""
        return self._packed_version != self.version

    # ---- sampling: per-sample strengths, construction from a file -----------------------------------------
    def set_strengths(self, strengths) -> None:
        """Per-sample LoRA strengths for forward-only (sampling) passes: row b of a UNet batch runs at
        ``strengths[b % len(strengths)]`` -- with classifier-free guidance `predict_noise` doubles the batch as
        [uncond...; cond...], so the vector is tiled -- all in ONE pass over shared weights (bf16 only; the batch must be a
        whole multiple of ``len(strengths)``).  The on / off switch stays ``multiplier`` (`with network:`); its value is not
        applied on top.  ``None`` restores the single ``multiplier``."""
        if strengths is not None:
            strengths = tuple(float(v) for v in strengths)
            if not strengths or not all(math.isfinite(v) for v in strengths):
                raise ValueError(f"set_strengths: expected a non-empty sequence of finite floats, got {strengths}")
        self.strengths = strengths
        self._strengths_version += 1

    @staticmethod
    def _coverage(unet, names: set):
        """(target_replace_modules, train_method) whose module discovery on ``unet`` gives exactly ``names``."""
        seen = []
        for targets in (UNET_TARGET_REPLACE_MODULE_TRANSFORMER, UNET_TARGET_REPLACE_MODULE_TRANSFORMER + UNET_TARGET_REPLACE_MODULE_CONV):
            for method in ("full", "noxattn", "innoxattn", "selfattn", "xattn"):
                found = {ln for _, ln, _ in _discover(LORA_PREFIX_UNET, unet, targets, method)}
                if found == names:
                    return list(targets), method
                seen.append(len(found))
        raise ValueError(f"the file's {len(names)} LoRA modules match no (network type, train_method) coverage of this UNet "
                         f"(candidates have {sorted(set(seen))} modules)")

    @staticmethod
    def _scan_file(path):
        """(state dict, {module: rank}, the file's rank, the first module that has it, the file's alpha)."""
        sd = _read_lora_file(path)
        ranks = {k[:-len(".lora_down.weight")]: int(v.shape[0]) for k, v in sd.items() if k.endswith(".lora_down.weight")}
        if not ranks:
            raise ValueError(f"{path}: no `<module>.lora_down.weight` keys")
        alphas = {k[:-len(".alpha")]: float(v) for k, v in sd.items() if k.endswith(".alpha")}
        detected = max(ranks.values())
        first = next(n for n, r in ranks.items() if r == detected)
        return sd, ranks, detected, first, alphas.get(first, float(detected))

    @classmethod
    def from_file(cls, unet, path, multiplier: float = 1.0, rank: Optional[int] = None, alpha: Optional[float] = None,
                  **kwargs) -> "LoRANetwork":
        """A network built FROM a saved file (this package's `save_weights` or the reference's: same keys): rank =
        ``lora_down.weight.shape[0]``, alpha and the coverage (lierla / c3lier targets, ``train_method``) are read from the
        file's keys and tensors, then the weights are loaded.  One rank for the whole file (a convolution narrower than the
        rank keeps its clamped ``min(rank, in, out)``, lora.py:72-74); anything else raises ValueError.  ``rank`` / ``alpha``
        override what the file says (`load_weights` then raises where they contradict it)."""
        _, ranks, detected, first, file_alpha = cls._scan_file(path)
        rank = detected if rank is None else rank
        alpha = file_alpha if alpha is None else alpha
        targets, method = cls._coverage(unet, set(ranks))
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):      # (the constructor prints its census and every clamped conv)
            net = cls(unet, rank=rank, multiplier=multiplier, alpha=alpha, train_method=method, target_replace_modules=targets,
                      **kwargs)
        for lora in net.unet_loras:
            if rank == detected and ranks[lora.lora_name] != lora.lora_dim:
                raise ValueError(f"{path}: the ranks are not uniform: {first} has rank {rank}, {lora.lora_name} has rank "
                                 f"{ranks[lora.lora_name]} (expected {lora.lora_dim})")
        net.load_weights(path)
        return net

    def __enter__(self):
        self.multiplier = 1.0
        for lora in self.unet_loras:
            lora.multiplier = 1.0

    def __exit__(self, exc_type, exc_value, tb):
        self.multiplier = 0
        for lora in self.unet_loras:
            lora.multiplier = 0


    @staticmethod
    def from_files(unet, paths, multipliers=None, **kwargs) -> "LoRAStack":
        """Several saved LoRA files as ONE network (`LoRAStack`): the files sit side by side in the rank dimension."""
        return LoRAStack(unet, paths, multipliers, **kwargs)


def _union_coverage(unet, names: set):
    """The smallest discoverable (target_replace_modules, train_method) whose module set contains ``names``."""
    best = None
    for targets in (UNET_TARGET_REPLACE_MODULE_TRANSFORMER, UNET_TARGET_REPLACE_MODULE_TRANSFORMER + UNET_TARGET_REPLACE_MODULE_CONV):
        for method in ("full", "noxattn", "innoxattn", "selfattn", "xattn"):
            found = {ln: child for _, ln, child in _discover(LORA_PREFIX_UNET, unet, targets, method)}
            if names <= set(found) and (best is None or len(found) < len(best[2])):
                best = (list(targets), method, found)
    if best is None:
        raise ValueError(f"the files' {len(names)} LoRA modules fit no (network type, train_method) coverage of this UNet, "
                         f"e.g. {sorted(names)[0]}")
    return best


class LoRAStack(LoRANetwork):
    """F >= 1 LoRA files combined into one ordinary network for SAMPLING (`LoRANetwork.from_files`): the engine attaches,
    packs and runs it like a single-file network of rank R = sum of the files' ranks r_j.

    Column layout, the same in every module: file j owns columns ``off_j .. off_j + r_j`` of the rank dimension, ``off_j =
    r_0 + ... + r_(j-1)`` (`col_file`: column -> file).  The rows of `lora_down` in that block are file j's `lora_down` (zero
    where the file does not cover the module); the columns of `lora_up` are ``alpha_j / r_j . lora_up_j`` -- the files'
    scales differ, the packed operand images of a GEMM site carry ONE, so each file's own scale is folded into its block (in
    fp32, before the bf16 shadow is made) and the network is built with ``alpha = R``: a network-level scale of 1.  (One
    file: the network keeps the file's alpha and its `lora_up` as it is -- the same slab as `from_file`.)

    `set_multipliers`: one FIXED multiplier per file, folded into the `lora_up` blocks (a re-pack, no new plan or graph).
    `set_strengths`: per-SAMPLE rows of F strengths for the forward-only sweep plans (bf16 only); the blocks then carry only
    ``alpha_j / r_j``.  ``multiplier`` / ``with stack:`` stay the on / off switch.  `save_weights` writes the merged rank-R
    network (alpha = R, the multipliers folded in): a normal LoRA file."""

    def __init__(self, unet, paths, multipliers=None, **kwargs) -> None:
        paths = [paths] if isinstance(paths, (str, os.PathLike)) else list(paths)
        if not paths:
            raise ValueError("LoRANetwork.from_files: no files given")
        scans = [self._scan_file(p) for p in paths]
        file_ranks = [sc[2] for sc in scans]
        R = sum(file_ranks)
        # one file keeps its own alpha; several get alpha = R (network scale 1) and their own alpha / r inside `lora_up`
        net_alpha = float(scans[0][4]) if len(paths) == 1 else float(R)
        names = set().union(*(set(sc[1]) for sc in scans))
        targets, method, found = _union_coverage(unet, names)
        for ln, child in found.items():
            conv = child.__class__.__name__ == "Conv2d"
            width = min(child.in_channels, child.out_channels) if conv else min(child.in_features, child.out_features)
            if R > width:
                raise ValueError(f"LoRANetwork.from_files: the stacked rank {R} (= {' + '.join(map(str, file_ranks))}) is wider than "
                                 f"{ln} ({width} channels)")
        import contextlib
        import io
        kwargs.setdefault("multiplier", 1.0)
        with contextlib.redirect_stdout(io.StringIO()):      # (the constructor prints its census)
            super().__init__(unet, rank=R, alpha=net_alpha, train_method=method, target_replace_modules=targets, **kwargs)
        self.paths = [str(p) for p in paths]
        self.file_ranks = file_ranks
        self.file_alphas = [float(sc[4]) for sc in scans]
        self.col_file = [j for j, r in enumerate(file_ranks) for _ in range(r)]
        with torch.no_grad():
            off = 0
            for path, (sd, ranks, r_file, first, alpha), j in zip(paths, scans, range(len(paths))):
                for lora in self.unet_loras:
                    dn, up = lora.lora_down.weight, lora.lora_up.weight
                    if off == 0:
                        dn.zero_(); up.zero_()
                    if lora.lora_name not in ranks:
                        continue
                    # a convolution narrower than the file's rank keeps its clamped min(rank, in, out) (lora.py:72-74)
                    r_mod = min(r_file, dn.shape[1], up.shape[0]) if dn.ndim == 4 else r_file
                    if ranks[lora.lora_name] != r_mod:
                        raise ValueError(f"{path}: the ranks are not uniform: {first} has rank {r_file}, {lora.lora_name} has rank "
                                         f"{ranks[lora.lora_name]} (expected {r_mod})")
                    fd = sd[lora.lora_name + ".lora_down.weight"].float()
                    fu = sd[lora.lora_name + ".lora_up.weight"].float()
                    scale = (alpha / r_mod) / (net_alpha / R)
                    dn[off:off + r_mod].copy_(fd.reshape(dn[off:off + r_mod].shape))
                    up[:, off:off + r_mod].copy_((fu if scale == 1.0 else fu * scale).reshape(up[:, off:off + r_mod].shape))
                off += r_file
        self._base = self.slab.detach().clone()      # the blocks at multiplier 1: what `_fold` scales
        self._folded = (1.0,) * len(paths)
        self.multipliers = self._folded
        self.mark_updated()
        self.sync_shadow()
        if multipliers is not None:
            self.set_multipliers(multipliers)

    def _fold(self, mults) -> None:
        """lora_up block j = its multiplier-1 image times mults[j] (fp32; the bf16 shadow and the packed operands follow at the
        next LoRA-on pass)."""
        mults = tuple(mults)
        if mults == self._folded:
            return
        if self._base.device != self.slab.device:
            self._base = self._base.to(self.slab.device)
        with torch.no_grad():
            self.slab.detach().copy_(self._base)
            per_col = torch.tensor([mults[j] for j in self.col_file], dtype=torch.float32, device=self.slab.device)
            for lora in self.unet_loras:
                up = lora.lora_up.weight
                up.mul_(per_col.view(1, -1, *([1] * (up.ndim - 2))))
        self._folded = mults
        self.mark_updated()

    def set_multipliers(self, multipliers) -> None:
        """One fixed multiplier per file (default: all 1) for the ordinary, non-sweep passes."""
        mults = tuple(float(v) for v in multipliers)
        if len(mults) != len(self.file_ranks) or not all(math.isfinite(v) for v in mults):
            raise ValueError(f"set_multipliers: expected {len(self.file_ranks)} finite floats (one per file), got {mults}")
        self.multipliers = mults
        if self.strengths is None:
            self._fold(mults)

    def set_strengths(self, rows) -> None:
        """Per-sample strengths, one ROW of F floats per sample: row b of a UNet batch runs file j at ``rows[b % len(rows)][j]``
        (tiled over the CFG-doubled batch; the batch must be a whole multiple of ``len(rows)``), in ONE forward-only pass
        (bf16 only).  One file: plain floats are accepted too.  The fixed multipliers are not applied on top; ``None``
        restores them."""
        F = len(self.file_ranks)
        if rows is None:
            self.strengths = None
            self._strengths_version += 1
            self._fold(self.multipliers)
            return
        out = []
        for row in rows:
            if isinstance(row, (int, float)):
                if F != 1:
                    raise ValueError(f"set_strengths: a stack of {F} files takes one tuple of {F} strengths per sample, got the "
                                     f"plain number {row}")
                row = (row,)
            row = tuple(float(v) for v in row)
            if len(row) != F:
                raise ValueError(f"set_strengths: expected {F} strengths per sample (one per file), got {row}")
            out.append(row)
        if not out or not all(math.isfinite(v) for row in out for v in row):
            raise ValueError(f"set_strengths: expected a non-empty sequence of rows of finite floats, got {out}")
        self.strengths = tuple(out)
        self._strengths_version += 1
        self._fold((1.0,) * F)

    def save_weights(self, file, dtype=None, metadata: Optional[dict] = None):
        """The merged network: rank R, alpha = R (one file: that file's alpha), the current multipliers folded into
        `lora_up` -- a normal LoRA file that `LoRANetwork.from_file` loads."""
        held = self._folded
        self._fold(self.multipliers)
        try:
            super().save_weights(file, dtype, metadata)
        finally:
            self._fold(held)


class _ForeignModuleView:
    """One forward-patching LoRA module of another implementation, seen through the fields the engine needs."""

    def __init__(self, leaf_name: str, fm):
        self.fm = fm
        self.leaf_name = leaf_name
        self.lora_name = getattr(fm, "lora_name", LORA_PREFIX_UNET + "_" + leaf_name.replace(".", "_"))
        self.lora_down, self.lora_up = fm.lora_down, fm.lora_up
        self.lora_dim = int(fm.lora_down.weight.shape[0])
        self.scale = float(fm.scale)
        self.alpha = fm.alpha if hasattr(fm, "alpha") else torch.tensor(self.scale * self.lora_dim)
        self.down_off = self.up_off = -1

    @property
    def multiplier(self):
        return self.fm.multiplier

    @multiplier.setter
    def multiplier(self, v):
        self.fm.multiplier = v

    def parameters(self):
        return [self.lora_down.weight, self.lora_up.weight]


class ForeignLoRANetwork(LoRANetwork):
    """The reference's LoRA-injection seam (lora.py:97-106): its own ``lora.LoRANetwork`` works by
    re-assigning ``org_module.forward`` of every target leaf.  This UNet never calls leaf modules, so instead of
    ignoring (or refusing) such a network the engine ADOPTS it: the foreign ``lora_down`` / ``lora_up`` Parameters become
    views into a flat fp32 slab exactly like this package's own modules (`_adopt`), the low-rank products run fused in
    the GEMMs, gradients land in ``param.grad`` views of the gradient slab -- the foreign optimizer, ``with network:``
    switch (its ``multiplier`` fields are read at every forward), ``state_dict()`` and ``save_weights`` keep working on
    the objects the caller created.  The parameters can change behind the engine's back (a torch optimizer stepping the
    views), so the operand images are re-packed before every LoRA-on pass."""

    def __init__(self, unet, patched):      # patched: [(leaf qualified name, foreign LoRA module)]
        nn.Module.__init__(self)
        self.strict_reference = False
        self.unet_loras = [_ForeignModuleView(n, fm) for n, fm in patched]
        self.lora_dim = self.unet_loras[0].lora_dim
        self.alpha = float(self.unet_loras[0].scale * self.lora_dim)
        # the packed operand images carry ONE rank and ONE scale per GEMM site (fused q|k|v: three modules): modules that
        # share a site must agree -- which the reference's own network guarantees (one rank / alpha for all, lora.py:118-127)
        for l in self.unet_loras:
            if l.lora_dim != self.lora_dim or abs(l.scale - self.unet_loras[0].scale) > 1e-12:
                raise ValueError(f"adopted LoRA modules must share rank and alpha: {l.lora_name} has rank {l.lora_dim} / scale "
                                 f"{l.scale}, the first module rank {self.lora_dim} / scale {self.unet_loras[0].scale}")
        self.version = 0
        self._packed_version = -1
        self._unet = [unet]
        self._build_slab(unet.device)
        unet.engine().attach_lora(self)

    @property
    def multiplier(self):
        return self.unet_loras[0].multiplier

    @multiplier.setter
    def multiplier(self, v):
        for lora in self.unet_loras:
            lora.multiplier = v

    def needs_repack(self) -> bool:
        return True


def adopt_forward_patches(unet) -> Optional[ForeignLoRANetwork]:
    """Finds leaves whose ``forward`` was re-assigned to a bound method of an object carrying ``lora_down`` / ``lora_up`` /
    ``multiplier`` / ``scale`` (the reference's LoRAModule.apply_to, lora.py:97-100) and adopts them (None if there are
    none).  Leaves patched by anything else raise: the launch plans would silently ignore such a patch."""
    patched = []
    for name, m in unet.named_modules():
        if isinstance(m, (nn.Linear, nn.Conv2d)) and "forward" in m.__dict__:
            fm = getattr(m.__dict__["forward"], "__self__", None)
            if fm is None or not all(hasattr(fm, a) for a in ("lora_down", "lora_up", "multiplier", "scale")):
                raise RuntimeError(
                    f"{name}.forward has been re-assigned by something that is not a LoRA module (lora_down / lora_up / "
                    "multiplier / scale): this UNet executes static launch plans and never calls leaf modules.")
            patched.append((name, fm))
    if not patched:
        return None
    return ForeignLoRANetwork(unet, patched)
