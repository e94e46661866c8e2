"""LECO training loop on the MI355X hot path.

``train(config, prompts)`` has the reference's signature and observable behaviour
(train_lora.py:34-321): same config / prompt objects, same per-iteration sampling (prompt pair,
``timesteps_to`` in [1, max_denoising_steps), resolution bucket, CPU Gaussian latents), same
save cadence and file names.  The per-step arithmetic (train_lora.py:141-290) is executed by
:class:`FusedStep`:

  1. k LoRA-ON classifier-free-guided UNet passes + DDIM updates (train_util.py:172-193);
     each pass is ONE hipGraph launch (UNet forward + guidance combine + DDIM update + timestep
     advance, all reading their scalars from device memory);
  2. three LoRA-OFF passes (positive / neutral / unconditional) at t = timesteps1000[k*1000/n]
     (train_lora.py:195-237) -- the predictions stay on the device (the reference copies each
     to the host);
  3. one LoRA-ON pass for the target prompt whose activations are kept;
  4. ESD objective + its gradient in one kernel (prompt_util.py:107-135, fp32, on device);
  5. backward plan (dgrad through the UNet, wgrad of LoRA down/up only) into the flat fp32
     gradient slab;
  6. data parallel: ONE all-reduce (RCCL over xGMI) of that slab -- no other collective;
  7. fused AdamW (or Lion / Prodigy) on the flat fp32 master slab, refreshing the bf16 shadow the kernels read.

Optional, both on the device: ``max_grad_norm`` clips the gradient by its global norm between 6 and 7 (one reduction launch
that rewrites the optimizers' device-side grad_scale); ``accumulate`` = A sums the gradients of A steps in a second slab and
runs 6 and 7 once per group; ``scale_weight_norms`` pulls every LoRA module whose effective update has grown past that
Frobenius norm back onto it after 7 (max-norm regularisation, one launch on the slab: `leco_lora_max_norm`).

Nothing in a step synchronises with the host; ``loss`` is a device scalar.
"""
from __future__ import annotations

import ast
import itertools
import math
import os
import sys
from pathlib import Path
from typing import List, Optional

import torch

from . import config_util, model_util, ops, prompt_util, trace, train_util
from .config_util import RootConfig
from .lora import DEFAULT_TARGET_REPLACE, UNET_TARGET_REPLACE_MODULE_CONV, LoRANetwork
from .prompt_util import PromptEmbedsCache, PromptEmbedsPair, PromptSettings

DENOISE_GUIDANCE = 3.0  # hard-coded in the reference loop (train_lora.py:192)
DP_BASE_SEED = 1234     # data parallel: LoRA init seed (all ranks); rank r's data stream is seeded DP_BASE_SEED + 1 + r


def dist_info():
    """(rank, world, local_rank) from the torchrun environment; (0, 1, 0) when single-process."""
    return int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))


def init_distributed(backend: Optional[str] = None):
    import torch.distributed as dist
    rank, world, local = dist_info()
    if world > 1 and not dist.is_initialized():
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend == "nccl":   # bind this rank to its GPU before RCCL creates the communicator
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world, local


def shutdown_distributed(failed: bool = False):
    """Counterpart of `init_distributed` for the entry points that own the process (the train CLIs, bench.py): called by
    every rank after its last collective, it takes the process group down at the same point on all of them (barrier, then
    `destroy_process_group`) instead of leaving that to interpreter exit at different times -- rank 0 still writes files
    (or times launches) after the others are done, and an implicit teardown of a communicator whose peers have already
    gone is where the c10d back ends abort.  ``failed``: this rank is leaving through an exception -- its peers may be
    anywhere (inside a collective, or already in their own teardown barrier), so it does NOT enter the barrier (which
    would only move the hang); it destroys its group and lets the exception end the process, which is what makes torchrun
    take the other ranks down instead of leaving them in the barrier until the c10d timeout.  Never raises."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return
    try:
        if not failed:
            dist.barrier(**({"device_ids": [torch.cuda.current_device()]} if dist.get_backend() == "nccl" else {}))
        dist.destroy_process_group()
    except Exception as e:
        print(f"process-group teardown: {e!r}", file=sys.stderr)


class StrictReferenceOptimizer:
    """`--strict_reference`: the reference keeps its LoRA parameters AND the optimizer state in the training precision
    (`network.to(DEVICE, dtype=weight_dtype)`, train_lora.py:72-78; the optimizer is built on those parameters, :80-89),
    i.e. bf16 weights, bf16 exp_avg / exp_avg_sq, every elementwise op of the update rounded to bf16.  The fused AdamW
    keeps fp32 masters instead (a deliberate improvement: an lr = 1e-4 update of a 3e-2 weight is at bf16 resolution).
    This wrapper reproduces the reference's arithmetic exactly by running THE SAME torch optimizer class on parameters
    of that dtype: gradients are rounded into them, `step()` runs, the results are written back to the slab (whose
    values then are bf16-representable).  One small copy per LoRA matrix and step each way: a fidelity mode, not a fast
    path."""

    def __init__(self, network: LoRANetwork, optimizer_cls, dtype: torch.dtype, **kwargs):
        self.net, self.dtype = network, dtype
        self.views = [p for l in network.unet_loras for p in (l.lora_down.weight, l.lora_up.weight)]
        self.params = [torch.nn.Parameter(v.detach().to(dtype).clone()) for v in self.views]
        self.opt = optimizer_cls(self.params, **kwargs)
        self.param_groups = self.opt.param_groups

    def step(self):
        net = self.net
        with torch.no_grad():
            off = 0
            for p, v in zip(self.params, self.views):       # slab order = view order
                n = v.numel()
                p.grad = net.grad[off:off + n].view(v.shape).to(self.dtype)
                off += n
            self.opt.step()
            for p, v in zip(self.params, self.views):
                v.copy_(p.detach().float())

    def state_dict(self):
        return self.opt.state_dict()

    def load_state_dict(self, sd):
        self.opt.load_state_dict(sd)
        with torch.no_grad():
            for p, v in zip(self.params, self.views):
                p.copy_(v.detach().to(self.dtype))


class FusedStep:
    """One optimizer step of LECO training as launch plans on the UNet engine."""
    _tokens = itertools.count(1)

    def __init__(self, unet, network: LoRANetwork, scheduler, max_denoising_steps: int = 50, lr: float = 1e-4,
                 betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, world_size: int = 1,
                 process_group=None, optimizer="adamw", dedup: bool = False, prodigy: Optional[dict] = None,
                 max_grad_norm: Optional[float] = None, accumulate: int = 1, scale_weight_norms: Optional[float] = None):
        """``optimizer``: "adamw" / "adam" (fused leco_adamw; adam = no decoupled decay), "lion" (fused leco_lion),
        "prodigy" (fused leco_prodigy; ``prodigy``: its keywords, `PRODIGY_DEFAULTS` -- ``betas`` / ``eps`` default to
        this constructor's arguments, ``weight_decay`` to Prodigy's own 0 unless the dict carries it; ``lr`` is the
        multiplier of the estimated step size, normally 1.0), or a ``torch.optim.Optimizer`` built on ``network.prepare_optimizer_params()`` (its ``step()``
        runs on the fp32 slab views, then the bf16 shadow is refreshed).
        ``max_grad_norm``: clip the (all-reduced, averaged) gradient to this global L2 norm before the optimizer, on the
        device (`leco_grad_clip` rewrites the optimizers' grad_scale); 0 = measure only (`grad_stats`); None = off, no launch.
        ``accumulate`` = A > 1: `step` adds its gradient to ``network.grad_acc`` and only every A-th call all-reduces and
        applies the optimizer, on the mean of the group (`flush` applies a partial group).
        ``scale_weight_norms``: max-norm regularisation -- after every optimizer step each module whose effective update
        ``scale * lora_up @ lora_down`` has a Frobenius norm above this bound is scaled back onto it, on the device
        (`leco_lora_max_norm`, `LoRANetwork.apply_max_norm`'s rule; `weight_norm_stats`); 0 = measure only; None = off, no
        launch and no allocation."""
        if scale_weight_norms is not None and not float(scale_weight_norms) >= 0.0:
            raise ValueError(f"scale_weight_norms must be >= 0 (0: measure only) or None, got {scale_weight_norms!r}")
        if scale_weight_norms is not None and (network.strict_reference or isinstance(optimizer, StrictReferenceOptimizer)):
            raise ValueError("scale_weight_norms cannot be combined with --strict_reference: the reference has no such step, and "
                             "that mode's bf16 master weights would need a rounding rule of their own")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"max_grad_norm must be >= 0 (0: measure only) or None, got {max_grad_norm!r}")
        if int(accumulate) != accumulate or accumulate < 1:
            raise ValueError(f"accumulate must be an integer >= 1, got {accumulate!r}")
        self.unet, self.net, self.sched = unet, network, scheduler
        self.optimizer = optimizer
        self.n_steps = max_denoising_steps
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.world, self.pg = world_size, process_group
        self.opt_step = 0
        self.prodigy = None
        self._prodigy_buf = None           # (s, p0, leco_prodigy_state): allocated at the first use, this optimizer only
        self._prodigy_p0_taken = False     # p0 holds the parameters of the first Prodigy step (or a resumed run's)
        if isinstance(optimizer, str) and optimizer == "prodigy":
            unknown = set(prodigy or {}) - set(PRODIGY_KEYS)
            if unknown:
                raise ValueError(f"prodigy: unsupported keyword(s) {sorted(unknown)}; the fused kernel implements {PRODIGY_KEYS}")
            cfg = dict(PRODIGY_DEFAULTS, betas=tuple(betas), eps=eps)
            cfg.update(prodigy or {})
            cfg["betas"] = tuple(cfg["betas"])
            if cfg["beta3"] is None:
                cfg["beta3"] = math.sqrt(cfg["betas"][1])
            self.prodigy = cfg
        elif prodigy is not None:
            raise ValueError('`prodigy` keywords need optimizer="prodigy"')
        dev = unet.device
        self.dev = dev
        # device-side schedule tables
        scheduler.set_timesteps(max_denoising_steps)
        self.ts_f = scheduler.timesteps.to(torch.float32).to(dev)          # [n] 980, 960, ...
        # DDIM: (c_x, c_e) table for leco_cfg_ddim_step.  ddpm / lms / euler_a: SCHED_ROW-wide rows for
        # leco_cfg_sched_step (+ one extra row, rewritten every step, that re-scales the denoised latents for the
        # "current timestep" of the frozen / target passes, train_util.py:153 via train_lora.py:195-199)
        self.generic = not hasattr(scheduler, "coef_table")
        if self.generic:
            from .scheduler import SCHED_ROW
            rows = scheduler.rows()
            fin = torch.zeros(1, SCHED_ROW)
            fin[0, 0] = fin[0, 6] = 1.0
            self.coef = torch.cat([rows, fin]).to(dev).contiguous()
            self.fin_idx = torch.tensor([max_denoising_steps], dtype=torch.int32, device=dev)
            self.first_scale = float(scheduler.scale_model_input(torch.ones(1), scheduler.timesteps[0]))
        else:
            self.coef = scheduler.coef_table().to(dev).contiguous()        # [n][2]
        self.all_t = torch.arange(0, scheduler.num_train_timesteps, dtype=torch.float32, device=dev)
        self.single_slot = 512
        self.slot_idx = torch.tensor([self.single_slot], dtype=torch.int32, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        # activation dtype of the engine: bf16 (MFMA path) or fp32 (`train.precision: float32`, csrc/f32.hip)
        self.adt = unet.engine().adt
        self._ctx_cache = {}
        self._state = {}
        # ancestral schedulers (ddpm / euler_a): `noise_fn(i, numel)` supplies the noise of denoising pass i (a replayable
        # stream for parity tests); None = fresh device-RNG noise, like diffusers' randn_tensor on the UNet's device
        self.noise_fn = None
        self._pin = {}          # (numel, dtype) -> ring of pinned host staging buffers (`_h2d`)
        # De-duplicated step (SURVEY 7.1 step 5 / 8(d) `W_min`): the reference evaluates the three frozen predictions and the
        # target prediction through predict_noise at guidance_scale = 1 (train_lora.py:202-256), i.e. it runs the
        # unconditional half of every CFG pair only to multiply it by zero (train_util.py:151,163-166: u + 1 (c - u)), and it
        # evaluates identical prompts separately.  With `dedup` those four passes run on the conditional samples only and each
        # DISTINCT prompt of {positive, neutral, unconditional} once: U bs + bs UNet samples instead of 6 bs + 2 bs, and a
        # backward of batch bs instead of 2 bs.  The k denoising passes (guidance 3) are untouched.  `train()` turns it on
        # unless `--strict_reference` (or LECO_DEDUP=0); this class, bench.py's headline and the parity tests default to the
        # reference-faithful pass structure.  May be flipped between steps: both plan sets are built on demand.
        self.dedup = bool(dedup)
        self.target_from_forward_only = False      # test hook, see `step`
        self._token = next(FusedStep._tokens)      # names this object's private launch lists on plans the engine shares by shape
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._grad_stats = torch.zeros(4, dtype=torch.float32, device=dev) if max_grad_norm is not None else None
        self.scale_weight_norms = None if scale_weight_norms is None else float(scale_weight_norms)
        if self.scale_weight_norms is not None:
            network.norm_buffers()                 # the module table is uploaded here, not inside the first step
        self.accumulate = int(accumulate)
        self.pending = 0                           # micro-steps summed in network.grad_acc since the last optimizer step
        if self.accumulate > 1:
            self._grad_acc()

    # ---- host -> device copies that do not stall the host -------------------------------------------------------
    N_PIN = 4

    def _h2d(self, dst: torch.Tensor, src: torch.Tensor) -> None:
        """``dst.copy_(src)`` for a CPU ``src`` without blocking the host.  A copy from PAGEABLE host memory is synchronous:
        the call returns only after the stream has executed everything queued in front of it -- i.e. the whole previous
        optimizer step (round-5 measurement: the host sat in the initial-latents copy of step i + 1 until step i had
        finished on the GPU, so every host hiccup at a step boundary -- a loaded box, a slow wake-up -- was added to the
        step time).  Staged through a small ring of pinned buffers the copy is asynchronous and the host runs up to
        ``N_PIN`` steps ahead of the GPU."""
        if self.dev.type != "cuda" or src.device.type != "cpu":
            dst.copy_(src)
            return
        key = (src.numel(), src.dtype)
        ring = self._pin.get(key)
        if ring is None:
            ring = self._pin[key] = {"buf": [torch.empty(src.numel(), dtype=src.dtype, pin_memory=True) for _ in range(self.N_PIN)],
                                     "ev": [None] * self.N_PIN, "i": 0}
        i = ring["i"]
        ring["i"] = (i + 1) % self.N_PIN
        if ring["ev"][i] is not None:
            ring["ev"][i].synchronize()      # this slot's previous copy has left the host buffer (N_PIN steps ago)
        buf = ring["buf"][i]
        buf.copy_(src.reshape(-1))
        dst.copy_(buf.view(dst.shape) if dst.is_contiguous() else buf.reshape(dst.shape), non_blocking=True)
        ev = ring["ev"][i] = ring["ev"][i] or torch.cuda.Event()
        ev.record()

    @staticmethod
    def _set_ctx(plan, ctx: torch.Tensor) -> None:
        """plan.ctx <- ctx unless it already holds THIS tensor (the cached embeddings of a prompt pair never change: the
        same pair on consecutive steps costs no copy).  `Plan.set_ctx` is the buffer's only writer, so a plan that another
        caller filled in between (plans are shared by shape) carries that caller's token, not ours."""
        plan.set_ctx(ctx, src=ctx)

    def _scale_at(self, t_train: int) -> float:
        """scale_model_input factor at train timestep `t_train` of the 1000-step schedule (train_lora.py:195-199)."""
        n_keep = self.sched.num_inference_steps
        self.sched.set_timesteps(self.sched.num_train_timesteps)
        try:
            return float(self.sched.scale_model_input(torch.ones(1), torch.tensor(float(t_train))))
        finally:
            self.sched.set_timesteps(n_keep)

    # ---- per (batch, h, w) state: latents + per-pass prediction copies + the denoise plan -----------
    MAX_BUCKETS = int(os.environ.get("LECO_MAX_BUCKETS", "4"))   # resident (bs, h, w) plan sets (LRU)

    def _bucket(self, bs: int, h: int, w: int):
        key = (bs, h, w)
        st = self._state.get(key)
        if st is not None:
            self._state[key] = self._state.pop(key)      # most recently used last
        if st is None:
            while len(self._state) >= self.MAX_BUCKETS:   # dynamic_resolution: do not pin every bucket's buffers
                old = self._state.pop(next(iter(self._state)))
                eng = self.unet.engine()
                # exactly the evicted bucket's plans: another resident bucket at the same (h, w) may own a plan whose
                # batch collides (bs = 1 frozen pass and bs = 3 denoising pass are both UNet batch 6)
                for pk in old["owned"]:
                    eng.drop_plan(pk)
            eng = self.unet.engine()
            # the k partial-denoising passes never see a backward: they run on their own forward-only plan
            # (GEGLU fused into the ff projection's epilogue, no gradient buffers)
            # (share: predict_noise's cat([latents] * 2) -- both halves are the same sample until the prompt is used)
            dplan = eng.plan(2 * bs, h, w, need_bwd=False, share=2)
            st = dict(dplan=dplan, x=torch.zeros(bs, 4, h, w, dtype=torch.float32, device=self.dev), half_n=bs * 4 * h * w,
                      owned=[dplan.key], fplan_d={}, preds_d={}, dn=f"denoise@{self._token}", bs=bs, h=h, w=w)
            with ops.f32_mode(eng.f32):       # (context manager: an exception in here must not leave the module flag set)
                if self.generic:
                    st["noise"] = (torch.zeros(st["half_n"], dtype=torch.float32, device=self.dev)
                                   if self.sched.needs_noise else None)
                    st["hist"] = (torch.zeros(self.sched.n_hist * st["half_n"], dtype=torch.float32, device=self.dev)
                                  if self.sched.n_hist else None)
                    tail = [ops.cfg_sched_step(dplan.pred, st["x"], dplan.x_in, self.coef, dplan.t_idx, DENOISE_GUIDANCE,
                                               st["half_n"], st["noise"], st["hist"], self.sched.n_hist),
                            ops.advance(dplan.t_idx)]
                else:
                    tail = [ops.cfg_ddim_step(dplan.pred, st["x"], dplan.x_in, self.coef, dplan.t_idx, DENOISE_GUIDANCE,
                                              st["half_n"]),
                            ops.advance(dplan.t_idx)]
            # cross-attention K/V (+ their LoRA down projections) depend only on the prompt embeddings: the k
            # denoising passes of a step share one evaluation ("ctx_on"), the per-pass list skips those ops
            dplan.lists["ctx_on"] = [op for op in dplan.lists["fwd_on"] if op.tag == "ctx"]
            # The engine shares plans by shape: a second FusedStep on the same model (another scheduler, another
            # max_denoising_steps) gets the SAME dplan object.  The per-pass list ends in THIS object's DDIM update (its
            # latents, its coefficient table), so it is stored under this object's name; the timestep table is re-written
            # whenever the plan was last driven by someone else (`_own`).
            dplan.lists[st["dn"]] = [op for op in dplan.lists["fwd_on"] if op.tag != "ctx"] + tail
            dplan.lists["denoise"] = dplan.lists[st["dn"]]       # (tools/plan_profile.py, bench.py read this name)
            self._state[key] = st
            if not self.dedup:
                self._faithful(st)
        return st

    def _own(self, dplan) -> None:
        """The denoising plan's timestep table is the scheduler's.  Written when this object takes the plan over -- once,
        unless another FusedStep on the same engine drove it in between."""
        if getattr(dplan, "owner", None) != self._token:
            dplan.t_table[:self.n_steps].copy_(self.ts_f)
            dplan.owner = self._token

    def _faithful(self, st):
        """The reference's pass structure: LoRA-on target pass + backward at UNet batch 2 bs, the three LoRA-off predictions
        (positive / neutral / unconditional, each CFG-doubled) as ONE forward-only pass of batch 3 x 2 bs: same arithmetic
        per sample (GroupNorm / attention are per sample), three times the rows per GEMM, a third of the launches."""
        if "plan" not in st:
            bs, h, w = st["bs"], st["h"], st["w"]
            plan = self.unet.prepare((2 * bs, 4, h, w), lora_on=True)
            fplan = self.unet.engine().plan(6 * bs, h, w, need_bwd=False, share=6)
            st.update(plan=plan, fplan=fplan,
                      preds={n: fplan.pred[2 * bs * i:2 * bs * (i + 1)] for i, n in enumerate(("positive", "neutral", "unconditional"))})
            st["owned"] += [plan.key, fplan.key]
        return st["plan"], st["fplan"], st["preds"]

    def _deduped(self, st, U: int):
        """The de-duplicated passes (see __init__): training plan at UNet batch bs (conditional samples only), frozen plan
        at batch U bs -- U distinct prompts, the bs latents repeated U times (`share`)."""
        bs, h, w = st["bs"], st["h"], st["w"]
        if "plan_d" not in st:
            st["plan_d"] = self.unet.prepare((bs, 4, h, w), lora_on=True, tag="dedup")
            st["owned"].append(st["plan_d"].key)
        if U not in st["fplan_d"]:
            fp = self.unet.engine().plan(U * bs, h, w, need_bwd=False, share=U, tag="dedup")
            st["fplan_d"][U] = fp
            st["owned"].append(fp.key)
        return st["plan_d"], st["fplan_d"][U]

    @staticmethod
    def _text(e):      # SD1/2: a tensor; SDXL: PromptEmbedsXL(text_embeds, pooled_embeds)
        return e.text_embeds if hasattr(e, "text_embeds") else e

    def _ctx(self, pair: PromptEmbedsPair, which: str, bs: int) -> torch.Tensor:
        key = (id(pair), which, bs)
        hit = self._ctx_cache.get(key)
        if hit is None:
            c = train_util.concat_embeddings(self._text(pair.unconditional), self._text(getattr(pair, which)), bs)
            c = c.to(self.dev, self.adt).contiguous()
            # (the entry holds the pair itself: its id cannot be re-used by another pair while the cached tensor lives, and
            # `_set_ctx` may compare cached tensors by identity)
            hit = self._ctx_cache[key] = (pair, c)
        return hit[1]

    def _pooled(self, pair: PromptEmbedsPair, which: str, bs: int) -> torch.Tensor:
        """SDXL add_text_embeddings = concat(uncond.pooled, cond.pooled) (train_lora_xl.py:214-218)."""
        key = (id(pair), "pooled." + which, bs)
        hit = self._ctx_cache.get(key)
        if hit is None:
            c = train_util.concat_embeddings(pair.unconditional.pooled_embeds, getattr(pair, which).pooled_embeds, bs)
            hit = self._ctx_cache[key] = (pair, c.to(self.dev, self.adt).contiguous())
        return hit[1]

    def _ctx3(self, pair: PromptEmbedsPair, bs: int) -> torch.Tensor:
        key = (id(pair), "frozen3", bs)
        hit = self._ctx_cache.get(key)
        if hit is None:
            c = torch.cat([self._ctx(pair, w, bs) for w in ("positive", "neutral", "unconditional")]).contiguous()
            hit = self._ctx_cache[key] = (pair, c)
        return hit[1]

    def _same_prompt(self, a, b) -> bool:
        if a is b:
            return True
        ta, tb = self._text(a), self._text(b)
        if ta.shape != tb.shape or not torch.equal(ta, tb):
            return False
        pa, pb = getattr(a, "pooled_embeds", None), getattr(b, "pooled_embeds", None)
        return (pa is None and pb is None) or (pa is not None and pb is not None and torch.equal(pa, pb))

    def _dedup_info(self, pair: PromptEmbedsPair, bs: int) -> dict:
        """Distinct prompts among {positive, neutral, unconditional} (compared by VALUE: text and, for SDXL, pooled embeddings),
        their conditional-only contexts for the frozen plan ([P_0] * bs + [P_1] * bs + ...) and the target plan."""
        key = (id(pair), "dedup", bs)
        hit = self._ctx_cache.get(key)
        if hit is None:
            distinct, index = [], {}
            for n in ("positive", "neutral", "unconditional"):
                e = getattr(pair, n)
                for j, d in enumerate(distinct):
                    if self._same_prompt(e, d):
                        index[n] = j
                        break
                else:
                    index[n] = len(distinct)
                    distinct.append(e)

            def rep(t):
                return t.repeat_interleave(bs, dim=0)
            info = dict(U=len(distinct), index=index,
                        ctx=torch.cat([rep(self._text(d)) for d in distinct]).to(self.dev, self.adt).contiguous(),
                        ctx_t=rep(self._text(pair.target)).to(self.dev, self.adt).contiguous())
            if hasattr(pair.target, "pooled_embeds"):
                info["pooled"] = torch.cat([rep(d.pooled_embeds) for d in distinct]).to(self.dev, self.adt).contiguous()
                info["pooled_t"] = rep(pair.target.pooled_embeds).to(self.dev, self.adt).contiguous()
            hit = self._ctx_cache[key] = (pair, info)
        return hit[1]

    def _run(self, plan, which: str):
        self.unet._run(plan, which)

    @torch.no_grad()
    def step(self, pair: PromptEmbedsPair, timesteps_to: int, latents: torch.Tensor, lr: Optional[float] = None,
             add_time_ids: Optional[torch.Tensor] = None):
        """``latents``: (bs,4,h,w) initial noise (any device / dtype), as returned by
        ``train_util.get_initial_latents``.  SDXL: ``add_time_ids`` = ``train_util.get_add_time_ids(...)`` (1,6).
        Returns the loss as a 1-element device tensor."""
        net, unet = self.net, self.unet
        bs, _, h, w = latents.shape
        st = self._bucket(bs, h, w)
        dd = self._dedup_info(pair, bs) if self.dedup else None
        if dd is None:
            plan, fplan, preds = self._faithful(st)
            nrep, ctx_f, ctx_t = 3, self._ctx3(pair, bs), self._ctx(pair, "target", bs)
        else:
            plan, fplan = self._deduped(st, dd["U"])
            nrep, ctx_f, ctx_t = dd["U"], dd["ctx"], dd["ctx_t"]
            preds = {n_: fplan.pred[bs * j:bs * (j + 1)] for n_, j in dd["index"].items()}
        pb = 2 * bs if dd is None else bs          # UNet batch of the target pass / of one frozen prediction
        k = int(timesteps_to)
        n = self.n_steps
        # 1. partial denoising with LoRA on (train_lora.py:179-193)
        trace.push(f"denoise k={k}")
        net.multiplier = 1.0
        unet.prepare((pb, 4, h, w), lora_on=True, tag=None if dd is None else "dedup")   # re-packs LoRA operands if the slab changed
        x = st["x"]
        if latents.device.type == "cpu":
            self._h2d(x, latents.to(torch.float32))
        else:
            x.copy_(latents)
        dplan = st["dplan"]
        self._own(dplan)
        # first UNet input cat([scale_model_input(x)] * 2) + pass counter = 0: one launch (leco_step_begin)
        ops.step_begin(x, dplan.x_in, self.first_scale if self.generic else 1.0, st["half_n"], dplan.t_idx).run()
        if self.generic and st["hist"] is not None:
            st["hist"].zero_()
        self._set_ctx(dplan, self._ctx(pair, "target", bs))
        xl = self.unet.cfg.addition_embed_type == "text_time"
        if xl:
            ids = add_time_ids.reshape(1, 6).to(self.dev, torch.float32)
            dplan.time_ids.copy_(ids.repeat(2 * bs, 1).reshape(-1))
            dplan.text_embeds.copy_(self._pooled(pair, "target", bs))
            plan.time_ids.copy_(ids.repeat(pb, 1).reshape(-1))
            plan.text_embeds.copy_(self._pooled(pair, "target", bs) if dd is None else dd["pooled_t"])
        self._run(dplan, "ctx_on")
        for i in range(k):
            if self.generic and st["noise"] is not None:
                if self.noise_fn is not None:
                    st["noise"].copy_(self.noise_fn(i, st["half_n"]).to(self.dev, torch.float32).reshape(-1))
                else:
                    st["noise"].normal_()      # fresh ancestral noise (device RNG, like diffusers' randn_tensor)
            self._run(dplan, st["dn"])
        trace.pop()
        # 2. frozen predictions at the "current" timestep (train_lora.py:195-237)
        trace.push("frozen predictions")
        t_cur = int(self.sched.num_train_timesteps - 1 - int(k * self.sched.num_train_timesteps / n))
        if self.generic:
            # sigma-space schedulers: the UNet input of the remaining passes is x / sqrt(sigma(t_cur)^2 + 1)
            sc = self._scale_at(t_cur)
            self._h2d(self.coef[n, 6:7], torch.tensor([sc], dtype=torch.float32))
            sx2 = plan.x_in if dd is None else st.setdefault("x2_tmp", torch.empty_like(dplan.x_in))
            with ops.f32_mode(unet.engine().f32):
                ops.cfg_sched_step(None, x, sx2, self.coef, self.fin_idx, 0.0, st["half_n"]).run()
            src_x2, dst_a = sx2, (None if dd is None else plan.x_in)
        else:
            src_x2, dst_a = dplan.x_in, plan.x_in      # the last denoising pass left cat([denoised] * 2) as its next input
        # inputs + `current_timestep` of the four remaining passes (train_lora.py:195-256): one launch (leco_step_mid).
        # Faithful: the pair cat([x] * 2) -> target plan, 3 x -> frozen plan; de-duplicated: its first half (bs samples)
        # -> target plan, U x -> frozen plan.
        if dd is not None:
            src_x2 = src_x2[:bs]
        ops.step_mid(src_x2, dst_a, fplan.x_in, nrep, float(t_cur), plan, fplan, self.single_slot).run()
        net.multiplier = 0
        self._set_ctx(fplan, ctx_f)
        if xl:
            fplan.time_ids.copy_(ids.repeat(nrep * pb, 1).reshape(-1))
            fplan.text_embeds.copy_(torch.cat([self._pooled(pair, w_, bs) for w_ in ("positive", "neutral", "unconditional")])
                                    if dd is None else dd["pooled"])
        self._run(fplan, "fwd_off")
        trace.pop()
        # 3. target prediction with LoRA on; activations stay resident for the backward
        trace.push("target forward")
        net.multiplier = 1.0
        self._set_ctx(plan, ctx_t)
        self._run(plan, "fwd_on")
        if self.target_from_forward_only and dd is None:
            # parity experiment (tests/test_fullsize.py): the VALUE of the target prediction comes from the forward-only plan --
            # the arithmetic of the frozen predictions it is subtracted from (stripe kernels, fused GEGLU, shared prefix) --
            # while the backward still runs on the training plan's activations
            ops.step_mid(plan.x_in, dplan.x_in, None, 0, float(t_cur), dplan, None, self.single_slot).run()
            self._run(dplan, "fwd_on")
            plan.pred.copy_(dplan.pred)
        trace.pop()
        # 4. ESD objective + gradient w.r.t. the raw target prediction
        trace.push("loss + backward")
        if dd is None:
            ops.esd_loss(plan.pred, preds["positive"], preds["neutral"], preds["unconditional"], 1.0,
                         float(pair.guidance_scale), pair.sign, st["half_n"], self.loss, plan.dpred).run()
        else:
            ops.esd_loss_cond(plan.pred, preds["positive"], preds["neutral"], preds["unconditional"],
                              float(pair.guidance_scale), pair.sign, st["half_n"], self.loss, plan.dpred).run()
        st["last"] = dict(plan=plan, fplan=fplan, preds=preds, dedup=dd is not None)      # (tests / tools: what this step ran on)
        # 5. backward into the flat gradient slab
        net.grad.zero_()
        self._run(plan, "bwd")
        net.multiplier = 0  # the reference leaves the `with network:` block here
        trace.pop()
        if self.accumulate > 1:
            # 5b. gradient accumulation: this micro-step's gradient joins the group's sum; the all-reduce and the optimizer
            # run once per group.  (Not by letting the backward add into a non-zero slab: the atomic wgrad path adds, the
            # deterministic and fp32 reduce paths write.)
            ops.grad_accumulate(self._grad_acc(), net.grad, net.grad.numel(), self.pending == 0).run()
            self.pending += 1
            if self.pending == self.accumulate:
                self.flush(lr)
            return self.loss
        # 6. data parallel: one all-reduce of the LoRA gradient slab
        if self.world > 1:
            import torch.distributed as dist
            trace.push("all_reduce LoRA gradients")
            dist.all_reduce(net.grad, group=self.pg)
            trace.pop()
        # 7. optimizer on the fp32 master slab (+ bf16 shadow)
        trace.push("optimizer")
        self.apply_optimizer(lr)
        trace.pop()
        return self.loss

    def _grad_acc(self) -> torch.Tensor:
        """`network.grad_acc`: the fp32 sum of a group's micro-step gradients (exists only when accumulate > 1)."""
        net = self.net
        acc = getattr(net, "grad_acc", None)
        if acc is None or acc.shape != net.grad.shape or acc.device != net.grad.device:
            acc = net.grad_acc = torch.zeros_like(net.grad)
            self.pending = 0
        return acc

    def flush(self, lr: Optional[float] = None) -> None:
        """Apply the pending group of c <= accumulate micro-steps: one all-reduce of `network.grad_acc`, then the optimizer
        on its mean (grad_scale 1 / (world c)).  Nothing pending: nothing happens.  `step` calls it when a group is full;
        call it after the last step of a run whose length is no multiple of `accumulate`.  Collective when data parallel."""
        if self.pending == 0:
            return
        acc, count = self._grad_acc(), self.pending
        if self.world > 1:
            import torch.distributed as dist
            trace.push("all_reduce LoRA gradients")
            dist.all_reduce(acc, group=self.pg)
            trace.pop()
        trace.push("optimizer")
        self.pending = 0
        self.apply_optimizer(lr, grad=acc, count=count)
        trace.pop()

    def apply_optimizer(self, lr: Optional[float] = None, grad: Optional[torch.Tensor] = None, count: int = 1) -> None:
        """Step 7 of `step`: consume `network.grad` (already all-reduced) with the configured optimizer.  ``grad`` /
        ``count``: another slab of that size holding the sum of `count` micro-steps (`flush`)."""
        net = self.net
        self.opt_step += 1
        b1, b2 = self.betas
        lr = self.lr if lr is None else lr
        g = net.grad if grad is None else grad
        self._h2d(net.hyper, torch.tensor([lr, 1 - b1 ** self.opt_step, 1 - b2 ** self.opt_step, 1.0 / (self.world * count)],
                                          dtype=torch.float32))
        if self.max_grad_norm is not None:
            # hyper[3] <- coef / (world count), on the device: the optimizer kernels below read it as their grad_scale
            ops.grad_clip(g, net.hyper, self.max_grad_norm, self._grad_stats, net.slab.numel()).run()
        if isinstance(self.optimizer, str) and self.optimizer in ("adam", "adamw"):
            ops.adamw(net.slab.detach(), g, net.exp_avg, net.exp_avg_sq, net.shadow, net.hyper, b1, b2, self.eps,
                      self.wd, net.slab.numel()).run()
        elif self.optimizer == "lion":
            ops.lion(net.slab.detach(), g, net.exp_avg, net.shadow, net.hyper, b1, b2, self.wd,
                     net.slab.numel()).run()
        elif self.optimizer == "prodigy":
            c = self.prodigy
            s, p0, state = self._prodigy_buffers()
            if not self._prodigy_p0_taken:       # the first Prodigy step: x_0 of the distance estimate
                p0.copy_(net.slab.detach())
                self._prodigy_p0_taken = True
            ops.prodigy(net.slab.detach(), g, net.exp_avg, net.exp_avg_sq, s, p0, net.shadow, net.hyper, state,
                        c["betas"][0], c["betas"][1], c["beta3"], c["eps"], c["weight_decay"], c["d_coef"], c["growth_rate"],
                        c["decouple"], c["use_bias_correction"], c["safeguard_warmup"], net.slab.numel()).run()
        else:   # any torch optimizer over the slab views (prodigy, dadapt*, 8-bit ... when their packages exist)
            if g is not net.grad:             # the optimizer objects read `network.grad` (their .grad views / the strict copy)
                net.grad.copy_(g)
            if self.max_grad_norm is not None:
                net.grad.mul_(net.hyper[3])      # the device scalar coef / (world count): no host synchronisation
            elif self.world * count > 1:
                net.grad.mul_(1.0 / (self.world * count))
            if not isinstance(self.optimizer, StrictReferenceOptimizer):
                net.attach_grads()
            for group in self.optimizer.param_groups:
                group["lr"] = lr
            self.optimizer.step()
            net.sync_shadow()
        if self.scale_weight_norms is not None:
            # max-norm regularisation on the stepped slab and its shadow: one launch, the decisions stay on the device
            net._max_norm_op(self.scale_weight_norms).run()
        net.mark_updated()

    def weight_norm_stats(self) -> dict:
        """{keys_scaled, avg_norm, max_norm, nonfinite} of the last optimizer step (`leco_lora_max_norm`: the modules pulled
        back, the mean and the maximum of the module norms after that, the modules whose norm was not finite).  Copies them
        from the device, i.e. waits for the queued steps: for tests and logging."""
        if self.scale_weight_norms is None:
            raise RuntimeError("this FusedStep was built without scale_weight_norms (0 measures without scaling)")
        k, avg, top, bad = self.net.norm_buffers()[3].cpu().tolist()
        return dict(zip(ops.WEIGHT_NORM_STATS_FIELDS, (int(k), avg, top, int(bad))))

    def grad_stats(self) -> dict:
        """{norm, coef, nonfinite} of the last optimizer step's gradient (`leco_grad_clip`: the norm of the averaged,
        all-reduced gradient before clipping, the factor applied, the number of inf / NaN elements).  Copies them from the
        device, i.e. waits for the queued steps: for tests and logging."""
        if self._grad_stats is None:
            raise RuntimeError("this FusedStep was built without max_grad_norm (0 measures without clipping)")
        norm, coef, bad, _ = self._grad_stats.cpu().tolist()
        return dict(zip(ops.GRAD_STATS_FIELDS, (norm, coef, int(bad))))

    def _prodigy_buffers(self):
        """Prodigy's slab-sized `s` and `p0` and its device scalar state (ops.prodigy_state)."""
        if self.prodigy is None:
            raise RuntimeError('this FusedStep was not built with optimizer="prodigy"')
        slab = self.net.slab.detach()
        buf = self._prodigy_buf
        if buf is None or buf[0].shape != slab.shape or buf[0].device != slab.device:
            buf = self._prodigy_buf = (torch.zeros_like(slab), torch.empty_like(slab), ops.prodigy_state(self.prodigy["d0"], slab.device))
            self._prodigy_p0_taken = False
        return buf

    def prodigy_state(self) -> dict:
        """Prodigy's scalars {d, d0, d_max, d_numerator, d_denom, d_hat, dlr, k} (dlr = d * lr * bias correction of the
        last step).  Copies them from the device, i.e. waits for the queued steps: for tests and logging."""
        return dict(zip(ops.PRODIGY_STATE_FIELDS, self._prodigy_buffers()[2].cpu().tolist()))


# optimizer_args the fused Prodigy implements (prodigyopt.Prodigy's keywords; `lr` is train.lr)
PRODIGY_DEFAULTS = dict(betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True, use_bias_correction=False,
                        safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf"))
PRODIGY_KEYS = tuple(PRODIGY_DEFAULTS)

STATE_KEYS = ("slab", "exp_avg", "exp_avg_sq")


def _rank_rng_states(dev) -> dict:
    """This rank's generator states: the CPU stream (prompt pair, resolution bucket, crops, initial latents --
    train_lora.py:148-176) and, on a GPU, the device stream (ancestral noise of ddpm / euler_a)."""
    st = {"cpu": torch.get_rng_state()}
    if dev.type == "cuda":
        st["cuda"] = torch.cuda.get_rng_state(dev)
    return st


def save_training_state(path, fused: "FusedStep", iteration: int, lr_scheduler=None) -> None:
    """Everything a continuation needs (the reference cannot resume): fp32 master slab, optimizer moments and step
    count, the iteration, EVERY rank's RNG state and the LR-scheduler state.  Collective when data parallel (all
    ranks call it; rank 0 writes).  Tensors and primitives only, so the file loads with ``weights_only=True``."""
    net = fused.net
    rngs = [_rank_rng_states(fused.dev)]
    rank = 0
    if fused.world > 1:
        import torch.distributed as dist
        rank = dist.get_rank(fused.pg)
        rngs = [None] * fused.world
        dist.all_gather_object(rngs, _rank_rng_states(fused.dev), group=fused.pg)
    accs = None
    if fused.pending:                # (the same count on every rank: they run the same loop)
        accs = [fused._grad_acc().cpu().clone()]
        if fused.world > 1:
            mine, accs = accs[0], [None] * fused.world
            dist.all_gather_object(accs, mine, group=fused.pg)
    if rank != 0:
        return
    blob = {k: getattr(net, k).detach().cpu().clone() for k in STATE_KEYS}
    blob.update(format=2, world_size=int(fused.world), opt_step=fused.opt_step, iteration=int(iteration), rng=rngs,
                lr_scheduler=None if lr_scheduler is None else lr_scheduler.state_dict(),
                optimizer=None if isinstance(fused.optimizer, str) else fused.optimizer.state_dict())
    if fused.prodigy is not None:    # the fused Prodigy: its two extra slabs and the scalar state (other optimizers: format 2 as ever)
        s, p0, state = fused._prodigy_buffers()
        if not fused._prodigy_p0_taken:      # saved before the first step: x_0 is the slab as it stands
            p0 = net.slab.detach()
        blob.update(format=3, prodigy=dict(s=s.cpu().clone(), p0=p0.cpu().clone(), state=state.cpu().clone()))
    if accs is not None:             # saved inside an accumulation group: every rank's partial sum (files saved on a group boundary stay as they were)
        blob.update(format=4, grad_acc=torch.stack(accs), pending=int(fused.pending), accumulate=int(fused.accumulate))
    torch.save(blob, path)


def load_training_state(path, fused: "FusedStep", lr_scheduler=None) -> int:
    """Restores `save_training_state`; returns the next iteration index."""
    blob = torch.load(path, map_location="cpu", weights_only=True)
    net = fused.net
    # ---- validate everything BEFORE touching the live network / optimizer (a refused resume must leave them as they were)
    rngs = blob["rng"]
    if isinstance(rngs, torch.Tensor):          # format 1 (single process): the CPU generator state alone
        rngs = [{"cpu": rngs}]
    saved_world = int(blob.get("world_size", len(rngs)))
    if saved_world != fused.world or len(rngs) != fused.world:
        # a different rank count means a different global batch and a different replay of the shared k stream: the
        # continuation would silently be another run
        raise ValueError(f"{path}: training state was saved by {saved_world} rank(s) ({len(rngs)} RNG streams); this run "
                         f"has {fused.world}.  Resume with the same number of ranks.")
    for k in STATE_KEYS:
        if tuple(blob[k].shape) != tuple(getattr(net, k).shape):
            raise ValueError(f"{path}: {k} has shape {tuple(blob[k].shape)}, the network's is {tuple(getattr(net, k).shape)} "
                             "(different rank / network type / model)")
    has_obj_state = blob.get("optimizer") is not None
    if has_obj_state == isinstance(fused.optimizer, str):
        raise ValueError(f"{path}: saved with {'an optimizer object' if has_obj_state else 'the fused optimizer kernel'}, this "
                         f"run uses {'the fused optimizer kernel' if has_obj_state else 'an optimizer object'}: same config needed")
    pz = blob.get("prodigy")
    if (pz is not None) != (fused.prodigy is not None):
        raise ValueError(f"{path}: saved {'by the fused Prodigy optimizer' if pz is not None else 'without Prodigy state'}, this run "
                         f"uses optimizer={fused.optimizer if isinstance(fused.optimizer, str) else type(fused.optimizer).__name__!r}"
                         ": same config needed")
    if pz is not None:
        for k in ("s", "p0"):
            if tuple(pz[k].shape) != tuple(net.slab.shape) or pz[k].dtype != torch.float32:
                raise ValueError(f"{path}: prodigy.{k} has shape {tuple(pz[k].shape)}, the network's slab {tuple(net.slab.shape)}")
        if pz["state"].dtype != torch.float64 or pz["state"].numel() != len(ops.PRODIGY_STATE_FIELDS):
            raise ValueError(f"{path}: prodigy.state is not the {len(ops.PRODIGY_STATE_FIELDS)} doubles of leco_prodigy_state")
    pending = int(blob.get("pending", 0))
    if pending:
        saved_acc = int(blob["accumulate"])
        if saved_acc != fused.accumulate:
            raise ValueError(f"{path}: saved inside an accumulation group ({pending} of {saved_acc} micro-steps pending); this run "
                             f"accumulates {fused.accumulate}.  Resume with gradient_accumulation_steps: {saved_acc}.")
        ga = blob["grad_acc"]
        if tuple(ga.shape) != (fused.world, *net.grad.shape) or ga.dtype != torch.float32 or not 0 < pending < saved_acc:
            raise ValueError(f"{path}: grad_acc has shape {tuple(ga.shape)} with {pending} pending micro-steps, expected "
                             f"{(fused.world, *net.grad.shape)} and fewer than {saved_acc}")
    rank = 0
    if fused.world > 1:
        import torch.distributed as dist
        rank = dist.get_rank(fused.pg)
    with torch.no_grad():
        for k in STATE_KEYS:
            getattr(net, k).detach().copy_(blob[k].to(getattr(net, k).device))
        if pending:
            fused._grad_acc().copy_(blob["grad_acc"][rank].to(net.grad.device))
        fused.pending = pending
        if pz is not None:
            for dst, k in zip(fused._prodigy_buffers(), ("s", "p0", "state")):
                dst.copy_(pz[k].to(dst.device))
            fused._prodigy_p0_taken = True
    fused.opt_step = int(blob["opt_step"])
    if has_obj_state:
        fused.optimizer.load_state_dict(blob["optimizer"])
    if lr_scheduler is not None and blob.get("lr_scheduler") is not None:
        lr_scheduler.load_state_dict(blob["lr_scheduler"])
        # recursive schedules (cosine) continue from the optimizer's current lr, which the scheduler state lacks
        for group, lr in zip(lr_scheduler.optimizer.param_groups, lr_scheduler.get_last_lr()):
            group["lr"] = lr
    torch.set_rng_state(rngs[rank]["cpu"])
    if fused.dev.type == "cuda" and "cuda" in rngs[rank]:
        torch.cuda.set_rng_state(rngs[rank]["cuda"], fused.dev)
    net.sync_shadow()
    net.mark_updated()
    return int(blob["iteration"]) + 1


def flush():
    import gc
    if torch.cuda.is_available():
        torch.cuda.empty_cache()
    gc.collect()


def _parse_optimizer_args(s: str) -> dict:
    kwargs = {}
    if s is not None and len(s) > 0:
        for arg in s.split(" "):
            key, value = arg.split("=")
            kwargs[key] = ast.literal_eval(value)
    return kwargs


def train(config: RootConfig, prompts: List[PromptSettings], device: Optional[torch.device] = None,
          use_graphs: bool = True, progress: bool = True, xl: bool = False, resume_from: Optional[str] = None,
          save_state: bool = False, stop_after: Optional[int] = None, strict_reference: bool = False,
          dedup: Optional[bool] = None, native_text_encoder: bool = False):
    """Reference entry point ``train(config, prompts)`` (train_lora.py:34; ``xl=True``: train_lora_xl.py:40).
    Extra keyword arguments only select the device and execution mode, and the resume extension:
    ``save_state`` writes ``{save.name}_state.pt`` next to every saved LoRA, ``resume_from`` continues from one
    (same config), ``stop_after`` ends the run after that iteration index (used to test resumption);
    ``strict_reference`` keeps the LoRA parameters and the optimizer state in ``train.precision`` like the reference
    (`StrictReferenceOptimizer`) instead of fp32 masters.  ``dedup`` (default: on unless ``strict_reference`` or
    LECO_DEDUP=0): the de-duplicated pass structure of `FusedStep` -- the guidance-1 passes run on the conditional samples
    only and identical prompts once; same objective, ~10 % fewer FLOPs per step at the reference's prompt settings.
    ``native_text_encoder``: the prompts are encoded by `leco_amd.clip` instead of the ``transformers`` models (bf16 only)."""
    if dedup is None:
        dedup = not strict_reference and os.environ.get("LECO_DEDUP", "1") not in ("", "0")
    if strict_reference and config.train.scale_weight_norms is not None:
        raise ValueError("train.scale_weight_norms cannot be combined with --strict_reference: the reference has no such step, "
                         "and that mode's bf16 master weights would need a rounding rule of their own")
    rank, world, local = init_distributed()
    if device is None:
        device = torch.device(f"cuda:{local}" if torch.cuda.is_available() else "cpu")
    if device.type == "cuda":
        torch.cuda.set_device(device)
    metadata = {"prompts": ",".join([p.model_dump_json() for p in prompts]), "config": config.model_dump_json()}
    save_path = Path(config.save.path)
    modules = list(DEFAULT_TARGET_REPLACE)
    if config.network.type == "c3lier":
        modules += UNET_TARGET_REPLACE_MODULE_CONV
    if config.logging.verbose:
        print(metadata)
    wandb = None
    if config.logging.use_wandb and rank == 0:
        import wandb  # optional dependency, only when requested
        wandb.init(project=f"LECO_{config.save.name}", config=metadata)
    weight_dtype = config_util.parse_precision(config.train.precision)
    save_weight_dtype = config_util.parse_precision(config.train.precision)  # sic, train_lora.py:55
    # train.precision (config_util.py:75-83, train_lora.py:54-67): float32 runs the fp32 compute mode (fp32 activations,
    # weights and LoRA operands, exact fp32 MFMA contractions: csrc/f32.hip -- the reference's arithmetic for such
    # configs, several times slower than the bf16 MFMA path); bfloat16 is the MFMA path; float16 (11 significand bits) has
    # no MFMA instantiation here and must not silently run on the narrower bf16 (8 bits): it is computed in the fp32 mode
    # (>= the requested precision everywhere), the saved LoRA is fp16 as requested.
    compute_dtype = torch.bfloat16 if weight_dtype == torch.bfloat16 else torch.float32
    if weight_dtype == torch.float16:
        print("note: train.precision=float16 is computed in the fp32 mode (there are no fp16 kernels; bf16 would be narrower "
              "than requested); only the saved LoRA is fp16.  Use bfloat16 for the fast MFMA path.")
    if native_text_encoder and compute_dtype != torch.bfloat16:
        raise NotImplementedError(f"--native_text_encoder: the native CLIP text encoder is bf16-only, train.precision "
                                  f"{config.train.precision!r} runs in the fp32 mode; drop the flag or use bfloat16")

    if xl:
        tokenizers, text_encoders, unet, noise_scheduler = model_util.load_models_xl(
            config.pretrained_model.name_or_path, scheduler_name=config.train.noise_scheduler,
            native_text_encoder=native_text_encoder)
        for text_encoder in text_encoders:
            text_encoder.to(device, dtype=compute_dtype)
            text_encoder.eval()
        tokenizer = None
    else:
        tokenizer, text_encoder, unet, noise_scheduler = model_util.load_models(
            config.pretrained_model.name_or_path, scheduler_name=config.train.noise_scheduler,
            v2=config.pretrained_model.v2, v_pred=config.pretrained_model.v_pred, native_text_encoder=native_text_encoder)
        text_encoder.to(device, dtype=compute_dtype)
        text_encoder.eval()
    unet.to(device, dtype=compute_dtype)
    unet.enable_xformers_memory_efficient_attention()
    unet.requires_grad_(False)
    unet.eval()
    unet.use_graphs = use_graphs and device.type == "cuda"

    if world > 1:   # identical LoRA init on every rank ...
        torch.manual_seed(DP_BASE_SEED)
    network = LoRANetwork(unet, rank=config.network.rank, multiplier=1.0, alpha=config.network.alpha,
                          train_method=config.network.training_method, target_replace_modules=modules,
                          strict_reference=strict_reference,
                          strict_dtype=weight_dtype).to(device, dtype=weight_dtype)   # float32: the round trip is a no-op, like network.to(dtype=weight_dtype)

    if world > 1:
        # ... and from here on every rank draws its OWN prompt pair / resolution / crops / latents (the reference's
        # sampling sites train_lora.py:148-156,175-177 all use the global CPU stream); only k comes from the shared
        # generator below
        torch.manual_seed(DP_BASE_SEED + 1 + rank)

    opt_name = config.train.optimizer.lower()
    optimizer_kwargs = _parse_optimizer_args(config.train.optimizer_args)
    if opt_name in ("adam", "adamw", "lion"):
        # fused on the flat slab.  torch.optim.Adam's weight_decay is a coupled L2 term, which the fused kernel
        # does not implement: fall through to the torch object in that (non-default) case -- and whenever
        # optimizer_args carries a keyword the fused kernels do not implement (amsgrad, maximize, ...): the reference
        # forwards every keyword to the optimizer constructor (train_lora.py:80-89), nothing may be dropped silently
        unsupported = set(optimizer_kwargs) - {"betas", "eps", "weight_decay"}
        coupled_l2 = opt_name == "adam" and optimizer_kwargs.get("weight_decay", 0.0)
        fused_opt = opt_name if not (coupled_l2 or unsupported) else None
    elif opt_name == "prodigy" and not strict_reference:
        # fused on the flat slab (leco_prodigy) when every keyword is one the kernel implements; anything else (slice_p, ...)
        # goes to the package like before -- nothing is dropped silently
        fused_opt = opt_name if set(optimizer_kwargs) <= set(PRODIGY_KEYS) else None
    else:
        fused_opt = None
    if strict_reference and weight_dtype != torch.float32:
        # the reference's own optimizer class on parameters of the training precision (train_lora.py:78-89)
        fused_opt = StrictReferenceOptimizer(network, train_util.get_optimizer(opt_name), weight_dtype, lr=config.train.lr,
                                             **optimizer_kwargs)
    if fused_opt is None:
        optimizer_module = train_util.get_optimizer(opt_name)     # ImportError names the missing package
        fused_opt = optimizer_module(network.prepare_optimizer_params(), lr=config.train.lr, **optimizer_kwargs)
    wd_default = 1e-2 if opt_name == "adamw" else 0.0
    default_betas = (0.9, 0.99) if opt_name == "lion" else (0.9, 0.999)
    fused = FusedStep(unet, network, noise_scheduler, config.train.max_denoising_steps, lr=config.train.lr,
                      betas=tuple(optimizer_kwargs.get("betas", default_betas)), eps=optimizer_kwargs.get("eps", 1e-8),
                      weight_decay=optimizer_kwargs.get("weight_decay", wd_default), world_size=world,
                      optimizer=fused_opt, dedup=dedup, max_grad_norm=config.train.max_grad_norm,
                      accumulate=config.train.gradient_accumulation_steps,
                      scale_weight_norms=config.train.scale_weight_norms,
                      prodigy={k: v for k, v in optimizer_kwargs.items() if k not in ("betas", "eps")}
                      if fused_opt == "prodigy" else None)
    # LR schedule: drive torch's own scheduler objects on a dummy parameter so the values are exact
    _dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=config.train.lr)
    lr_scheduler = train_util.get_lr_scheduler(config.train.lr_scheduler, _dummy, max_iterations=config.train.iterations,
                                               lr_min=config.train.lr / 100)
    criteria = torch.nn.MSELoss()

    print("Prompts")
    cache = PromptEmbedsCache()
    prompt_pairs: List[PromptEmbedsPair] = []
    with torch.no_grad():
        for settings in prompts:
            print(settings)
            for prompt in [settings.target, settings.positive, settings.neutral, settings.unconditional]:
                if cache[prompt] is None:
                    if xl:   # (text_embeds, pooled) -- the reference passes the tuple un-unpacked and crashes
                        cache[prompt] = prompt_util.PromptEmbedsXL(
                            *train_util.encode_prompts_xl(tokenizers, text_encoders, [prompt], num_images_per_prompt=1))
                    else:
                        cache[prompt] = train_util.encode_prompts(tokenizer, text_encoder, [prompt])
            prompt_pairs.append(PromptEmbedsPair(criteria, cache[settings.target], cache[settings.positive],
                                                 cache[settings.unconditional], cache[settings.neutral], settings))
    tokenizer = text_encoder = tokenizers = text_encoders = None
    flush()

    it = range(config.train.iterations)
    pbar = None
    if progress and rank == 0:
        from tqdm import tqdm
        pbar = it = tqdm(it)
    # DP: every rank draws its own prompt pair / noise, but the SAME k (shared-seed generator) so that
    # all ranks run the same number of denoising passes.
    k_gen = torch.Generator().manual_seed(20230701) if world > 1 else None
    # ... and the SAME shape class: a step's (batch_size, height, width) decides which launch plans run, so ranks in
    # different classes would wait for the slowest at the all-reduce ("prefer same-shape prompts per
    # step").  The shared generator draws a pair index (uniform over the pairs, like train_lora.py:148-150) and -- for
    # dynamic_resolution prompts -- the bucket; every rank then draws ITS pair among the pairs of that index's class
    # (batch_size, resolution, dynamic_resolution) from its own stream.  The marginal distribution over pairs stays uniform.
    shape_gen = torch.Generator().manual_seed(20230702) if world > 1 else None
    shape_class = lambda p: (p.batch_size, p.resolution, bool(p.dynamic_resolution))
    class_members = {}
    for idx, p in enumerate(prompt_pairs):
        class_members.setdefault(shape_class(p), []).append(idx)

    def draw_shared(step_k_only: bool = False):
        """One step's shared draws, in a fixed order (the resume path replays them)."""
        k = torch.randint(1, config.train.max_denoising_steps, (1,), generator=k_gen).item()
        if shape_gen is None:
            return k, None, None
        lead = prompt_pairs[torch.randint(0, len(prompt_pairs), (1,), generator=shape_gen).item()]
        hw = None
        if lead.dynamic_resolution:
            hw = train_util.get_random_resolution_in_bucket(lead.resolution, generator=shape_gen)
        return k, shape_class(lead), hw
    loss = None
    lr_now = config.train.lr
    start = 0
    if resume_from is not None:
        start = load_training_state(resume_from, fused, lr_scheduler)
        if k_gen is not None:   # replay the shared streams up to the resume point
            for _ in range(start):
                draw_shared()
    for i in it:
        if i < start:
            continue
        if shape_gen is None:
            # single process: the reference's order on the ONE global CPU stream -- prompt pair, then timesteps_to, then
            # (below) the resolution bucket and the latents (train_lora.py:148-156,162-177), so a seeded run reproduces the
            # reference's (pair, k, resolution, latents) sequence
            pair = prompt_pairs[torch.randint(0, len(prompt_pairs), (1,)).item()]
            timesteps_to, cls, shared_hw = draw_shared()
        else:
            timesteps_to, cls, shared_hw = draw_shared()
            members = class_members[cls]
            pair = prompt_pairs[members[torch.randint(0, len(members), (1,)).item()]]
        height, width = pair.resolution, pair.resolution
        if pair.dynamic_resolution:
            height, width = shared_hw if shared_hw is not None else train_util.get_random_resolution_in_bucket(pair.resolution)
        if config.logging.verbose:
            print("gudance_scale:", pair.guidance_scale, "resolution:", pair.resolution, "dynamic_resolution:",
                  pair.dynamic_resolution, (height, width), "batch_size:", pair.batch_size)
        latents = train_util.get_initial_latents(noise_scheduler, pair.batch_size, height, width, 1)
        add_time_ids = train_util.get_add_time_ids(height, width, dynamic_crops=pair.dynamic_crops) if xl else None
        lr_now = lr_scheduler.get_last_lr()[0]
        loss = fused.step(pair, timesteps_to, latents, lr=lr_now, add_time_ids=add_time_ids)
        show = pbar is not None and (i % 10 == 0 or config.logging.verbose)
        # (the loss already waits for the step where it is shown: Prodigy's estimated step size d * lr comes along, fetched once)
        dlr = fused.prodigy_state()["dlr"] if fused.prodigy and (show or wandb is not None) else None
        # ... and, when clipping is configured, the norm of the last applied gradient.  Non-finite gradients are DETECTED here,
        # i.e. as coarsely as the loss is shown (every 10th iteration unless verbose, every iteration with wandb): the step
        # itself never meets the host, and no step is skipped.
        gstat = fused.grad_stats() if fused.max_grad_norm is not None and fused.opt_step and (show or wandb is not None) else None
        if gstat is not None and gstat["nonfinite"] > 0:
            raise FloatingPointError(f"iteration {i}: {gstat['nonfinite']} non-finite element(s) in the LoRA gradient of the last "
                                     f"optimizer step (norm {gstat['norm']}); the weights are no longer usable")
        # ... and, with scale_weight_norms, the module norms the last optimizer step left
        wstat = (fused.weight_norm_stats() if fused.scale_weight_norms is not None and fused.opt_step and (show or wandb is not None)
                 else None)
        if show:
            pbar.set_description(f"Loss*1k: {loss.item() * 1000:.4f}" + ("" if dlr is None else f" d*lr: {dlr:.3e}")
                                 + ("" if gstat is None else f" |g|: {gstat['norm']:.2e}" + ("*" if gstat["coef"] < 1 else ""))
                                 + ("" if wstat is None else f" |w|: {wstat['avg_norm']:.2e}/{wstat['max_norm']:.2e}"
                                    + (f"*{wstat['keys_scaled']}" if wstat["keys_scaled"] else "")))
        if wandb is not None:
            wandb.log({"loss": loss.item(), "iteration": i, "lr": lr_scheduler.get_last_lr()[0],
                       **({} if dlr is None else {"d*lr": dlr}),
                       **({} if gstat is None else {"grad_norm": gstat["norm"], "clip_coef": gstat["coef"]}),
                       **({} if wstat is None else {"avg_key_norm": wstat["avg_norm"], "max_key_norm": wstat["max_norm"],
                                                    "keys_scaled": wstat["keys_scaled"]})})
        _dummy.step()
        lr_scheduler.step()
        if i % config.save.per_steps == 0 and i != 0 and i != config.train.iterations - 1:
            if rank == 0:
                print("Saving...")
                save_path.mkdir(parents=True, exist_ok=True)
                network.save_weights(save_path / f"{config.save.name}_{i}steps.safetensors", dtype=save_weight_dtype,
                                     metadata=metadata)
            if save_state:      # collective: gathers every rank's RNG streams, rank 0 writes
                save_training_state(save_path / f"{config.save.name}_state.pt", fused, i, lr_scheduler)
        if stop_after is not None and i >= stop_after:
            if save_state:
                if rank == 0:
                    save_path.mkdir(parents=True, exist_ok=True)
                save_training_state(save_path / f"{config.save.name}_state.pt", fused, i, lr_scheduler)
            break
    fused.flush(lr_now)      # a trailing partial accumulation group (nothing pending: no-op)
    if rank == 0:
        print("Saving...")
        save_path.mkdir(parents=True, exist_ok=True)
        # the reference builds `metadata` (train_lora.py:38-41) and then drops it; it is written here
        network.save_weights(save_path / f"{config.save.name}_last.safetensors", dtype=save_weight_dtype,
                             metadata=metadata)
    flush()
    print("Done.")
    return network, (loss.item() if loss is not None else None)


def main(args, xl: bool = False):
    config = config_util.load_config_from_yaml(args.config_file)
    prompts = prompt_util.load_prompts_from_yaml(config.prompts_file)
    failed = True
    try:
        train(config, prompts, xl=xl, resume_from=getattr(args, "resume", None),
              save_state=bool(getattr(args, "save_state", False)),
              strict_reference=bool(getattr(args, "strict_reference", False)),
              native_text_encoder=bool(getattr(args, "native_text_encoder", False)))
        failed = False
    finally:      # every rank, also the one that is on its way out with an exception
        shutdown_distributed(failed=failed)
