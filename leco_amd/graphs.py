"""hipGraph capture and replay of launch lists (``csrc/runtime.hip``), for the UNet, VAE and CLIP plans and the measurement
tools: the one place that names the graph entry points of the C ABI.

A captured graph is an opaque handle stored wherever its owner says (``store[key]``): ``plan.graphs[which]`` on a UNet plan,
``vars(plan)["graph"]`` -- the ``plan.graph`` attribute -- on a VAE or CLIP plan.  Every model object captures on a side stream
of its own (``model._capture_stream``, created on first use); nothing here owns a stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Iterable, MutableMapping, Optional, Sequence

import torch
from torch import nn

from . import hip, ops

SIGNATURES = {
    "leco_graph_begin_capture": [C.c_void_p],
    "leco_graph_end_capture": [C.c_void_p, C.POINTER(C.c_void_p)],
    "leco_graph_launch": [C.c_void_p, C.c_void_p],
    "leco_graph_destroy": [C.c_void_p],
}
# ctypes argument types belong to ONE loaded-library object and `hip._use_library` makes a new one: `ops._fn` declares per
# bound library and forgets the old one's functions.  An undeclared entry point would take a stream handle as a C int.
ops._SIGS.update(SIGNATURES)


def api() -> C.CDLL:
    """The library that is bound now, with the four graph entry points declared on that object."""
    for name in SIGNATURES:
        ops._fn(name)
    return hip.lib()


def enabled(model) -> bool:
    """Replay ``model``'s lists from graphs?  Only on a GPU; the emulator and LECO_TRACE_OPS launch eagerly."""
    return bool(model.use_graphs and model.device.type == "cuda" and not hip.is_emulated()) and not ops._TRACE_OPS


def _capture(oplist: Sequence[ops.Op], side: torch.cuda.Stream, cur: torch.cuda.Stream) -> C.c_void_p:
    side.wait_stream(cur)
    sp = side.cuda_stream
    hip.check(ops._fn("leco_graph_begin_capture")(sp), "graph begin")
    try:
        ops.run_plan(oplist, sp)
    finally:
        gh = C.c_void_p()
        hip.check(ops._fn("leco_graph_end_capture")(sp, C.byref(gh)), "graph end")
    return gh


def launch(owner, store: MutableMapping, key, oplist: Sequence[ops.Op], *, warm: bool) -> None:
    """Replay ``oplist`` on the current stream from the graph ``store[key]``, capturing it first if there is none yet.

    ``warm``: run the list eagerly once before the capture, so that one-time kernel attributes are set outside it.  Only for
    a list that may run twice: the VAE's and CLIP's are pure functions of their input buffers, the UNet's ``denoise`` list
    advances the device step counter and overwrites the latents, so the UNet passes ``warm=False``."""
    cur = torch.cuda.current_stream()
    g = store.get(key)
    if g is None:
        if warm:
            ops.run_plan(oplist)
        side = owner.__dict__.get("_capture_stream")
        if side is None:
            side = owner.__dict__["_capture_stream"] = torch.cuda.Stream()
        g = store[key] = _capture(oplist, side, cur)
    hip.check(ops._fn("leco_graph_launch")(g, cur.cuda_stream), "graph launch")


def destroy(device: torch.device, handles: Iterable[Optional[C.c_void_p]]) -> None:
    """Wait for the device, then destroy the graphs (None: never captured).  The caller drops its references."""
    if device.type == "cuda" and not hip.is_emulated():
        torch.cuda.synchronize(device)
        fn = ops._fn("leco_graph_destroy")
        for g in handles:
            if g is not None:
                fn(g)


def replay_us(oplist: Sequence[ops.Op], reps: int = 20, warm: int = 3) -> float:
    """Measurement tools: microseconds per replay of ``oplist`` captured into one graph (HIP events around ``reps`` replays
    on the current stream, after ``warm`` untimed ones)."""
    cur = torch.cuda.current_stream()
    g = _capture(oplist, torch.cuda.Stream(), cur)
    fn, sp = ops._fn("leco_graph_launch"), cur.cuda_stream
    try:
        for _ in range(warm):
            hip.check(fn(g, sp), "graph launch")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        rc = 0
        e0.record()
        for _ in range(reps):
            rc = fn(g, sp) or rc
        e1.record()
        e1.synchronize()
        hip.check(rc, "graph launch")
    finally:
        destroy(cur.device, [g])
    return e0.elapsed_time(e1) / reps * 1e3


# ---- the forward-only models (VAE; the CLIP text encoder and image tower, one encoder stack: encoder.py) ------------------------
class PlanEngine:
    """Packed device operands of one model and its launch plans by shape; a plan keeps its graph in ``plan.graph``."""

    def __init__(self, device: torch.device):
        self.device = device
        self.plans: dict = {}

    def cached(self, key, build: Callable):
        """``plans[key]``, made by ``build()`` on first use."""
        p = self.plans.get(key)
        if p is None:
            p = self.plans[key] = build()
        return p

    def release(self) -> None:
        destroy(self.device, [p.graph for p in self.plans.values()])
        self.plans.clear()


class ForwardOnlyModel(nn.Module):
    """A module tree that only holds weights and runs launch plans from an engine (``engine_type(model, device)``) built on
    first use.  The packed operands follow the parameters: anything that may change them -- ``.to()`` / ``.half()`` / ...
    (``_apply``), ``load_state_dict`` -- drops the engine with its plans and graphs, and the next call rebuilds it.  Compute is
    bf16 with fp32 accumulation whatever dtype the parameters are held in; outputs come back in that dtype.  A subclass keeps its
    configuration in ``self.cfg``."""
    engine_type: type = None
    label: str = None                        # "CLIP text encoder": what this model's error messages start with
    bf16_only: str = "bfloat16 only"         # `set_precision`'s refusal, in the parentheses

    def __init__(self, use_graphs: bool):
        super().__init__()
        self.use_graphs = use_graphs
        self._engine: Optional[PlanEngine] = None

    @property
    def config(self):
        return self.cfg

    def set_precision(self, precision):
        if precision not in ("bfloat16", "bf16", torch.bfloat16):
            raise NotImplementedError(f"{self.label}: compute precision {precision!r} is not implemented ({self.bf16_only})")
        return self

    def load_strict(self, state_dict, strict: bool = True, **kw):
        """A ``load_state_dict`` for the subclass that wants one: a missing or unexpected key is a KeyError naming it
        (``position_ids``, a buffer of older checkpoints, is ignored)."""
        sd = {k: v for k, v in state_dict.items() if not k.endswith("position_ids")}
        missing, unexpected = ForwardOnlyModel.load_state_dict(self, sd, strict=False, **kw)
        for what, keys in (("the state dict lacks", missing), ("unexpected key", unexpected)):
            if strict and keys:
                raise KeyError(f"{self.label}: {what} {keys[0]!r}" + (f" (and {len(keys) - 1} more)" if len(keys) > 1 else ""))
        return missing, unexpected

    def copy_out(self, t: torch.Tensor, *shape) -> torch.Tensor:
        """A plan buffer as an output of this model's dtype; a copy, the next call reuses the plan's buffers."""
        return t.view(*shape).to(self.dtype, copy=True)

    def engine(self):
        if self._engine is None or self._engine.device != self.device:
            self.release()
            self._engine = self.engine_type(self, self.device)
        return self._engine

    def release(self) -> None:
        if self.__dict__.get("_engine") is not None:      # (a no-op on a model that is still being constructed)
            self._engine.release()
            self._engine = None

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self.release()
        return out

    def load_state_dict(self, *a, **kw):
        out = super().load_state_dict(*a, **kw)
        self.release()
        return out

    def _run(self, plan) -> None:
        if enabled(self):
            launch(self, vars(plan), "graph", plan.ops, warm=True)
        else:
            ops.run_plan(plan.ops)
