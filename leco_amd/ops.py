"""Typed Python front for every entry point of ``libleco_hip.so``.

Each function returns an :class:`Op` -- the C function plus its marshalled argument tuple --
so that callers can either run it immediately (``op.run()``) or append it to a static launch
plan that is later replayed eagerly or captured into a hipGraph (``leco_amd.unet``).  Tensors
are only used for their device pointers; nothing here computes in PyTorch.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import torch

from . import hip
from .hip import ACT_NONE, ACT_SILU, A_PLAIN, GemmArgs, LoraSite, ptr  # noqa: F401

_vp, _i32, _i64, _f32, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double

_SIGS = {
    "leco_groupnorm_fwd": [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _i64, _vp],
    "leco_groupnorm_bwd": [_vp, _i64, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _i64, _vp],
    "leco_groupnorm_apply_stats": [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _i64, _vp],
    "leco_colstats": [_vp, _i64, _vp, _i32, _i32, _i32, _i32, _vp],
    "leco_layernorm_fwd": [_vp, _i64, _vp, _vp, _f32, _i32, _i32, _vp, _i64, _vp, _vp, _vp],
    "leco_layernorm_bwd": [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp],
    "leco_attention_fwd": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp],
    "leco_attention_bwd": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64,
                           _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64,
                           _i32, _i32, _i32, _i32, _i32, _f32, _vp],
    "leco_attention_causal_fwd": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _f32, _vp],
    "leco_embed_rows": [_vp, _i64, _i32, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i32, _vp],
    "leco_clip_preprocess": [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _i64, _vp],
    "leco_vit_embed": [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp],
    "leco_cosine_scores": [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _f32, _vp],
    "leco_xattn_token_maps": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp],
    "leco_attn_maps_merge": [_vp, _i32, _vp, _i32, _i32, _i32, _vp],
    "leco_heat_overlay": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp],
    "leco_image_compare": [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp],
    "leco_gemm_ex": [C.POINTER(GemmArgs), _i32, _i32, _vp, _i64, _vp],
    "leco_geglu_fwd": [_vp, _i64, _vp, _i64, _i32, _i32, _vp],
    "leco_geglu_bwd": [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp],
    "leco_add": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp],
    "leco_upsample2x_bwd": [_vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "leco_conv_in": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "leco_conv_out": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "leco_conv_out_bwd": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "leco_latent_affine": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp],
    "leco_conv_out_rgb": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "leco_conv_in_rgb": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "leco_conv_out_moments": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _i32, _i32, _i32, _i32, _vp],
    "leco_timestep_embedding": [_vp, _vp, _i32, _i32, _i32, _vp, _vp],
    "leco_advance": [_vp, _vp],
    "leco_cfg_ddim_step": [_vp, _vp, _vp, _vp, _vp, _f32, _i64, _vp],
    "leco_cfg_sched_step": [_vp, _vp, _vp, _vp, _vp, _f32, _i64, _vp, _vp, _i32, _vp],
    "leco_esd_loss": [_vp, _vp, _vp, _vp, _f32, _f32, _f32, _i64, _vp, _vp, _vp],
    "leco_esd_loss_cond": [_vp, _vp, _vp, _vp, _f32, _f32, _i64, _vp, _vp, _vp],
    "leco_adamw": [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _i64, _vp],
    "leco_lion": [_vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _i64, _vp],
    "leco_prodigy": [_vp] * 9 + [_f64] * 7 + [_i32, _i64, _vp],
    "leco_grad_clip": [_vp, _i64, _vp, _f32, _vp, _vp],
    "leco_grad_accumulate": [_vp, _vp, _i64, _i32, _vp],
    "leco_lora_max_norm": [_vp, _vp, _i64, _vp, _i32, _f32, _vp, _vp, _vp, _vp],
    "leco_cast_f32_bf16": [_vp, _vp, _i64, _vp],
    "leco_memset": [_vp, _i32, _i64, _vp],
    "leco_repeat": [_vp, _vp, _i64, _i32, _vp],
    "leco_step_begin": [_vp, _vp, _i32, _f32, _i64, _vp, _vp],
    "leco_step_mid": [_vp, _vp, _vp, _i64, _i32, _f32, _vp, _vp, _vp, _vp, _i32, _vp],
    "leco_lora_pack": [_vp, _i32, _vp],
    "leco_lora_rowscale": [_vp, _i64, _i32, _i32, _i32, _vp, _vp],
    "leco_lora_rowscale_stack": [_vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp],
    "leco_lora_wgrad_conv": [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _f32, _i32, _i32, _i32, _i32, _i32,
                             _i32, _i32, _vp, _i64, _vp],
    "leco_rowgroup_sum": [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp],
    "leco_lora_wgrad_grouped": [_vp, _i32, _i32, _i32, _vp],
    "leco_lora_wgrad": [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _f32, _vp, _i64, _vp],
    "leco_xattn_prep": [_vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "leco_xblock_tail": [_vp, _vp],
    "leco_xgemm": [_vp, _vp],
    "leco_xblock_head": [_vp, _vp],
}
# fp32 compute mode (csrc/f32.hip): the same argument lists behind `leco_f32_` entry points; activations / weights /
# LoRA operand images are float.  While `f32_mode(True)` is active (the plan builder of an fp32 engine), every Op that
# has an fp32 twin is created on it.
_F32_TWINS = ("leco_groupnorm_fwd", "leco_groupnorm_bwd", "leco_layernorm_fwd", "leco_layernorm_bwd", "leco_attention_fwd",
              "leco_attention_bwd", "leco_geglu_fwd", "leco_geglu_bwd", "leco_add", "leco_upsample2x_bwd", "leco_conv_in",
              "leco_conv_out", "leco_conv_out_bwd", "leco_timestep_embedding", "leco_cfg_ddim_step", "leco_cfg_sched_step",
              "leco_cast_f32_bf16", "leco_lora_pack", "leco_lora_wgrad_conv", "leco_rowgroup_sum", "leco_lora_wgrad")
for _n in _F32_TWINS:
    _SIGS["leco_f32_" + _n[len("leco_"):]] = _SIGS[_n]
_SIGS["leco_f32_gemm"] = [C.POINTER(GemmArgs), _vp]
_f32_active = False


class f32_mode:
    """Context manager: Ops created inside are bound to the fp32 kernels."""

    def __init__(self, on: bool = True):
        self.on = bool(on)

    def __enter__(self):
        global _f32_active
        self.prev, _f32_active = _f32_active, self.on
        return self

    def __exit__(self, *exc):
        global _f32_active
        _f32_active = self.prev


_fn_cache = {}
_fn_lib = None


def _fn(name: str):
    global _fn_lib
    lib = hip.lib()
    if _fn_lib is not lib:
        _fn_cache.clear()
        _fn_lib = lib
    f = _fn_cache.get(name)
    if f is None:
        f = getattr(lib, name)
        if name in _SIGS:
            f.argtypes = _SIGS[name]
        f.restype = C.c_int
        _fn_cache[name] = f
    return f


class Op:
    """One enqueue-only C-ABI call: ``fn(*args, stream)``."""
    __slots__ = ("name", "fn", "args", "keep", "tag")

    def __init__(self, name: str, args: tuple, keep=None):
        self.tag = None   # plan builders label ops (e.g. "ctx": depends only on the prompt embeddings)
        if _f32_active:
            if name in _F32_TWINS:
                name = "leco_f32_" + name[len("leco_"):]
            elif name == "leco_lora_wgrad_grouped":
                raise RuntimeError("fp32 mode accumulates the LoRA weight gradients per problem (leco_f32_lora_wgrad)")
        self.name = name
        self.fn = _fn(name)
        self.args = args
        self.keep = keep  # python objects whose memory the args point to

    def run(self, stream=None) -> None:
        if stream is None:
            stream = default_stream()
        rc = self.fn(*self.args, stream)
        if rc != 0:
            hip.check(rc, self.name)


def default_stream():
    """torch's current HIP stream handle (None when bound to the host emulator)."""
    if hip.is_emulated() or not torch.cuda.is_available():
        return None
    return torch.cuda.current_stream().cuda_stream


_TRACE_OPS = os.environ.get("LECO_TRACE_OPS", "0") not in ("", "0")


def _describe_op(op) -> str:
    try:
        if op.name.endswith("gemm_ex"):
            g = op.keep[0]
            return f"m={g.m} n={g.n} k={g.k} a_mode={g.a_mode} ext={g.ext_k} tile={op.args[1]} split={op.args[2]} stats={bool(g.col_stats)}"
        return " ".join(str(a) for a in op.args if isinstance(a, int) and 0 <= a < (1 << 24))
    except Exception:
        return ""


def run_plan(plan: Sequence[Op], stream=None) -> None:
    if stream is None:
        stream = default_stream()
    if _TRACE_OPS:       # LECO_TRACE_OPS=1: name every launch on stderr before it goes out and wait for it (a GPU memory
        import sys        # fault kills the process without a Python error: the last name printed is the faulting launch)
        for op in plan:
            print(f"[leco op] {op.name} {_describe_op(op)}", file=sys.stderr, flush=True)
            rc = op.fn(*op.args, stream)
            if rc != 0:
                hip.check(rc, op.name)
            if torch.cuda.is_available() and not hip.is_emulated():
                torch.cuda.synchronize()
        return
    for op in plan:
        rc = op.fn(*op.args, stream)
        if rc != 0:
            hip.check(rc, op.name)


# ---------------------------------------------------------------------------------------------
def gemm(args: GemmArgs, keep=None, ws: Optional[torch.Tensor] = None, tile: int = 0, split_k: int = 0) -> Op:
    """``ws``: fp32 scratch for split-K partial slabs (without it the GEMM never splits).  ``tile == 0 and
    split_k == 0``: the launch shape comes from the tuner (leco_amd/tune.py: table / measurement), else the C heuristic."""
    if _f32_active:      # one exact-fp32 MFMA kernel, no launch shapes to choose
        return Op("leco_f32_gemm", (C.byref(args),), keep=(args, keep))
    if tile == 0 and split_k == 0:
        from . import tune
        tile, split_k = tune.choose(args, ws)
        if ws is None and split_k == 0:
            split_k = 1
    if ws is None:
        return Op("leco_gemm_ex", (C.byref(args), tile, max(1, split_k), None, 0), keep=(args, keep))
    return Op("leco_gemm_ex", (C.byref(args), tile, split_k, ws.data_ptr(), ws.numel() * ws.element_size()),
              keep=(args, keep, ws))


def groupnorm_fwd(x0, ld0, x1, ld1, c0, gamma, beta, batch, hw, c, groups, eps, act, stats, y, ldy) -> Op:
    return Op("leco_groupnorm_fwd", (ptr(x0), ld0, ptr(x1), ld1, c0, ptr(gamma), ptr(beta), batch, hw, c,
                                     groups, eps, act, ptr(stats), ptr(y), ldy))


def groupnorm_bwd(x0, ld0, x1, ld1, c0, dy, lddy, gamma, beta, stats, batch, hw, c, groups, eps, act,
                  bstats, dx, lddx) -> Op:
    return Op("leco_groupnorm_bwd", (ptr(x0), ld0, ptr(x1), ld1, c0, ptr(dy), lddy, ptr(gamma), ptr(beta),
                                     ptr(stats), batch, hw, c, groups, eps, act, ptr(bstats), ptr(dx), lddx))


def layernorm_fwd(x, ldx, gamma, beta, eps, m, c, y, ldy, mean, rstd) -> Op:
    return Op("leco_layernorm_fwd", (ptr(x), ldx, ptr(gamma), ptr(beta), eps, m, c, ptr(y), ldy, ptr(mean),
                                     ptr(rstd)))


def layernorm_bwd(x, ldx, dy, lddy, gamma, mean, rstd, dres, ldres, m, c, dx, lddx) -> Op:
    return Op("leco_layernorm_bwd", (ptr(x), ldx, ptr(dy), lddy, ptr(gamma), ptr(mean), ptr(rstd), ptr(dres),
                                     ldres, m, c, ptr(dx), lddx))


def attention_fwd(q, ldq, bsq, k, ldk, bsk, v, ldv, bsv, o, ldo, bso, lse, batch, heads, sq, skv, d, scale) -> Op:
    return Op("leco_attention_fwd", (q, ldq, bsq, k, ldk, bsk, v, ldv, bsv, o, ldo, bso, ptr(lse), batch, heads,
                                     sq, skv, d, scale))


def attention_bwd(q, ldq, bsq, k, ldk, bsk, v, ldv, bsv, o, ldo, bso, do, lddo, bsdo, lse, delta,
                  dq, lddq, bsdq, dk, lddk, bsdk, dv, lddv, bsdv, batch, heads, sq, skv, d, scale) -> Op:
    return Op("leco_attention_bwd", (q, ldq, bsq, k, ldk, bsk, v, ldv, bsv, o, ldo, bso, do, lddo, bsdo,
                                     ptr(lse), ptr(delta), dq, lddq, bsdq, dk, lddk, bsdk, dv, lddv,
                                     bsdv, batch, heads, sq, skv, d, scale))


CAUSAL_ATTN_MAX_S = 128      # LECO_CAUSAL_ATTN_MAX_S


def attention_causal_fwd(q, ldq, bsq, k, ldk, bsk, v, ldv, bsv, o, ldo, bso, batch, heads, s, d, scale, keep=None) -> Op:
    """softmax(q k^T scale + causal) v per (batch, head); q, k, v, o are raw device addresses (column views of a fused
    q|k|v buffer can be passed), head dim 64, s <= CAUSAL_ATTN_MAX_S."""
    return Op("leco_attention_causal_fwd", (q, ldq, bsq, k, ldk, bsk, v, ldv, bsv, o, ldo, bso, batch, heads, s, d, scale),
              keep=keep)


def check_row_ids(ids: torch.Tensor, rows: int, what: str = "ids") -> torch.Tensor:
    """The HOST-side index check of `embed_rows`: ``ids`` (any integer tensor) as contiguous int32 on the host, or
    IndexError when an entry lies outside [0, rows) -- before anything is launched."""
    t = torch.as_tensor(ids)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError(f"{what}: expected an integer tensor, got {t.dtype}")
    t = t.detach().to("cpu", torch.int64).reshape(-1)
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= rows):
        bad = int(t[(t < 0) | (t >= rows)][0])
        raise IndexError(f"{what}: index {bad} is out of range for a table of {rows} rows")
    return t.to(torch.int32).contiguous()


def embed_rows(table, ldt, rows, idx, pos, ldp, period, out, ldo, n, c, keep=None) -> Op:
    """out[i] = table[idx[i]] (+ pos[i % period]) on bf16 rows; ``idx``: DEVICE int32 [n] whose values went through
    `check_row_ids` on the host."""
    return Op("leco_embed_rows", (ptr(table), ldt, rows, ptr(idx), ptr(pos), ldp, period, ptr(out), ldo, n, c),
              keep=(table, idx, pos, out, keep))


def embed_rows_checked(table: torch.Tensor, ids: torch.Tensor, pos: Optional[torch.Tensor], period: int,
                       out: torch.Tensor) -> Op:
    """`embed_rows` on whole tensors: validates ``ids`` on the host (IndexError) and moves them to the table's device."""
    rows, c = table.shape
    idx = check_row_ids(ids, rows).to(table.device)
    return embed_rows(table, table.stride(0), rows, idx, pos, 0 if pos is None else pos.stride(0), period, out, out.stride(0),
                      idx.numel(), c)


def clip_preprocess(img, batch, h, w, row_tab, row_w, row_taps, col_tab, col_w, col_taps, mean_std, image_size, patch_size,
                    out, ldo, keep=None) -> Op:
    """uint8 NHWC ``img`` [batch][h][w][3] -> bf16 patch rows ``out`` [batch * P][ldo]: antialiased bicubic resize of the
    shortest edge to ``image_size``, centre crop, 1/255, mean / std, patch flattening, zero padding up to a multiple of 64
    columns.  The tap tables (`clip_vision.resize_taps`) and ``mean_std`` (fp32 [6]) are DEVICE tensors, see
    include/leco_hip.h."""
    return Op("leco_clip_preprocess", (ptr(img), batch, h, w, ptr(row_tab), ptr(row_w), row_taps, ptr(col_tab), ptr(col_w), col_taps,
                                       ptr(mean_std), image_size, patch_size, ptr(out), ldo),
              keep=(img, row_tab, row_w, col_tab, col_w, mean_std, out, keep))


def vit_embed(patches, ldp, cls, pos, ldpos, out, ldo, batch, tokens, c, keep=None) -> Op:
    """out[b][0] = cls + pos[0], out[b][1 + t] = patches[b][t] + pos[1 + t] on bf16 rows (fp32 sum, one rounding)."""
    return Op("leco_vit_embed", (ptr(patches), ldp, ptr(cls), ptr(pos), ldpos, ptr(out), ldo, batch, tokens, c),
              keep=(patches, cls, pos, out, keep))


def cosine_scores(x, ldx, y, ldy, out, ldo, nb, nt, d, scale: float = 1.0, keep=None) -> Op:
    """out[b][t] = scale * cos(x[b], y[t]): bf16 ``x`` [nb][d], ``y`` [nt][d] -> fp32 ``out`` [nb][nt]."""
    return Op("leco_cosine_scores", (ptr(x), ldx, ptr(y), ldy, ptr(out), ldo, nb, nt, d, float(scale)), keep=(x, y, out, keep))


TOKEN_MAPS_MAX, TOKEN_MAPS_MAX_KEYS = 8, 128
TOKEN_MAPS_HEAD_DIMS = (32, 40, 64, 80, 160)


def xattn_token_maps(q, ldq, bsq, k, ldk, bsk, tok_w, n_maps, step_w, maps, batch, heads, sq, skv, d, scale, keep=None) -> Op:
    """maps[b][m][i] += step_w / heads * sum_h sum_j tok_w[m][j] softmax_j(scale <q_bhi, k_bhj>): ``q`` / ``k`` are raw device
    addresses of bf16 operands as `attention_fwd` takes them, ``tok_w`` fp32 [n_maps][skv], ``step_w`` fp32 [1] and ``maps``
    fp32 [batch][n_maps][sq] are DEVICE tensors (include/leco_hip.h).  bf16 compute mode only."""
    if _f32_active:
        raise NotImplementedError("xattn_token_maps (attention heatmaps) is implemented for the bf16 compute mode only")
    return Op("leco_xattn_token_maps", (ptr(q), ldq, bsq, ptr(k), ldk, bsk, ptr(tok_w), n_maps, ptr(step_w), ptr(maps), batch, heads,
                                        sq, skv, d, float(scale)), keep=(tok_w, step_w, maps, keep))


def attn_map_layers(layers: Sequence[tuple], device) -> torch.Tensor:
    """The DEVICE table of `attn_maps_merge` (`leco_attn_map_layer`: pointer, h, w, weight) from (map tensor or address, h, w,
    weight) tuples, as raw bytes."""
    import struct
    raw = b"".join(struct.pack("<Qiif4x", ptr(m), int(h), int(w), float(wgt)) for m, h, w, wgt in layers)      # 24 bytes: 8-aligned
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def attn_maps_merge(table: torch.Tensor, n_layers: int, heat: torch.Tensor, planes: int, ht: int, wt: int, keep=None) -> Op:
    """heat[p] = sum_l weight_l * bilinear(map_l[p] -> ht x wt) (torch's align_corners=False rule); ``table``: `attn_map_layers`."""
    return Op("leco_attn_maps_merge", (ptr(table), n_layers, ptr(heat), planes, ht, wt), keep=(table, heat, keep))


def heat_overlay(heat, rmax, pic, lut, out, batch, n_maps, map_index, ht, wt, alpha) -> Op:
    """out = the uint8 pictures ``pic`` [batch][ht][wt][3] with heat map ``map_index`` of ``heat`` [batch][n_maps][ht][wt] blended
    over them through the colour table ``lut`` (uint8 [256][3]); ``rmax``: fp32 [batch * n_maps] reciprocal full-heat values."""
    return Op("leco_heat_overlay", (ptr(heat), ptr(rmax), ptr(pic), ptr(lut), ptr(out), batch, n_maps, map_index, ht, wt, float(alpha)),
              keep=(heat, rmax, pic, lut, out))


def image_compare_workspace(batch: int, h: int, w: int) -> int:
    """Bytes of scratch `image_compare` needs (0 for shapes it refuses)."""
    fn = getattr(hip.lib(), "leco_image_compare_workspace")
    fn.argtypes, fn.restype = [_i32, _i32, _i32], _i64
    return int(fn(batch, h, w))


def image_compare(a, ref, ref_stride, batch, h, w, taps, change_map, stats, workspace=None, workspace_bytes=None, keep=None) -> Op:
    """Mean SSIM, exact SSE and (``change_map`` not None) the map 1 - ssim of the uint8 NHWC pictures ``a`` [batch][h][w][3]
    against ``ref`` (``ref_stride`` bytes between its pictures: 0 = one baseline for all, h * w * 3 = pairwise); ``taps`` fp32
    [11], ``stats`` float64 [batch][2] = (mean SSIM, SSE), ``change_map`` fp32 [batch][h][w]: DEVICE tensors or raw addresses
    (include/leco_hip.h).  ``workspace``: a DEVICE buffer of `image_compare_workspace` bytes (its size is taken from the
    tensor unless ``workspace_bytes`` says otherwise); None: one is allocated on ``stats``' device and kept by the Op."""
    if workspace is None:
        workspace = torch.empty(max(image_compare_workspace(batch, h, w), 8) // 8, dtype=torch.float64, device=stats.device)
    if workspace_bytes is None:
        workspace_bytes = workspace.numel() * workspace.element_size()
    return Op("leco_image_compare", (ptr(a), ptr(ref), int(ref_stride), batch, h, w, ptr(taps), ptr(change_map), ptr(stats),
                                     ptr(workspace), int(workspace_bytes)), keep=(a, ref, taps, change_map, stats, workspace, keep))


def geglu_fwd(u, ldu, y, ldy, m, f) -> Op:
    return Op("leco_geglu_fwd", (ptr(u), ldu, ptr(y), ldy, m, f))


def geglu_bwd(u, ldu, dy, lddy, du, lddu, m, f) -> Op:
    return Op("leco_geglu_bwd", (ptr(u), ldu, ptr(dy), lddy, ptr(du), lddu, m, f))


def add(a, lda, b, ldb, c, ldc, out, ldo, m, cols) -> Op:
    """a, b, c, out are raw device addresses (ints) so that column-offset views can be passed."""
    return Op("leco_add", (a, lda, b, ldb, c, ldc, out, ldo, m, cols))


def upsample2x_bwd(dy, dx, batch, h, w, c) -> Op:
    return Op("leco_upsample2x_bwd", (ptr(dy), ptr(dx), batch, h, w, c))


def conv_in(x, w, bias, y, batch, h, wd, cin, cout) -> Op:
    return Op("leco_conv_in", (ptr(x), ptr(w), ptr(bias), ptr(y), batch, h, wd, cin, cout))


def conv_out(x, w, bias, y, batch, h, wd, c, cout) -> Op:
    return Op("leco_conv_out", (ptr(x), ptr(w), ptr(bias), ptr(y), batch, h, wd, c, cout))


def latent_affine(x, w, bias, y, batch, hw, cin, cout, in_scale) -> Op:
    """y (bf16 NCHW) = 1x1 conv of in_scale * x (fp32 NCHW): the VAE's post_quant_conv on latents / scaling_factor."""
    return Op("leco_latent_affine", (ptr(x), ptr(w), ptr(bias), ptr(y), batch, hw, cin, cout, float(in_scale)), keep=(x, w, bias, y))


def conv_out_rgb(x, w, bias, y, img, batch, h, wd, c) -> Op:
    """3x3 conv to RGB: ``y`` fp32 NCHW and / or ``img`` uint8 NHWC (either may be None), see include/leco_hip.h."""
    return Op("leco_conv_out_rgb", (ptr(x), ptr(w), ptr(bias), ptr(y), ptr(img), batch, h, wd, c), keep=(x, w, bias, y, img))


def conv_in_rgb(x, img, w, bias, y, batch, h, wd, cout) -> Op:
    """The VAE encoder's conv_in: ``x`` fp32 NCHW in [-1, 1] or ``img`` uint8 NHWC (exactly one, the other None) -> channels-last
    bf16 ``y``; ``w`` fp32 [cout][3][3][3], see include/leco_hip.h."""
    return Op("leco_conv_in_rgb", (ptr(x), ptr(img), ptr(w), ptr(bias), ptr(y), batch, h, wd, cout), keep=(x, img, w, bias, y))


def conv_out_moments(x, w, bias, qw, qb, noise, moments, latents, scale, batch, h, wd, c) -> Op:
    """The VAE encoder's exit: 3x3 conv to 8 channels + quant_conv (fp32 8x8) -> ``moments`` fp32 (B,8,h,w) and / or
    ``latents`` fp32 (B,4,h,w) = scale * (mean + std * noise) (``noise`` None: the mode), see include/leco_hip.h."""
    return Op("leco_conv_out_moments", (ptr(x), ptr(w), ptr(bias), ptr(qw), ptr(qb), ptr(noise), ptr(moments), ptr(latents),
                                        float(scale), batch, h, wd, c), keep=(x, w, bias, qw, qb, noise, moments, latents))


def conv_out_bwd(dy, w, dx, batch, h, wd, c, cout) -> Op:
    return Op("leco_conv_out_bwd", (ptr(dy), ptr(w), ptr(dx), batch, h, wd, c, cout))


def timestep_embedding(t_table, idx, t_stride, n, dim, out) -> Op:
    return Op("leco_timestep_embedding", (ptr(t_table), ptr(idx), t_stride, n, dim, ptr(out)))


def advance(counter) -> Op:
    return Op("leco_advance", (ptr(counter),))


def cfg_sched_step(pred, x, x2, coef, step, guidance, half_n, noise=None, hist=None, n_hist=0) -> Op:
    return Op("leco_cfg_sched_step", (ptr(pred), ptr(x), ptr(x2), ptr(coef), ptr(step), guidance, half_n, ptr(noise),
                                      ptr(hist), n_hist))


def cfg_ddim_step(pred, x, x2, coef, step, guidance, half_n) -> Op:
    return Op("leco_cfg_ddim_step", (ptr(pred), ptr(x), ptr(x2), ptr(coef), ptr(step), guidance, half_n))


def esd_loss(tgt, pos, neu, unc, g_pred, g_loss, sign, half_n, loss, dpred) -> Op:
    return Op("leco_esd_loss", (ptr(tgt), ptr(pos), ptr(neu), ptr(unc), g_pred, g_loss, sign, half_n, ptr(loss),
                                ptr(dpred)))


def esd_loss_cond(tgt_c, pos_c, neu_c, unc_c, g_loss, sign, half_n, loss, dpred_c) -> Op:
    """The ESD objective on conditional-only predictions (the de-duplicated step: guidance_scale = 1 makes u + 1 (c - u) = c)."""
    return Op("leco_esd_loss_cond", (ptr(tgt_c), ptr(pos_c), ptr(neu_c), ptr(unc_c), g_loss, sign, half_n, ptr(loss), ptr(dpred_c)),
              keep=(tgt_c, pos_c, neu_c, unc_c, loss, dpred_c))


def adamw(p, g, m, v, shadow, hyper, beta1, beta2, eps, wd, n) -> Op:
    return Op("leco_adamw", (ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow), ptr(hyper), beta1, beta2, eps, wd, n))


def lion(p, g, m, shadow, hyper, beta1, beta2, wd, n) -> Op:
    return Op("leco_lion", (ptr(p), ptr(g), ptr(m), ptr(shadow), ptr(hyper), beta1, beta2, wd, n))


PRODIGY_DECOUPLE, PRODIGY_BIAS_CORRECTION, PRODIGY_SAFEGUARD_WARMUP = 1, 2, 4
PRODIGY_STATE_FIELDS = ("d", "d0", "d_max", "d_numerator", "d_denom", "d_hat", "dlr", "k")   # leco_prodigy_state


def prodigy_state(d0: float, device) -> torch.Tensor:
    """A fresh `leco_prodigy_state` (eight doubles) on `device`."""
    return torch.tensor([d0, d0, d0, 0.0, 0.0, d0, 0.0, 0.0], dtype=torch.float64, device=device)


def prodigy(p, g, m, v, s, p0, shadow, hyper, state, beta1, beta2, beta3, eps, wd, d_coef, growth_rate, decouple,
            use_bias_correction, safeguard_warmup, n) -> Op:
    """Two launches: moments + s + the two global sums + the scalar state, then the parameter update + bf16 shadow."""
    if state.dtype != torch.float64 or state.numel() != len(PRODIGY_STATE_FIELDS):
        raise ValueError("prodigy: state must be the 8 doubles of leco_prodigy_state (ops.prodigy_state)")
    flags = ((PRODIGY_DECOUPLE if decouple else 0) | (PRODIGY_BIAS_CORRECTION if use_bias_correction else 0)
             | (PRODIGY_SAFEGUARD_WARMUP if safeguard_warmup else 0))
    return Op("leco_prodigy", (ptr(p), ptr(g), ptr(m), ptr(v), ptr(s), ptr(p0), ptr(shadow), ptr(hyper), ptr(state),
                               float(beta1), float(beta2), float(beta3), float(eps), float(wd), float(d_coef),
                               float(growth_rate), flags, n), keep=(s, p0, state))


GRAD_STATS_FIELDS = ("norm", "coef", "nonfinite")          # stats[0..2] of leco_grad_clip


def grad_clip(g, hyper, max_norm, stats, n) -> Op:
    """norm of hyper[3] * g over the flat slab -> stats {norm, coef, non-finite count, 0}; hyper[3] *= coef when it clips
    (``max_norm == 0``: measure only).  One launch, before the optimizer kernel that reads hyper[3]."""
    if stats.dtype != torch.float32 or stats.numel() < 4 or hyper.dtype != torch.float32 or hyper.numel() < 4:
        raise ValueError("grad_clip: hyper and stats must be 4 fp32 values each")
    return Op("leco_grad_clip", (ptr(g), n, ptr(hyper), float(max_norm), ptr(stats)), keep=(g, hyper, stats))


def grad_accumulate(acc, g, n, first) -> Op:
    """acc = g (``first``) or acc + g: one micro-step of a gradient-accumulation group."""
    return Op("leco_grad_accumulate", (ptr(acc), ptr(g), n, 1 if first else 0), keep=(acc, g))


WEIGHT_NORM_STATS_FIELDS = ("keys_scaled", "avg_norm", "max_norm", "nonfinite")          # stats[0..3] of leco_lora_max_norm


def lora_norm_table(modules, device) -> torch.Tensor:
    """The module table of `leco_lora_max_norm` on ``device``: one `leco_lora_norm_module` (32 bytes) per entry of
    ``modules``, each ``(down_off, up_off, r, k, n, scale)`` -- element offsets into the slab, `lora_down` = [r][k],
    `lora_up` = [n][r].  Returned as a uint8 tensor of 32 * M bytes; uploaded once and reused by every launch."""
    rows = (hip.LoraNormModule * len(modules))()
    for row, (down_off, up_off, r, k, n, scale) in zip(rows, modules):
        row.down_off, row.up_off, row.r, row.k, row.n, row.scale = int(down_off), int(up_off), int(r), int(k), int(n), float(scale)
    return torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(device)


def lora_max_norm(slab, shadow, table, max_norm, norms, factors, stats) -> Op:
    """Max-norm regularisation over the modules of ``table`` (`lora_norm_table`): norms[m] = scale_m |up_m down_m|_F before
    scaling, modules above ``max_norm`` pulled back onto it (slab and bf16 shadow, factors[m] on both matrices), stats =
    {modules scaled, mean norm, max norm (after scaling), non-finite modules}.  ``max_norm == 0``: measure only."""
    M = table.numel() // C.sizeof(hip.LoraNormModule)
    if table.dtype != torch.uint8 or table.numel() != M * C.sizeof(hip.LoraNormModule):
        raise ValueError("lora_max_norm: table must come from lora_norm_table")
    if slab.dtype != torch.float32 or shadow.dtype != torch.bfloat16 or shadow.numel() != slab.numel():
        raise ValueError("lora_max_norm: slab must be fp32 and shadow its bf16 image of the same length")
    for name, t, need in (("norms", norms, M), ("factors", factors, M), ("stats", stats, 4)):
        if t.dtype != torch.float32 or t.numel() < need:
            raise ValueError(f"lora_max_norm: {name} must hold {need} fp32 values")
    return Op("leco_lora_max_norm", (ptr(slab), ptr(shadow), slab.numel(), ptr(table), M, float(max_norm), ptr(norms),
                                     ptr(factors), ptr(stats)), keep=(slab, shadow, table, norms, factors, stats))


def cast_f32_bf16(x, y, n) -> Op:
    return Op("leco_cast_f32_bf16", (ptr(x), ptr(y), n))


def memset(t: torch.Tensor, value: int = 0) -> Op:
    return Op("leco_memset", (ptr(t), value, t.numel() * t.element_size()))


def repeat(src: int, dst: int, nbytes: int, reps: int, keep=None) -> Op:
    """dst = `reps` back-to-back copies of the `nbytes` at src (raw device addresses)."""
    return Op("leco_repeat", (src, dst, nbytes, reps), keep=keep)


def step_begin(x: torch.Tensor, x2: torch.Tensor, scale: float, half_n: int, t_idx: Optional[torch.Tensor]) -> Op:
    """x2 = cat([scale x] * 2) in x2's dtype (bf16 / fp32), *t_idx = 0: the first UNet input of the denoising passes."""
    return Op("leco_step_begin", (ptr(x), ptr(x2), 1 if x2.dtype == torch.float32 else 0, float(scale), half_n, ptr(t_idx)),
              keep=(x, x2, t_idx))


def step_mid(src: torch.Tensor, dst_a: Optional[torch.Tensor], dst_b: Optional[torch.Tensor], reps_b: int, t_cur: float,
             plan_a, plan_b, slot: int) -> Op:
    """dst_a = src, dst_b = `reps_b` copies of src; both plans' timestep slot `slot` = t_cur and their step index -> slot."""
    nbytes = src.numel() * src.element_size()
    ta = None if plan_a is None else plan_a.t_table.data_ptr() + 4 * slot
    tb = None if plan_b is None else plan_b.t_table.data_ptr() + 4 * slot
    return Op("leco_step_mid", (ptr(src), ptr(dst_a), ptr(dst_b), nbytes, reps_b, float(t_cur), ta, tb,
                                None if plan_a is None else ptr(plan_a.t_idx), None if plan_b is None else ptr(plan_b.t_idx), slot),
              keep=(src, dst_a, dst_b))


def lora_pack(sites_dev: torch.Tensor, nsites: int) -> Op:
    return Op("leco_lora_pack", (ptr(sites_dev), nsites))


def lora_rowscale(t, ld, rows, cols, rows_per_sample, strengths, keep=None) -> Op:
    """t[m][c] *= strengths[m // rows_per_sample] in place (bf16 [rows][cols], row stride ``ld``; ``t`` may be a raw device
    address).  ``strengths``: fp32 DEVICE tensor [rows // rows_per_sample], read at launch / graph replay (bf16 only)."""
    if _f32_active:
        raise NotImplementedError("lora_rowscale (per-sample LoRA strengths) is implemented for the bf16 compute mode only")
    return Op("leco_lora_rowscale", (ptr(t), ld, rows, cols, rows_per_sample, ptr(strengths)), keep=(t, strengths, keep))


def lora_rowscale_stack(t, ld, rows, cols, rows_per_sample, strengths, files, col_file, period, keep=None) -> Op:
    """t[m][c] *= strengths[m // rows_per_sample][col_file[c % period]] in place: `lora_rowscale` for a stack of ``files``
    LoRA files (`LoRAStack`).  ``strengths``: fp32 DEVICE tensor [rows // rows_per_sample][files]; ``col_file``: int32 DEVICE
    tensor [period] (column of a module -> file), or a host list, which is checked and copied to the device of ``strengths``.
    Both are read at launch / graph replay (bf16 only)."""
    if _f32_active:
        raise NotImplementedError("lora_rowscale_stack (per-sample LoRA strengths) is implemented for the bf16 compute mode only")
    if not isinstance(col_file, torch.Tensor):
        table = [int(v) for v in col_file]
        if len(table) != period or any(v < 0 or v >= files for v in table):
            raise ValueError(f"lora_rowscale_stack: col_file must hold period={period} entries in 0..{files - 1}, got {table}")
        col_file = torch.tensor(table, dtype=torch.int32, device=strengths.device)
    return Op("leco_lora_rowscale_stack", (ptr(t), ld, rows, cols, rows_per_sample, ptr(strengths), files, ptr(col_file), period),
              keep=(t, strengths, col_file, keep))


def lora_wgrad(p, ldp, q, ldq, g, g_sj, g_sc, m, r, cols, scale, part: Optional[torch.Tensor] = None) -> Op:
    """p, q, g are raw device addresses (ints).  ``part``: fp32 scratch -> deterministic (atomic-free) accumulation."""
    return Op("leco_lora_wgrad", (p, ldp, q, ldq, g, g_sj, g_sc, m, r, cols, scale, ptr(part),
                                  0 if part is None else part.numel() * part.element_size()), keep=(part,))


def lora_wgrad_conv(p, ldp, q, ldq, g, g_sj, g_sc, m, r, cols, scale, a_mode, h_out, w_out, h_in, w_in, kh, kw,
                    part: Optional[torch.Tensor] = None) -> Op:
    """`lora_wgrad` with q gathered like tap (kh, kw) of a 3x3 convolution (a_mode A_CONV3_S1 / S2 / UP2)."""
    return Op("leco_lora_wgrad_conv", (p, ldp, q, ldq, g, g_sj, g_sc, m, r, cols, scale, a_mode, h_out, w_out, h_in, w_in, kh, kw,
                                       ptr(part), 0 if part is None else part.numel() * part.element_size()), keep=(part,))


def rowgroup_sum(x, ldx, out, ldo, groups, rows_per_group, cols) -> Op:
    """out[g][c] = sum of x[g * rows_per_group + r][c] over r (fp32 ``out``)."""
    return Op("leco_rowgroup_sum", (ptr(x), ldx, ptr(out), ldo, groups, rows_per_group, cols), keep=(x, out))


def lora_wgrad_grouped(problems: list, device) -> Optional[Op]:
    """ONE launch for a list of weight-gradient problems.  Each entry: dict(p, ldp, q, ldq, g, g_sj, g_sc, m, r, cols,
    scale[, a_mode, h_out, w_out, h_in, w_in, kh, kw]) with raw device addresses, as for `lora_wgrad` /
    leco_lora_wgrad_conv.  The problem table is built here and kept on the device."""
    if not problems:
        return None
    tab = (hip.WgradProblem * len(problems))()
    start = 0
    for d, pr in zip(tab, problems):
        for k, v in pr.items():
            setattr(d, k, v)
        d.blocks_x = -(-pr["cols"] // 256)
        d.block_start = start
        start += d.blocks_x * -(-pr["m"] // 128)
    raw = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(device)
    return Op("leco_lora_wgrad_grouped", (raw.data_ptr(), len(problems), start, max(pr["r"] for pr in problems)), keep=(raw,))


# ---- row-stripe fused transformer-block kernels (csrc/stripe.hip; bf16, forward-only plans) ---------------------------------
def xblock_supported(c: int, heads: int, skv: int, rows_per_sample: int) -> bool:
    f = hip.declare("leco_xblock_supported", [_i32, _i32, _i32, _i32])
    return bool(f(c, heads, skv, rows_per_sample))


def xattn_prep(kv_ptr: int, ld_kv: int, kp: torch.Tensor, vt: torch.Tensor, batch: int, heads: int, skv: int, head_dim: int) -> Op:
    """Cross-attention K / V^T operand images for `xblock_tail` (once per step: they depend only on the prompt)."""
    return Op("leco_xattn_prep", (kv_ptr, ld_kv, ptr(kp), ptr(vt), batch, heads, skv, head_dim), keep=(kp, vt))


def xattn_buffers(batch: int, heads: int, head_dim: int, device) -> tuple:
    dv = (head_dim + 15) // 16 * 16
    return (torch.zeros(batch * heads * 80 * 64, dtype=torch.bfloat16, device=device),
            torch.zeros(batch * heads * dv * 96, dtype=torch.bfloat16, device=device))


def xblock_tail(args: "hip.XBlockTailArgs", keep=None) -> Op:
    """Tail of a BasicTransformerBlock (+ proj_out) as ONE launch (include/leco_hip.h `leco_xblock_tail_args`)."""
    return Op("leco_xblock_tail", (C.cast(C.pointer(args), _vp),), keep=(args, keep))


def xblock_head(args: "hip.XBlockHeadArgs", keep=None) -> Op:
    """GroupNorm apply + proj_in + LayerNorm + q|k|v of a Transformer2DModel's first block as ONE launch (`leco_xblock_head_args`)."""
    return Op("leco_xblock_head", (C.cast(C.pointer(args), _vp),), keep=(args, keep))


def xgemm_supported(m: int, n: int, k: int) -> bool:
    f = hip.lib().leco_xgemm_supported
    f.argtypes, f.restype = [_i32, _i32, _i32], C.c_int
    return bool(f(m, n, k))


def xgemm(a_ptr: int, lda: int, lin: "hip.XLin", c_ptr: int, ldc: int, m: int, n: int, k: int, residual: Optional[int] = None,
          ldr: int = 0, keep=None) -> Op:
    """c = a lin.w^T (+ LoRA) + bias (+ residual) on the A-stationary kernel (include/leco_hip.h `leco_xgemm_args`)."""
    A = hip.XGemmArgs()
    A.m, A.n, A.k = m, n, k
    A.a, A.lda = a_ptr, lda
    A.lin = lin
    A.residual, A.ldr = residual, ldr
    A.c, A.ldc = c_ptr, ldc
    return Op("leco_xgemm", (C.cast(C.pointer(A), _vp),), keep=(A, lin, keep))


def deterministic_default() -> bool:
    """LECO_DETERMINISTIC=1: bitwise reproducible steps (LoRA wgrads without atomics; ~1-2 % slower)."""
    import os
    return os.environ.get("LECO_DETERMINISTIC", "0") not in ("", "0")

