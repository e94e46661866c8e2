"""Kernels added for the CLIP text encoder, each against a plain fp32 PyTorch statement of the same op on the same
bf16-rounded inputs: the causal attention core, the quick-GELU / erf-GELU GEMM epilogues and the embedding row gather.
Runs on the host emulator (CPU tier) and on the gfx950 build (`-m gpu`).  Bound: the project's bf16 bound of
tests/test_kernels.py (one bf16 rounding of the result, relative L2)."""
import ctypes as C
import errno
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from leco_amd import hip, ops

bf = torch.bfloat16
TOLBF = 3e-3
S_MAX = ops.CAUSAL_ATTN_MAX_S
D = 64


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _last_error() -> str:
    return (hip.lib().leco_last_error() or b"").decode()


def _causal_ref(q, k, v, H, scale):
    """softmax(q k^T scale + triu(-inf, 1)) v in fp32; q, k, v: [B][S][H * 64]."""
    B, S, _ = q.shape
    sp = lambda t: t.float().cpu().reshape(B, S, H, D).permute(0, 2, 1, 3)      # noqa: E731
    s = sp(q) @ sp(k).transpose(-1, -2) * scale + torch.full((S, S), float("-inf")).triu(1)
    return (torch.softmax(s, -1) @ sp(v)).permute(0, 2, 1, 3).reshape(B, S, H * D)


def _causal_run(dev, q, k, v, H, scale):
    """q, k, v: [B][S][*] views with unit column stride (token stride = stride(1), batch stride = stride(0))."""
    B, S = q.shape[:2]
    o = torch.zeros(B, S, H * D, dtype=bf, device=dev)
    ops.attention_causal_fwd(q.data_ptr(), q.stride(1), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0),
                             v.data_ptr(), v.stride(1), v.stride(0), o.data_ptr(), H * D, S * H * D, B, H, S, D, scale,
                             keep=(q, k, v, o)).run()
    _sync(dev)
    return o


@pytest.mark.parametrize("B,H,S", [(1, 1, 1), (1, 2, 16), (2, 3, 17), (2, 12, 77), (1, 2, S_MAX)])
def test_causal_attention_values(dev, B, H, S):
    """One row, exactly one 16-row block, one row past a block, CLIP's own shape (two key tiles), the largest S."""
    torch.manual_seed(20 + S)
    q, k, v = (torch.randn(B, S, H * D).to(bf).to(dev) for _ in range(3))
    scale = D ** -0.5
    o = _causal_run(dev, q, k, v, H, scale)
    err = rel_err(o.cpu(), _causal_ref(q, k, v, H, scale))
    print(f"causal attention B={B} H={H} S={S}: rel {err:.3e}")
    assert err < TOLBF


def test_causal_attention_fused_qkv_views(dev):
    """q | k | v as column views of one fused [B][S][3C] buffer (what the q|k|v GEMM of the encoder writes)."""
    torch.manual_seed(21)
    B, H, S = 2, 2, 33
    Cw = H * D
    qkv = torch.randn(B, S, 3 * Cw).to(bf).to(dev)
    q, k, v = qkv[..., :Cw], qkv[..., Cw:2 * Cw], qkv[..., 2 * Cw:]
    o = _causal_run(dev, q, k, v, H, 0.2)
    err = rel_err(o.cpu(), _causal_ref(q, k, v, H, 0.2))
    print(f"causal attention on fused views: rel {err:.3e}")
    assert err < TOLBF


def test_causal_attention_is_causal_bitwise(dev):
    """Replacing q, k and v of every token >= j leaves the output rows < j bitwise unchanged."""
    torch.manual_seed(22)
    B, H, S = 1, 2, 77
    q, k, v = (torch.randn(B, S, H * D).to(bf).to(dev) for _ in range(3))
    first = _causal_run(dev, q, k, v, H, D ** -0.5)
    for j in (1, 16, 17, 76):
        q2, k2, v2 = q.clone(), k.clone(), v.clone()
        for t in (q2, k2, v2):
            t[:, j:] = (torch.randn(B, S - j, H * D) * 3).to(bf).to(dev)
        second = _causal_run(dev, q2, k2, v2, H, D ** -0.5)
        assert torch.equal(first[:, :j].cpu().view(torch.int16), second[:, :j].cpu().view(torch.int16)), j
        assert not torch.equal(first[:, j:].cpu(), second[:, j:].cpu()), j


def test_causal_attention_rejections(dev):
    B, H, S = 1, 1, 8
    t = torch.zeros(B, 2 * S_MAX, 128, dtype=bf, device=dev)
    p = t.data_ptr()

    def call(q=p, k=p, v=p, o=p, s=S, d=D, ld=128):
        fn = ops.Op("leco_attention_causal_fwd", (q, ld, 0, k, ld, 0, v, ld, 0, o, ld, 0, B, H, s, d, 0.125), keep=(t,)).fn
        return fn(q, ld, 0, k, ld, 0, v, ld, 0, o, ld, 0, B, H, s, d, 0.125, ops.default_stream())
    assert call() == 0
    _sync(dev)
    assert call(d=40) == -errno.EINVAL and "head_dim" in _last_error()
    assert call(s=S_MAX + 1) == -errno.EINVAL and "s=" in _last_error()
    assert call(s=0) == -errno.EINVAL and "s=" in _last_error()
    assert call(k=None) == -errno.EINVAL and "(k)" in _last_error()
    assert call(o=None) == -errno.EINVAL and "(o)" in _last_error()
    assert call(ld=68) == -errno.EINVAL and "strides" in _last_error()
    # (the signature has ONE sequence length: sq != skv cannot be expressed)


# ---- GEMM epilogues -------------------------------------------------------------------------------------------------
ACTS = {hip.ACT_QUICK_GELU: lambda z: z * torch.sigmoid(1.702 * z), hip.ACT_GELU: F.gelu}
SHAPES = [(77, 512, 128), (154, 3072, 768)]
_gemm_cache = {}


def _gemm_case(M, N, K):
    """Operands and the fp32 pre-activation reference, computed once per shape and shared (never modified)."""
    if (M, N, K) not in _gemm_cache:
        g = torch.Generator().manual_seed(30 + M)
        a = torch.randn(M, K, generator=g).to(bf)
        w = (torch.randn(N, K, generator=g) / K ** 0.5).to(bf)
        bias = torch.randn(N, generator=g)
        _gemm_cache[(M, N, K)] = (a, w, bias, a.float() @ w.float().T + bias)
    return _gemm_cache[(M, N, K)]


@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_gelu_epilogues_every_tile(dev, act, M, N, K):
    """C = act(acc + bias) through leco_gemm and through every tile id of leco_gemm_tile that accepts the shape; ids 7..10
    (the patch convolution) fall back to the heuristic for a plain operand, 2 needs n % 160 == 0 beyond one tile."""
    a, w, bias, pre = _gemm_case(M, N, K)
    ref = ACTS[act](pre)
    ad, wd, bd = a.to(dev), w.to(dev), bias.to(dev)
    lib = hip.lib()
    ran = []
    for tile in ("gemm", 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11):
        out = torch.zeros(M, N, dtype=bf, device=dev)
        o32 = torch.zeros(M, N, device=dev)
        g = hip.gemm_args(ad, wd, out, m=M, n=N, k=K, bias=bd, act=act, out_f32=o32)
        rc = lib.leco_gemm(C.byref(g), ops.default_stream()) if tile == "gemm" else \
            lib.leco_gemm_tile(C.byref(g), tile, ops.default_stream())
        _sync(dev)
        if rc != 0:
            assert rc == -errno.EINVAL, (tile, rc, _last_error())
            continue
        ran.append(tile)
        e32, e16 = rel_err(o32.cpu(), ref), rel_err(out.cpu(), ref)
        print(f"act {act} {M}x{N}x{K} tile {tile}: fp32 copy rel {e32:.3e}, bf16 rel {e16:.3e}")
        # the fp32 copy carries no output rounding: 1e-5 for the MFMA sum + the fast exp / erf (|err| <= 1.5e-7 absolute)
        assert e32 < 1e-5 and e16 < TOLBF, (tile, e32, e16)
    assert {"gemm", 0, 1, 3, 4, 5, 6, 11} <= set(ran), ran


@pytest.mark.parametrize("act", sorted(ACTS))
def test_gemm_gelu_epilogues_under_split_k(dev, act):
    """split_k = 2: the finishing kernel applies the activation (bias and residual in front of it)."""
    M, N, K = SHAPES[0]
    a, w, bias, pre = _gemm_case(M, N, K)
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(31)).to(bf)
    ref = ACTS[act](pre + res.float())
    out = torch.zeros(M, N, dtype=bf, device=dev)
    ws = torch.empty(2 * M * N, device=dev)
    g = hip.gemm_args(a.to(dev), w.to(dev), out, m=M, n=N, k=K, bias=bias.to(dev), residual=res.to(dev), act=act)
    for tile in (1, 3):
        out.zero_()
        assert "split=2" in hip.gemm_describe(g, tile, 2, ws.data_ptr(), ws.numel() * 4)
        hip.gemm(g, ops.default_stream(), tile, 2, ws)
        _sync(dev)
        err = rel_err(out.cpu(), ref)
        print(f"act {act} split-K tile {tile}: rel {err:.3e}")
        assert err < TOLBF


@pytest.mark.parametrize("act", sorted(ACTS))
def test_other_gemm_entry_points_never_drop_the_activation(dev, act):
    """leco_f32_gemm rejects the new values (its epilogue knows NONE / SILU); leco_xgemm and the stripe chains have no
    act argument at all, so they cannot be handed one; an act outside the enum is an error everywhere."""
    M, N, K = 64, 64, 64
    a, w = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev)
    out = torch.zeros(M, N, device=dev)
    g = hip.gemm_args(a, w, out, m=M, n=N, k=K, act=act)
    with ops.f32_mode():
        op = ops.gemm(g)
    rc = op.fn(*op.args, ops.default_stream())
    _sync(dev)
    if rc == 0:      # an implementation is allowed -- then it must be right
        assert rel_err(out.cpu(), ACTS[act](a.float().cpu() @ w.float().cpu().T)) < 1e-5
    else:
        assert rc == -errno.EINVAL and "act" in _last_error()
    assert "act" not in {f for f, _ in hip.XGemmArgs._fields_} | {f for f, _ in hip.XLin._fields_}
    assert "act" not in {f for f, _ in hip.XBlockTailArgs._fields_} | {f for f, _ in hip.XBlockHeadArgs._fields_}
    ab, wb = a.to(bf), w.to(bf)
    gb = hip.gemm_args(ab, wb, torch.zeros(M, N, dtype=bf, device=dev), m=M, n=N, k=K, act=7)
    assert hip.lib().leco_gemm(C.byref(gb), ops.default_stream()) == -errno.EINVAL and "act" in _last_error()


# ---- embedding gather -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_pos", [True, False])
def test_embed_rows(dev, with_pos):
    torch.manual_seed(40)
    vocab, Cw, S, B = 50, 136, 7, 3
    table = torch.randn(vocab, Cw).to(bf).to(dev)
    pos = torch.randn(S, Cw).to(bf).to(dev) if with_pos else None
    ids = torch.randint(0, vocab, (B, S))
    ids[0, 0], ids[1, 3], ids[2, 6] = 0, vocab - 1, vocab - 1
    out = torch.zeros(B * S, Cw, dtype=bf, device=dev)
    ops.embed_rows_checked(table, ids, pos, S, out).run()
    _sync(dev)
    ref = table.float().cpu()[ids.reshape(-1)]
    if with_pos:
        ref = ref + pos.float().cpu().repeat(B, 1)
    assert torch.equal(out.cpu(), ref.to(bf))       # the fp32 sum rounded once: exact


def test_embed_rows_rejects_an_id_outside_the_table_on_the_host(dev):
    vocab, Cw = 50, 64
    table = torch.zeros(vocab, Cw, dtype=bf, device=dev)
    out = torch.zeros(4, Cw, dtype=bf, device=dev)
    for bad in (vocab, -1):
        with pytest.raises(IndexError, match=str(bad)):
            ops.embed_rows_checked(table, torch.tensor([0, 1, bad, 2]), None, 1, out)
    rc = hip.lib().leco_embed_rows      # the C side rejects what it cannot vectorise
    idx = torch.zeros(4, dtype=torch.int32, device=dev)
    op = ops.embed_rows(table, Cw, vocab, idx, None, 0, 1, out, Cw, 4, 60)
    assert op.fn(*op.args, ops.default_stream()) == -errno.EINVAL and "c=60" in _last_error()
    assert rc is not None and math.isfinite(float(out.float().sum()))
