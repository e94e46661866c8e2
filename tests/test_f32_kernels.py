"""Per-kernel parity of the fp32 compute mode (csrc/f32.hip, the `leco_f32_*` entry points): every kernel against the
same operation stated plainly in torch float64 on the CPU, from the same fp32 inputs (gradients by autograd on that
statement).  Runs on the host emulator of the kernel sources (CPU tier) and on the gfx950 build (`-m gpu`).

Bound: relative L2 (`conftest.rel_err`) < TOL32 = 1e-5, the bound `tests/test_kernels.py` states for results compared in
fp32; every measured error is printed (`-s` shows them; tabulated in DESIGN.md, section 4).

Guards: every output lives in a buffer with a leading dimension larger than its width and rows past M, pre-filled with
a finite sentinel, and everything outside the logical region must still hold the sentinel after the launch; inputs have
padded leading dimensions filled with junk, so a kernel that strides by a width reads wrong data."""
import errno
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from leco_amd import hip, ops

TOL32 = 1e-5
SENT = 12345.0      # finite (not NaN): the emulator's LDS poison mode stays distinguishable
JUNK = 777.0
f64 = torch.float64


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _in(t, dev, pad=4, rows=1):
    """Device buffer [rows(t) + rows][cols(t) + pad] holding the 2-D view of `t`, junk elsewhere."""
    t2 = t.reshape(-1, t.shape[-1]).float()
    b = torch.full((t2.shape[0] + rows, t2.shape[1] + pad), JUNK)
    b[:t2.shape[0], :t2.shape[1]] = t2
    return b.to(dev)


def _out(m, n, dev, pad=3, rows=2):
    return torch.full((m + rows, n + pad), SENT, device=dev)


def _flat(n, dev, extra=7):
    return torch.full((n + extra,), SENT, device=dev)


def _guard(buf, m, n):
    """The logical [m][n] region of an output buffer (on the host); everything else must be untouched."""
    c = buf.cpu()
    assert bool((c[m:] == SENT).all()) and bool((c[:m, n:] == SENT).all()), "wrote outside the logical region"
    return c[:m, :n]


def _guard_flat(buf, n):
    c = buf.cpu()
    assert bool((c[n:] == SENT).all()), "wrote past the end"
    return c[:n]


def _check(name, got, ref, tol=TOL32):
    e = rel_err(got, ref)
    print(f"[f32] {name}: {e:.3e} (bound {tol:.1e})")
    assert e < tol, (name, e, tol)
    return e


def _run(op, dev):
    op.run()
    _sync(dev)


# ---------------------------------------------------------------------------------------------------------------------
# 1. leco_f32_gemm, plain
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,ext_k,k_split,outs", [
    (100, 72, 128, 0, 0, "c"),
    (70, 64, 20, 0, 0, "c32"),        # K % 16 = 4, no extension: the last K chunk runs into nothing
    (129, 65, 36, 8, 0, "both"),      # the extension columns start in the middle of a 16-wide chunk
    (200, 130, 64, 0, 12, "both"),    # two sources, k_split % 16 != 0, different lda0 / lda1
])
def test_f32_gemm_plain(dev, M, N, K, ext_k, k_split, outs):
    torch.manual_seed(100 + K)
    a = torch.randn(M, K); w = torch.randn(N, K) / K ** 0.5
    bias = torch.randn(N); rb = torch.randn((M + 49) // 50, N); res = torch.randn(M, N)
    ae = torch.randn(M, ext_k); we = torch.randn(N, ext_k) * 0.1
    kw = {}
    if k_split:
        a0d, a1d = _in(a[:, :k_split], dev, pad=4), _in(a[:, k_split:], dev, pad=8)
        kw.update(a1=a1d, lda1=K - k_split + 8, k_split=k_split)
        lda = k_split + 4
    else:
        a0d, lda = _in(a, dev, pad=4), K + 4
    if ext_k:
        aed, wed = _in(ae, dev, pad=4), _in(we, dev, pad=8)
        kw.update(a_ext=aed, w_ext=wed, ext_k=ext_k, ld_aext=ext_k + 4, ld_wext=ext_k + 8)
    wd, bd, rbd, resd = _in(w, dev, pad=8), bias.to(dev), _in(rb, dev, pad=1), _in(res, dev, pad=5)
    c = _out(M, N, dev, pad=3) if outs in ("c", "both") else None
    c32 = _out(M, N, dev, pad=6) if outs in ("c32", "both") else None
    with ops.f32_mode(True):
        g = hip.gemm_args(a0d, wd, c, m=M, n=N, k=K, lda=lda, ldw=K + 8, bias=bd, rowbias=rbd, rows_per_group=50,
                          ld_rowbias=N + 1, residual=resd, ldr=N + 5, act=hip.ACT_SILU, ldc=N + 3, out_f32=c32, ldc32=N + 6, **kw)
        op = ops.gemm(g, keep=(a0d, wd, bd, rbd, resd, c, c32, kw))
    assert op.name == "leco_f32_gemm"
    _run(op, dev)
    ref = a.to(f64) @ w.to(f64).T + ae.to(f64) @ we.to(f64).T + bias.to(f64) + rb.to(f64).repeat_interleave(50, 0)[:M] + res.to(f64)
    ref = F.silu(ref)
    if c is not None:
        _check(f"gemm {M}x{N}x{K} c", _guard(c, M, N), ref)
    if c32 is not None:
        _check(f"gemm {M}x{N}x{K} c_f32", _guard(c32, M, N), ref)


def test_f32_gemm_mfma_layout_asymmetric(dev):
    """Identity A against an asymmetric W: a transposed fragment layout cannot pass (exact in fp32)."""
    M = N = K = 64
    a = torch.eye(M); w = torch.arange(N)[:, None] * 0.5 - torch.arange(K)[None, :] * 0.25
    ad, wd, c = _in(a, dev), _in(w, dev), _out(M, N, dev)
    with ops.f32_mode(True):
        op = ops.gemm(hip.gemm_args(ad, wd, c, m=M, n=N, k=K, lda=K + 4, ldw=K + 4, ldc=N + 3), keep=(ad, wd, c))
    _run(op, dev)
    assert torch.equal(_guard(c, M, N), w.T)


# ---------------------------------------------------------------------------------------------------------------------
# 2. leco_f32_gemm, implicit-GEMM 3x3 convolution: B = 2, 5 x 7 input, cin = 12 (k = 108, k % 16 = 12), Cout = 40
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,ext_k", [("s1", 0), ("s1", 4), ("s2", 0), ("up2", 0), ("up2", 64), ("tr2", 0), ("concat", 0)])
def test_f32_gemm_conv_modes(dev, mode, ext_k):
    torch.manual_seed(200 + ext_k)
    B, H, W_, Ci, Co = 2, 5, 7, 12, 40
    x = torch.randn(B, Ci, H, W_); bias = torch.randn(Co)
    xd = x.to(f64)
    if mode == "tr2":       # the input gradient of a stride-2 convolution: the 5 x 7 tensor is dy, the result is 9 x 13
        wt = torch.randn(Ci, Co, 3, 3) / (9 * Ci) ** 0.5          # conv_transpose2d layout [in][out][3][3]
        wh = wt.flip(2, 3).permute(1, 2, 3, 0).reshape(Co, 9 * Ci)
        ho, wo, amode = 2 * H - 1, 2 * W_ - 1, hip.A_CONV3_TR2
        ref = F.conv_transpose2d(xd, wt.to(f64), stride=2, padding=1)
    else:
        wt = torch.randn(Co, Ci, 3, 3) / (9 * Ci) ** 0.5
        wh = wt.permute(0, 2, 3, 1).reshape(Co, 9 * Ci)
        if mode == "s2":
            ho, wo, amode = (H + 1) // 2, (W_ + 1) // 2, hip.A_CONV3_S2
            ref = F.conv2d(xd, wt.to(f64), padding=1, stride=2)
        elif mode == "up2":
            ho, wo, amode = 2 * H, 2 * W_, hip.A_CONV3_UP2
            ref = F.conv2d(F.interpolate(xd, scale_factor=2.0, mode="nearest"), wt.to(f64), padding=1)
        else:
            ho, wo, amode = H, W_, hip.A_CONV3_S1
            ref = F.conv2d(xd, wt.to(f64), padding=1)
    assert tuple(ref.shape[2:]) == (ho, wo)
    M = B * ho * wo
    ref = ref.permute(0, 2, 3, 1).reshape(M, Co) + bias.to(f64)
    xh = x.permute(0, 2, 3, 1).reshape(B * H * W_, Ci)
    kw = {}
    if mode == "concat":    # channels [0, 4) from one tensor, [4, 12) from another
        a0d, a1d = _in(xh[:, :4], dev, pad=4), _in(xh[:, 4:], dev, pad=8)
        kw.update(a1=a1d, lda1=16, k_split=4)
        lda = 8
    else:
        a0d, lda = _in(xh, dev, pad=4), Ci + 4
    if ext_k:               # the c3lier LoRA branch: a low-rank image per OUTPUT pixel against scale * up
        ae = torch.randn(M, ext_k); we = torch.randn(Co, ext_k) * 0.1
        aed, wed = _in(ae, dev, pad=8), _in(we, dev, pad=4)
        kw.update(a_ext=aed, w_ext=wed, ext_k=ext_k, ld_aext=ext_k + 8, ld_wext=ext_k + 4)
        ref = ref + ae.to(f64) @ we.to(f64).T
    wd, bd = _in(wh, dev, pad=4), bias.to(dev)
    c, c32 = _out(M, Co, dev, pad=3), _out(M, Co, dev, pad=5)
    with ops.f32_mode(True):
        g = hip.gemm_args(a0d, wd, c, m=M, n=Co, k=9 * Ci, lda=lda, ldw=9 * Ci + 4, a_mode=amode, conv=(B, ho, wo, H, W_),
                          bias=bd, ldc=Co + 3, out_f32=c32, ldc32=Co + 5, **kw)
        op = ops.gemm(g, keep=(a0d, wd, bd, c, c32, kw))
    _run(op, dev)
    _check(f"conv {mode} ext_k={ext_k} c", _guard(c, M, Co), ref)
    _check(f"conv {mode} ext_k={ext_k} c_f32", _guard(c32, M, Co), ref)


# ---------------------------------------------------------------------------------------------------------------------
# 3. attention forward / backward
# ---------------------------------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, do, B, H, Sq, Skv, D, sc, dt=f64):
    qq, kk, vv = [t.to(dt).requires_grad_(True) for t in (q, k, v)]
    qh = qq.reshape(B, Sq, H, D).transpose(1, 2); kh = kk.reshape(B, Skv, H, D).transpose(1, 2)
    vh = vv.reshape(B, Skv, H, D).transpose(1, 2)
    s = (qh @ kh.transpose(-1, -2)) * sc
    o = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Sq, H * D)
    o.backward(do.to(dt))
    delta = (o.detach() * do.to(dt)).reshape(B, Sq, H, D).sum(-1).transpose(1, 2)      # [B][H][Sq]
    return o.detach(), torch.logsumexp(s, -1).detach(), delta, qq.grad, kk.grad, vv.grad, s.detach()


@pytest.mark.parametrize("B,H,Sq,Skv,D,gain,packed", [
    (2, 2, 70, 77, 40, 1.0, False),
    (1, 2, 65, 33, 80, 1.0, False),
    (1, 1, 64, 200, 160, 1.0, False),      # the backward asks for 140,288 B of dynamic LDS
    (2, 1, 50, 64, 64, 1.0, False),
    (1, 1, 1, 1, 4, 1.0, False),
    (2, 2, 48, 48, 40, 1.0, True),         # q|k|v in one [B][S][3C] buffer, dq|dk|dv likewise (the engine's self-attention)
    (1, 1, 40, 100, 40, 4.5, False),       # raw scores reach about +-60: the running maximum moves between key tiles
])
def test_f32_attention_fwd_bwd(dev, B, H, Sq, Skv, D, gain, packed):
    """o, lse, delta, dq, dk, dv against the float64 statement at TOL32.

    The "hot" case (scores up to +-75) is where fp32 itself comes closest to the bound: p = exp(s - lse) with |s| ~ 60 carries
    the rounding of s (ulp 4e-6), and dS = p (dP - delta) cancels.  For orientation the test prints the error of the same
    statement evaluated by torch in float32 on the CPU (3.9e-6 dq / 3.7e-6 dk / 1.2e-6 dv); the kernel measures 5.2e-6 /
    4.9e-6 / 2.0e-6 on the emulator, 3.8e-6 / 3.5e-6 / 1.9e-6 on gfx950, and is held to TOL32 like every other case."""
    torch.manual_seed(300 + D + Sq)
    C = H * D
    sc = D ** -0.5
    q = torch.randn(B, Sq, C) * gain; k = torch.randn(B, Skv, C) * gain; v = torch.randn(B, Skv, C); do = torch.randn(B, Sq, C)
    o_ref, lse_ref, delta_ref, dq_ref, dk_ref, dv_ref, s_ref = _attn_ref(q, k, v, do, B, H, Sq, Skv, D, sc)
    if gain != 1.0:
        assert 40.0 < float(s_ref.abs().max()) < 90.0
        assert float(s_ref[..., :32].max(-1).values.sub(s_ref.max(-1).values).min()) < -1.0     # the maximum does move

    def rows(t, pad):       # [B][S][C] -> [B][S + 1][C + pad] buffer: padded row stride and a padded batch stride
        b = torch.full((t.shape[0], t.shape[1] + 1, t.shape[2] + pad), JUNK)
        b[:, :t.shape[1], :t.shape[2]] = t
        return b.to(dev)

    def orows(S, cols, pad):
        return torch.full((B, S + 2, cols + pad), SENT, device=dev)

    def oguard(buf, S, c0, c1, width):      # logical [:, :S, c0:c1]; [:, :, width:] and rows past S stay untouched
        c = buf.cpu()
        assert bool((c[:, S:] == SENT).all()) and bool((c[:, :S, width:] == SENT).all()), "wrote outside the logical region"
        return c[:, :S, c0:c1]

    if packed:
        qkv = rows(torch.cat([q, k, v], -1), 5)
        ld = 3 * C + 5
        qa = (qkv.data_ptr(), ld, (Sq + 1) * ld); ka = (qkv.data_ptr() + 4 * C, ld, (Sq + 1) * ld)
        va = (qkv.data_ptr() + 8 * C, ld, (Sq + 1) * ld)
        dqkv = orows(Sq, 3 * C, 7)
        ldg = 3 * C + 7
        dqa = (dqkv.data_ptr(), ldg, (Sq + 2) * ldg); dka = (dqkv.data_ptr() + 4 * C, ldg, (Sq + 2) * ldg)
        dva = (dqkv.data_ptr() + 8 * C, ldg, (Sq + 2) * ldg)
    else:
        qd, kd, vd = rows(q, 3), rows(k, 5), rows(v, 9)
        qa = (qd.data_ptr(), C + 3, (Sq + 1) * (C + 3)); ka = (kd.data_ptr(), C + 5, (Skv + 1) * (C + 5))
        va = (vd.data_ptr(), C + 9, (Skv + 1) * (C + 9))
        dqd, dkd, dvd = orows(Sq, C, 1), orows(Skv, C, 2), orows(Skv, C, 6)
        dqa = (dqd.data_ptr(), C + 1, (Sq + 2) * (C + 1)); dka = (dkd.data_ptr(), C + 2, (Skv + 2) * (C + 2))
        dva = (dvd.data_ptr(), C + 6, (Skv + 2) * (C + 6))
    od = orows(Sq, C, 4)
    oa = (od.data_ptr(), C + 4, (Sq + 2) * (C + 4))
    dod = rows(do, 7)
    doa = (dod.data_ptr(), C + 7, (Sq + 1) * (C + 7))
    lse, delta = _flat(B * H * Sq, dev), _flat(B * H * Sq, dev)
    with ops.f32_mode(True):
        fwd = ops.attention_fwd(*qa, *ka, *va, *oa, lse, B, H, Sq, Skv, D, sc)
        bwd = ops.attention_bwd(*qa, *ka, *va, *oa, *doa, lse, delta, *dqa, *dka, *dva, B, H, Sq, Skv, D, sc)
    assert fwd.name == "leco_f32_attention_fwd" and bwd.name == "leco_f32_attention_bwd"
    _run(fwd, dev)
    _run(bwd, dev)       # D = 160: a refused dynamic-LDS request raises here (leco_f32_attention_bwd checks it)
    tag = f"attn B{B} H{H} {Sq}x{Skv} d{D}" + (" packed" if packed else "") + (" hot" if gain != 1.0 else "")
    _check(tag + " o", oguard(od, Sq, 0, C, C), o_ref)
    _check(tag + " lse", _guard_flat(lse, B * H * Sq), lse_ref.reshape(-1))
    _check(tag + " delta", _guard_flat(delta, B * H * Sq), delta_ref.reshape(-1))
    if packed:
        got = [oguard(dqkv, Sq, i * C, (i + 1) * C, 3 * C) for i in range(3)]
    else:
        got = [oguard(dqd, Sq, 0, C, C), oguard(dkd, Skv, 0, C, C), oguard(dvd, Skv, 0, C, C)]
    if gain != 1.0:
        r32 = _attn_ref(q, k, v, do, B, H, Sq, Skv, D, sc, torch.float32)[3:6]
        e32 = [rel_err(a_, b_) for a_, b_ in zip(r32, (dq_ref, dk_ref, dv_ref))]
        print(f"[f32] {tag} torch-float32 dq / dk / dv: " + " / ".join(f"{e:.3e}" for e in e32))
    for name, g_, r_ in zip(("dq", "dk", "dv"), got, (dq_ref, dk_ref, dv_ref)):
        _check(f"{tag} {name}", g_, r_)


# ---------------------------------------------------------------------------------------------------------------------
# 4. norms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,C0,C1,G,act,std", [
    (2, 70, 64, 0, 32, 1, 1.0),
    (3, 33, 64, 128, 32, 0, 1.0),       # two sources
    (1, 300, 320, 0, 32, 1, 1.0),       # cg = 10
    (2, 9, 640, 0, 32, 0, 1.0),         # cg = 20
    (2, 70, 64, 0, 32, 1, 0.05),        # var = 2.5e-3: eps = 1e-5 moves the output by 2e-3
    (2, 33, 64, 128, 32, 0, 0.05),
])
def test_f32_groupnorm_fwd_bwd(dev, B, HW, C0, C1, G, act, std):
    torch.manual_seed(400 + C0 + HW)
    C, eps = C0 + C1, 1e-5
    x0 = torch.randn(B * HW, C0) * std + 0.3
    x1 = (torch.randn(B * HW, C1) * 2 * std + 0.5) if C1 else None
    gamma = torch.randn(C) * 0.5 + 1.0; beta = torch.randn(C); dy = torch.randn(B * HW, C)
    x0d = _in(x0, dev, pad=3); x1d = _in(x1, dev, pad=5) if C1 else None
    gd, bd, dyd = gamma.to(dev), beta.to(dev), _in(dy, dev, pad=2)
    y, dx, stats = _out(B * HW, C, dev, pad=7), _out(B * HW, C, dev, pad=1), _flat(B * G * 2, dev)
    with ops.f32_mode(True):
        fwd = ops.groupnorm_fwd(x0d, C0 + 3, x1d, C1 + 5, C0, gd, bd, B, HW, C, G, eps, act, stats, y, C + 7)
        bwd = ops.groupnorm_bwd(x0d, C0 + 3, x1d, C1 + 5, C0, dyd, C + 2, gd, bd, stats, B, HW, C, G, eps, act, None, dx, C + 1)
    assert fwd.name == "leco_f32_groupnorm_fwd" and bwd.name == "leco_f32_groupnorm_bwd"
    _run(fwd, dev)
    _run(bwd, dev)
    xc = (torch.cat([x0, x1], 1) if C1 else x0).to(f64).reshape(B, HW, C).permute(0, 2, 1).requires_grad_(True)
    ref = F.group_norm(xc, G, gamma.to(f64), beta.to(f64), eps)
    ref = F.silu(ref) if act else ref
    ref.backward(dy.to(f64).reshape(B, HW, C).permute(0, 2, 1))
    xg = xc.detach().reshape(B, G, (C // G) * HW)
    st_ref = torch.stack([xg.mean(-1), (xg.var(-1, unbiased=False) + eps).rsqrt()], -1).reshape(-1)
    tag = f"groupnorm B{B} HW{HW} C{C0}+{C1} act{act} std{std}"
    _check(tag + " y", _guard(y, B * HW, C), ref.detach().permute(0, 2, 1).reshape(B * HW, C))
    _check(tag + " stats", _guard_flat(stats, B * G * 2), st_ref)
    _check(tag + " dx", _guard(dx, B * HW, C), xc.grad.permute(0, 2, 1).reshape(B * HW, C))


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("M,C,std", [(37, 320, 1.5), (9, 1280, 1.5), (5, 64, 1.5), (1, 4, 1.5), (37, 320, 0.05)])
def test_f32_layernorm_fwd_bwd(dev, M, C, std, with_dres):
    torch.manual_seed(500 + C)
    eps = 1e-5
    x = torch.randn(M, C) * std + 0.3; gamma = torch.randn(C) * 0.5 + 1.0; beta = torch.randn(C)
    dy = torch.randn(M, C); dres = torch.randn(M, C)
    xd, gd, bd, dyd = _in(x, dev, pad=3), gamma.to(dev), beta.to(dev), _in(dy, dev, pad=5)
    dresd = _in(dres, dev, pad=2) if with_dres else None
    y, dx, mean, rstd = _out(M, C, dev, pad=1), _out(M, C, dev, pad=6), _flat(M, dev), _flat(M, dev)
    with ops.f32_mode(True):
        fwd = ops.layernorm_fwd(xd, C + 3, gd, bd, eps, M, C, y, C + 1, mean, rstd)
        bwd = ops.layernorm_bwd(xd, C + 3, dyd, C + 5, gd, mean, rstd, dresd, C + 2, M, C, dx, C + 6)
    assert fwd.name == "leco_f32_layernorm_fwd" and bwd.name == "leco_f32_layernorm_bwd"
    _run(fwd, dev)
    _run(bwd, dev)
    xx = x.to(f64).requires_grad_(True)
    ref = F.layer_norm(xx, (C,), gamma.to(f64), beta.to(f64), eps)
    ref.backward(dy.to(f64))
    dx_ref = xx.grad + (dres.to(f64) if with_dres else 0.0)
    tag = f"layernorm {M}x{C} std{std} dres{int(with_dres)}"
    _check(tag + " y", _guard(y, M, C), ref.detach())
    _check(tag + " mean", _guard_flat(mean, M), xx.detach().mean(-1))
    _check(tag + " rstd", _guard_flat(rstd, M), (xx.detach().var(-1, unbiased=False) + eps).rsqrt())
    _check(tag + " dx", _guard(dx, M, C), dx_ref)


# ---------------------------------------------------------------------------------------------------------------------
# 5. elementwise, glue and LoRA kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_f32_geglu_fwd_bwd(dev):
    torch.manual_seed(600)
    M, Fd = 33, 128
    u = torch.randn(M, 2 * Fd); dy = torch.randn(M, Fd)
    ud, dyd = _in(u, dev, pad=4), _in(dy, dev, pad=1)
    y, du = _out(M, Fd, dev, pad=3), _out(M, 2 * Fd, dev, pad=5)
    with ops.f32_mode(True):
        fwd = ops.geglu_fwd(ud, 2 * Fd + 4, y, Fd + 3, M, Fd)
        bwd = ops.geglu_bwd(ud, 2 * Fd + 4, dyd, Fd + 1, du, 2 * Fd + 5, M, Fd)
    _run(fwd, dev)
    _run(bwd, dev)
    uu = u.to(f64).requires_grad_(True)
    a, g = uu.chunk(2, -1)
    ref = a * F.gelu(g)
    ref.backward(dy.to(f64))
    _check("geglu y", _guard(y, M, Fd), ref.detach())
    _check("geglu du", _guard(du, M, 2 * Fd), uu.grad)


@pytest.mark.parametrize("three", [False, True])
def test_f32_add(dev, three):
    torch.manual_seed(610)
    M, N = 10, 61
    a, b, c = torch.randn(M, N), torch.randn(M, 2 * N), torch.randn(M, N)
    ad, bd, cd = _in(a, dev, pad=3), _in(b, dev, pad=2), _in(c, dev, pad=5)
    o = _out(M, N, dev, pad=4)
    with ops.f32_mode(True):        # b: a column-offset view of a wider buffer
        op = ops.add(ad.data_ptr(), N + 3, bd.data_ptr() + 4 * N, 2 * N + 2, cd.data_ptr() if three else None, N + 5, o.data_ptr(),
                     N + 4, M, N)
    assert op.name == "leco_f32_add"
    _run(op, dev)
    ref = a.to(f64) + b[:, N:].to(f64) + (c.to(f64) if three else 0.0)
    _check(f"add {3 if three else 2} operands", _guard(o, M, N), ref)


def test_f32_upsample2x_bwd(dev):
    torch.manual_seed(620)
    B, H, W, C = 2, 3, 5, 12
    dyh = torch.randn(B, 2 * H, 2 * W, C)
    dyd, dx = dyh.to(dev), _flat(B * H * W * C, dev)
    with ops.f32_mode(True):
        op = ops.upsample2x_bwd(dyd, dx, B, H, W, C)
    _run(op, dev)
    xx = torch.zeros(B, C, H, W, dtype=f64, requires_grad=True)
    F.interpolate(xx, scale_factor=2.0, mode="nearest").backward(dyh.to(f64).permute(0, 3, 1, 2))
    _check("upsample2x_bwd", _guard_flat(dx, B * H * W * C).reshape(B, H, W, C), xx.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize("B,H,W,C", [(2, 6, 7, 128), (1, 3, 3, 320)])      # C % 64 != 0: a ragged last step of the wave reduction
def test_f32_conv_in_out(dev, B, H, W, C):
    torch.manual_seed(630 + C)
    Ci = 4
    x = torch.randn(B, Ci, H, W); w = torch.randn(C, Ci, 3, 3) * 0.2; bias = torch.randn(C)
    xd, wd, bd = x.to(dev), w.permute(1, 2, 3, 0).contiguous().to(dev), bias.to(dev)
    y = _flat(B * H * W * C, dev)
    with ops.f32_mode(True):
        op = ops.conv_in(xd, wd, bd, y, B, H, W, Ci, C)
    assert op.name == "leco_f32_conv_in"
    _run(op, dev)
    ref = F.conv2d(x.to(f64), w.to(f64), bias.to(f64), padding=1)
    _check(f"conv_in {B}x{H}x{W} C{C}", _guard_flat(y, B * H * W * C).reshape(B, H, W, C), ref.permute(0, 2, 3, 1))
    xh = torch.randn(B, H, W, C); w4 = torch.randn(4, C, 3, 3) * 0.05; b4 = torch.randn(4); dyo = torch.randn(B, 4, H, W)
    xhd, wl, b4d, dyod = xh.to(dev), w4.permute(0, 2, 3, 1).contiguous().to(dev), b4.to(dev), dyo.to(dev)
    yo, dxh = _flat(B * 4 * H * W, dev), _flat(B * H * W * C, dev)
    with ops.f32_mode(True):
        fwd = ops.conv_out(xhd, wl, b4d, yo, B, H, W, C, 4)
        bwd = ops.conv_out_bwd(dyod, wl, dxh, B, H, W, C, 4)
    _run(fwd, dev)
    _run(bwd, dev)
    xx = xh.to(f64).permute(0, 3, 1, 2).requires_grad_(True)
    ref = F.conv2d(xx, w4.to(f64), b4.to(f64), padding=1)
    ref.backward(dyo.to(f64))
    _check(f"conv_out {B}x{H}x{W} C{C}", _guard_flat(yo, B * 4 * H * W).reshape(B, 4, H, W), ref.detach())
    _check(f"conv_out_bwd {B}x{H}x{W} C{C}", _guard_flat(dxh, B * H * W * C).reshape(B, H, W, C), xx.grad.permute(0, 2, 3, 1))


def test_f32_timestep_embedding(dev):
    """out[i] = [cos(t_i f_j) | sin(t_i f_j)], f_j = 10000^(-j / half), t_i = t_table[*idx + i * stride].

    Timesteps here are <= 20 on purpose: cos(a) moves by |a| eps_a, and an fp32 evaluation of a = t exp(-9.21 j / half)
    carries a relative error of up to ~7e-7 (the exponent's own rounding, 9.21 * 6e-8, plus expf), i.e. 7e-4 absolute
    at t = 999 -- no fp32 kernel is within 1e-5 of the float64 statement there.  At t <= 20 that intrinsic error is
    <= 20 * (0.37 * 6e-8 + 1.2e-7) ~ 3e-6 on the worst element, so the 1e-5 bound tests the kernel, not the format."""
    tt = torch.tensor([3.0, 17.5, 0.0, 1.0, 9.25, 20.0, 12.0])
    idx = torch.tensor([1], dtype=torch.int32)
    n, dim, stride = 3, 320, 2
    ttd, idxd, out = tt.to(dev), idx.to(dev), _flat(n * dim, dev)
    with ops.f32_mode(True):
        op = ops.timestep_embedding(ttd, idxd, stride, n, dim, out)
    assert op.name == "leco_f32_timestep_embedding"
    _run(op, dev)
    half = dim // 2
    t = tt.to(f64)[[1, 3, 5]]
    a = t[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=f64) / half)[None, :]
    _check("timestep_embedding", _guard_flat(out, n * dim).reshape(n, dim), torch.cat([a.cos(), a.sin()], -1))


@pytest.mark.parametrize("n_hist,with_noise", [(-1, False), (0, False), (0, True), (1, False), (1, True), (3, False), (3, True)])
def test_f32_cfg_steps(dev, n_hist, with_noise):
    """n_hist = -1: leco_f32_cfg_ddim_step (two-coefficient rows); else leco_f32_cfg_sched_step on LECO_SCHED_ROW-wide rows."""
    torch.manual_seed(640 + n_hist)
    half, g, st = 1000, 3.0, 2
    pred, x, noise = torch.randn(2 * half), torch.randn(half), torch.randn(half)
    hist = torch.randn(max(n_hist, 1), half)
    ddim = n_hist < 0
    coef = torch.randn(4, 2 if ddim else 12)
    predd, coefd, std_ = pred.to(dev), coef.to(dev), torch.tensor([st], dtype=torch.int32).to(dev)
    xd, x2d, histd = _flat(half, dev), _flat(2 * half, dev), _flat(max(n_hist, 1) * half, dev)
    xd[:half] = x.to(dev)
    histd[:hist.numel()] = hist.reshape(-1).to(dev)
    noised = noise.to(dev) if with_noise else None
    with ops.f32_mode(True):
        if ddim:
            op = ops.cfg_ddim_step(predd, xd, x2d, coefd, std_, g, half)
        else:
            op = ops.cfg_sched_step(predd, xd, x2d, coefd, std_, g, half, noised, histd if n_hist else None, n_hist)
    assert op.name == ("leco_f32_cfg_ddim_step" if ddim else "leco_f32_cfg_sched_step")
    _run(op, dev)
    r = coef[st].to(f64)
    out = pred[:half].to(f64) + g * (pred[half:].to(f64) - pred[:half].to(f64))
    xn = r[0] * x.to(f64) + r[1] * out
    tag = "cfg_ddim_step" if ddim else f"cfg_sched_step n_hist={n_hist} noise={int(with_noise)}"
    if ddim:
        s_in = 1.0
    else:
        s_in = r[6]
        if with_noise:
            xn = xn + r[2] * noise.to(f64)
        h = hist.to(f64)
        for j in range(n_hist):
            xn = xn + r[3 + j] * h[j]
        h_new = torch.cat([(r[7] * x.to(f64) + r[8] * out)[None], h[:n_hist - 1]], 0) if n_hist else None
    _check(tag + " x", _guard_flat(xd, half), xn)
    _check(tag + " x2", _guard_flat(x2d, 2 * half), torch.cat([s_in * xn, s_in * xn]))
    hh = _guard_flat(histd, max(n_hist, 1) * half).reshape(-1, half)
    if n_hist > 0:
        _check(tag + " hist", hh, h_new)
    else:
        assert torch.equal(hh, hist)      # no history: the buffer is not touched


def test_f32_cast_is_a_copy(dev):
    torch.manual_seed(650)
    n = 1000
    x = torch.randn(n)
    x[:4] = torch.tensor([0.0, -0.0, 1e-40, 3.0e38])
    xd, y = x.to(dev), _flat(n, dev)
    with ops.f32_mode(True):
        op = ops.cast_f32_bf16(xd, y, n)
    assert op.name == "leco_f32_cast_f32_bf16"
    _run(op, dev)
    assert torch.equal(_guard_flat(y, n).view(torch.int32), x.view(torch.int32))


def test_f32_rowgroup_sum(dev):
    torch.manual_seed(660)
    groups, rpg, cols = 3, 35, 50
    x = torch.randn(groups * rpg, cols)
    xd, out = _in(x, dev, pad=3), _out(groups, cols, dev, pad=5)
    with ops.f32_mode(True):
        op = ops.rowgroup_sum(xd, cols + 3, out, cols + 5, groups, rpg, cols)
    assert op.name == "leco_f32_rowgroup_sum"
    _run(op, dev)
    _check("rowgroup_sum", _guard(out, groups, cols), x.to(f64).reshape(groups, rpg, cols).sum(1))


def test_f32_lora_pack(dev):
    """Three sites in one launch: a Linear of rank 20, a grouped site (fused q|k|v: 3 groups of rank 4) and a 3x3 conv site
    (taps = 9); the four operand images as include/leco_hip.h documents them (`leco_lora_site`)."""
    torch.manual_seed(670)
    sites = [dict(groups=1, r=20, k=20, n=24, taps=0, scale=0.25), dict(groups=3, r=4, k=20, n=36, taps=0, scale=0.5),
             dict(groups=1, r=4, k=108, n=40, taps=9, scale=0.75)]
    tab = (hip.LoraSite * len(sites))()
    keep = []
    for s, site in zip(sites, tab):
        R = s["groups"] * s["r"]
        conv = s["taps"] == 9
        s["R"], s["Rp"] = R, 64 if conv else (R + 31) // 32 * 32
        s["rows_s"] = s["Rp"] if conv else (R + 15) // 16 * 16
        s["down"] = [torch.randn(s["r"], s["k"]) for _ in range(s["groups"])]
        s["up"] = [torch.randn(s["n"] // s["groups"], s["r"]) for _ in range(s["groups"])]
        dd, ud = [t.to(dev) for t in s["down"]], [t.to(dev) for t in s["up"]]
        keep += dd + ud
        for g in range(s["groups"]):
            site.down[g], site.up[g] = dd[g].data_ptr(), ud[g].data_ptr()
        site.groups, site.r, site.k, site.n, site.scale, site.taps = s["groups"], s["r"], s["k"], s["n"], s["scale"], s["taps"]
        s["bufs"] = [_flat(s["rows_s"] * s["k"], dev), _flat(s["n"] * s["Rp"], dev), _flat(s["rows_s"] * s["n"], dev),
                     _flat(s["k"] * s["Rp"], dev)]
        site.dn_s, site.up_p, site.up_t, site.dn_p = [b.data_ptr() for b in s["bufs"]]
    raw = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).clone().to(dev)
    with ops.f32_mode(True):
        op = ops.lora_pack(raw, len(sites))
    assert op.name == "leco_f32_lora_pack"
    _run(op, dev)
    for i, s in enumerate(sites):
        R, Rp, rows_s, k, n, sc = s["R"], s["Rp"], s["rows_s"], s["k"], s["n"], s["scale"]
        down = torch.cat(s["down"], 0).to(f64)                       # [R][k]
        upbd = torch.block_diag(*[u.to(f64) for u in s["up"]])       # [n][R]
        if s["taps"] == 9:
            cin = k // 9
            d4 = down.reshape(R, cin, 9)                             # lora_down [r][Cin][3][3]
            dn_s_ref = d4.permute(0, 2, 1).reshape(R, k)             # dn_s[j][tap * Cin + c]
            dn_p_ref = sc * d4.flip(2).permute(1, 2, 0).reshape(k, R)    # dn_p[c][tap][j] = scale * down[j][c][8 - tap]
        else:
            dn_s_ref, dn_p_ref = down, sc * down.T
        dn_s = _guard_flat(s["bufs"][0], rows_s * k).reshape(rows_s, k)
        up_p = _guard_flat(s["bufs"][1], n * Rp).reshape(n, Rp)
        up_t = _guard_flat(s["bufs"][2], rows_s * n).reshape(rows_s, n)
        dn_p = _guard_flat(s["bufs"][3], k * Rp).reshape(k, Rp)
        assert torch.equal(dn_s[:R].to(f64), dn_s_ref) and float(dn_s[R:].abs().sum()) == 0.0, i
        assert torch.equal(up_t[:R].to(f64), upbd.T) and float(up_t[R:].abs().sum()) == 0.0, i
        assert float(up_p[:, R:].abs().sum()) == 0.0 and float(dn_p[:, R:].abs().sum()) == 0.0, i
        _check(f"lora_pack site {i} up_p", up_p[:, :R], sc * upbd)
        _check(f"lora_pack site {i} dn_p", dn_p[:, :R], dn_p_ref)


@pytest.mark.parametrize("r", [4, 20])
@pytest.mark.parametrize("mode", ["wgrad", "plain", "s1", "s2", "up2"])
def test_f32_lora_wgrad(dev, mode, r):
    """G[j g_sj + c g_sc] += scale sum_m P[m][j] Q[row(m)][c]: leco_f32_lora_wgrad ("wgrad") and leco_f32_lora_wgrad_conv with
    Q gathered like tap (kh, kw) of a 3x3 convolution.  G starts non-zero (the kernel accumulates) and is strided as the
    engine strides a conv lora_down gradient (g_sj = 9 cols, g_sc = 9): the other eight taps' elements must not move."""
    torch.manual_seed(680 + r)
    B, cols, scale, kh, kw = 2, 12, 0.5, 2, 0
    hi, wi, ho, wo, amode = {"wgrad": (5, 7, 5, 7, hip.A_PLAIN), "plain": (5, 7, 5, 7, hip.A_PLAIN),
                             "s1": (5, 7, 5, 7, hip.A_CONV3_S1), "s2": (9, 13, 5, 7, hip.A_CONV3_S2),
                             "up2": (3, 4, 6, 8, hip.A_CONV3_UP2)}[mode]
    M = B * ho * wo
    P = torch.randn(M, r); Q = torch.randn(B * hi * wi, cols); G0 = torch.randn(r * cols * 9 + 5)
    Pd, Qd, Gd = _in(P, dev, pad=3), _in(Q, dev, pad=5), G0.clone().to(dev)
    tap_off = 4
    gp = Gd.data_ptr() + 4 * tap_off
    with ops.f32_mode(True):
        if mode == "wgrad":
            op = ops.lora_wgrad(Pd.data_ptr(), r + 3, Qd.data_ptr(), cols + 5, gp, 9 * cols, 9, M, r, cols, scale)
        else:
            op = ops.lora_wgrad_conv(Pd.data_ptr(), r + 3, Qd.data_ptr(), cols + 5, gp, 9 * cols, 9, M, r, cols, scale, amode, ho, wo,
                                     hi, wi, kh, kw)
    assert op.name == ("leco_f32_lora_wgrad" if mode == "wgrad" else "leco_f32_lora_wgrad_conv")
    _run(op, dev)
    q4 = Q.to(f64).reshape(B, hi, wi, cols)
    if amode == hip.A_PLAIN:
        qg = q4
    else:
        if mode == "up2":
            q4 = q4.repeat_interleave(2, 1).repeat_interleave(2, 2)
        sy = 2 if mode == "s2" else 1
        qp = F.pad(q4, (0, 0, 1, 1, 1, 1))      # output (oy, ox), tap (kh, kw) reads padded pixel (oy sy + kh, ox sy + kw)
        qg = qp[:, kh:kh + sy * (ho - 1) + 1:sy, kw:kw + sy * (wo - 1) + 1:sy]
    ref = G0.to(f64).clone()
    idx = tap_off + torch.arange(r)[:, None] * 9 * cols + torch.arange(cols)[None, :] * 9
    ref[idx] += scale * (P.to(f64).T @ qg.reshape(M, cols))
    got = Gd.cpu()
    touched = torch.zeros_like(G0, dtype=torch.bool)
    touched[idx] = True
    assert torch.equal(got[~touched], G0[~touched]), "wrote outside its tap"
    _check(f"lora_wgrad {mode} r={r}", got[touched], ref[touched])


# ---------------------------------------------------------------------------------------------------------------------
# 6. argument checks: nothing invalid is launched -- only the return code and the message are looked at
# ---------------------------------------------------------------------------------------------------------------------
def _rejected(op, entry):
    rc = op.fn(*op.args, ops.default_stream())
    msg = (hip.lib().leco_last_error() or b"").decode()
    assert rc == -errno.EINVAL, (rc, msg)
    assert entry in msg, msg


@pytest.mark.parametrize("what", ["t_w", "geglu", "pad01", "k_mod_4", "ld", "conv_m", "ext_without_a_ext", "ext_without_both"])
def test_f32_gemm_rejects(dev, what):
    M, N, K = 8, 8, 36
    buf = torch.zeros(64, 64, device=dev)
    kw = dict(m=M, n=N, k=K, lda=64, ldw=64, ldc=64)
    if what == "t_w":
        kw.update(t_w=buf, t_rows=16, w_ext=buf, ext_k=32)
    elif what == "geglu":
        kw.update(act=hip.ACT_GEGLU)
    elif what == "pad01":
        kw.update(a_mode=hip.A_CONV3_S2_PAD01, conv=(2, 2, 2, 4, 4))
    elif what == "k_mod_4":
        kw.update(k=18)
    elif what == "ld":
        kw.update(lda=62)
    elif what == "conv_m":
        kw.update(a_mode=hip.A_CONV3_S1, conv=(1, 3, 3, 3, 3))      # batch * h_out * w_out = 9 != m = 8
    elif what == "ext_without_a_ext":      # k % 16 != 0: the last K chunk would index off the null a_ext
        kw.update(w_ext=buf, ext_k=8, ld_wext=64)
    elif what == "ext_without_both":
        kw.update(ext_k=8)
    with ops.f32_mode(True):
        op = ops.gemm(hip.gemm_args(buf, buf, buf, **kw), keep=(buf,))
    _rejected(op, "leco_f32_gemm")


@pytest.mark.parametrize("d", [164, 42, 0])
def test_f32_attention_rejects_head_dim(dev, d):
    buf = torch.zeros(4096, device=dev)
    p = buf.data_ptr()
    with ops.f32_mode(True):
        fwd = ops.attention_fwd(p, 8, 64, p, 8, 64, p, 8, 64, p, 8, 64, buf, 1, 1, 4, 4, d, 1.0)
        bwd = ops.attention_bwd(p, 8, 64, p, 8, 64, p, 8, 64, p, 8, 64, p, 8, 64, buf, buf, p, 8, 64, p, 8, 64, p, 8, 64,
                                1, 1, 4, 4, d, 1.0)
    _rejected(fwd, "leco_f32_attention")
    _rejected(bwd, "leco_f32_attention")


def test_f32_groupnorm_rejects_ragged_groups(dev):
    buf = torch.zeros(4096, device=dev)
    with ops.f32_mode(True):
        fwd = ops.groupnorm_fwd(buf, 40, None, 0, 40, buf, buf, 1, 4, 40, 32, 1e-5, 0, buf, buf, 40)
        bwd = ops.groupnorm_bwd(buf, 40, None, 0, 40, buf, 40, buf, buf, buf, 1, 4, 40, 32, 1e-5, 0, None, buf, 40)
    _rejected(fwd, "leco_f32_groupnorm")
    _rejected(bwd, "leco_f32_groupnorm")


@pytest.mark.parametrize("amode", [hip.A_CONV3_TR2, hip.A_CONV3_S2_PAD01])
def test_f32_lora_wgrad_conv_rejects_modes_without_a_weight_gradient(dev, amode):
    """As the bf16 leco_lora_wgrad_conv: the transposed and the bottom / right padded gathers are refused by name (the
    kernel would otherwise gather them as stride 1)."""
    buf = torch.zeros(4096, device=dev)
    p = buf.data_ptr()
    with ops.f32_mode(True):
        op = ops.lora_wgrad_conv(p, 4, p, 4, p, 4, 1, 16, 4, 4, 1.0, amode, 4, 4, 4, 4, 0, 0)
    _rejected(op, "leco_f32_lora_wgrad_conv")
