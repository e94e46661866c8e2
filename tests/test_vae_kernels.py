"""Kernels the VAE decoder adds: the wide-head (d = 512 / 128) flash attention forward and the RGB output convolution with
its 8-bit image epilogue -- each against fp32 PyTorch, on the host emulator of the kernel sources and (marked `gpu`) on
gfx950.  Also the decoder's largest launches (1024^2 images) on the GPU, where a 32-bit index product would show."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from leco_amd import hip, ops

bf = torch.bfloat16
TOLBF = 3e-3          # the project's bf16 bound (tests/test_kernels.py)


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _attn_ref(q, k, v, scale):
    return torch.softmax(q.float() @ k.float().transpose(-1, -2) * scale, -1) @ v.float()


def _run_wide(dev, B, Sq, Skv, D, lse=None):
    q = torch.randn(B, Sq, D).to(bf).to(dev); k = torch.randn(B, Skv, D).to(bf).to(dev); v = torch.randn(B, Skv, D).to(bf).to(dev)
    o = torch.zeros(B, Sq, D, dtype=bf, device=dev)
    ops.attention_fwd(q.data_ptr(), D, Sq * D, k.data_ptr(), D, Skv * D, v.data_ptr(), D, Skv * D, o.data_ptr(), D, Sq * D,
                      lse, B, 1, Sq, Skv, D, D ** -0.5).run()
    _sync(dev)
    return q, k, v, o


@pytest.mark.parametrize("B,Sq,Skv", [(1, 64, 64), (2, 960, 960), (1, 192, 320)])
def test_attention_wide_head_512(dev, B, Sq, Skv):
    """One tile; 24x40 latents (ragged last tile, batch stride); Sq != Skv.  lse = NULL is accepted."""
    torch.manual_seed(60)
    D = 512
    q, k, v, o = _run_wide(dev, B, Sq, Skv, D)
    e = rel_err(o.cpu(), _attn_ref(q.cpu(), k.cpu(), v.cpu(), D ** -0.5))
    print(f"wide attention d=512 B={B} Sq={Sq} Skv={Skv}: rel {e:.3e}")
    assert e < TOLBF


@pytest.mark.parametrize("B,Sq,Skv", [(2, 70, 70), (1, 1, 1), (1, 130, 65)])
def test_attention_wide_head_128(dev, B, Sq, Skv):
    """The tiny synthetic decoder's width; ragged tiles on both sides, a single row / key, and the saved lse."""
    torch.manual_seed(61)
    D = 128
    lse = torch.zeros(B, 1, Sq, device=dev)
    q, k, v, o = _run_wide(dev, B, Sq, Skv, D, lse)
    s = q.cpu().float() @ k.cpu().float().transpose(-1, -2) * D ** -0.5
    assert rel_err(o.cpu(), torch.softmax(s, -1) @ v.cpu().float()) < TOLBF
    assert (lse.cpu()[:, 0] - torch.logsumexp(s, -1)).abs().max().item() < 1e-3


@pytest.mark.gpu
def test_attention_wide_head_512_real_mid_block():
    """S = 4096: the mid-block attention of a 512^2 decode (64x64 latents)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conftest import _bind_hip
    _bind_hip()
    dev = torch.device("cuda:0")
    torch.manual_seed(62)
    D, S = 512, 4096
    q, k, v, o = _run_wide(dev, 1, S, S, D)
    e = rel_err(o, _attn_ref(q, k, v, D ** -0.5))
    print(f"wide attention d=512 S=4096: rel {e:.3e}")
    assert e < TOLBF


def test_attention_wide_head_strided_fused_qkv(dev):
    """q | k | v as column views of one [B][S][3C] buffer (how the decoder plan lays them out)."""
    torch.manual_seed(63)
    B, S, D = 2, 100, 512
    qkv = torch.randn(B, S, 3 * D).to(bf).to(dev)
    o = torch.zeros(B, S, D, dtype=bf, device=dev)
    p0 = qkv.data_ptr()
    ops.attention_fwd(p0, 3 * D, S * 3 * D, p0 + 2 * D, 3 * D, S * 3 * D, p0 + 4 * D, 3 * D, S * 3 * D, o.data_ptr(), D, S * D,
                      None, B, 1, S, S, D, D ** -0.5).run()
    _sync(dev)
    q, k, v = [t.cpu() for t in qkv.chunk(3, -1)]
    assert rel_err(o.cpu(), _attn_ref(q, k, v, D ** -0.5)) < TOLBF


def test_attention_bwd_rejects_wide_head(dev):
    D, S = 512, 64
    t = [torch.zeros(1, S, D, dtype=bf, device=dev) for _ in range(8)]
    lse = torch.zeros(1, 1, S, device=dev); delta = torch.zeros(1, 1, S, device=dev)
    a = [x.data_ptr() for x in t]
    with pytest.raises(hip.LecoError, match="unsupported head_dim"):
        ops.attention_bwd(a[0], D, S * D, a[1], D, S * D, a[2], D, S * D, a[3], D, S * D, a[4], D, S * D, lse, delta,
                          a[5], D, S * D, a[6], D, S * D, a[7], D, S * D, 1, 1, S, S, D, D ** -0.5).run()


# ---- RGB output convolution + pixel epilogue ---------------------------------------------------------------------------------
def _quantise(y):
    """The rule of the epilogue on a fp32 NCHW image, as (B, H, W, 3) integers."""
    return torch.floor((y / 2 + 0.5).clamp(0, 1) * 255 + 0.5).permute(0, 2, 3, 1)


@pytest.mark.parametrize("B,h,w,c", [(2, 8, 8, 64), (1, 24, 40, 128)])
def test_conv_out_rgb(dev, B, h, w, c):
    torch.manual_seed(64)
    x = torch.randn(B, c, h, w).to(bf)
    wt = (torch.randn(3, c, 3, 3) / (9 * c) ** 0.5).to(bf); bias = torch.randn(3) * 0.1
    xcl = x.permute(0, 2, 3, 1).reshape(B * h * w, c).contiguous().to(dev)
    wcl = wt.permute(0, 2, 3, 1).contiguous().to(dev)
    y = torch.zeros(B, 3, h, w, device=dev); img = torch.zeros(B, h, w, 3, dtype=torch.uint8, device=dev)
    ops.conv_out_rgb(xcl, wcl, bias.to(dev), y, img, B, h, w, c).run()
    _sync(dev)
    ref = F.conv2d(x.float(), wt.float(), bias, padding=1)
    assert rel_err(y.cpu(), ref) < TOLBF
    # the uint8 image is the quantised fp32 output of the same call (1 level: a value on a rounding boundary)
    assert (img.cpu().float() - _quantise(y.cpu())).abs().max().item() <= 1
    # each output alone gives the same values
    y2 = torch.zeros_like(y); img2 = torch.zeros_like(img)
    ops.conv_out_rgb(xcl, wcl, bias.to(dev), y2, None, B, h, w, c).run()
    ops.conv_out_rgb(xcl, wcl, bias.to(dev), None, img2, B, h, w, c).run()
    _sync(dev)
    assert torch.equal(y2, y) and torch.equal(img2, img)
    with pytest.raises(hip.LecoError):
        ops.conv_out_rgb(xcl, wcl, bias.to(dev), None, None, B, h, w, c).run()


def test_conv_out_rgb_uint8_rule_is_exact(dev):
    """Pre-images y = (k + 0.25) / 127.5 - 1 sit a quarter level above the boundary of level k: the exact result is k, and
    0 / 255 for -3 / 3.  y is fed through a centre-tap weight of ones on three channels that carry y split into three bf16
    pieces (hi + mid + lo: 24 mantissa bits, summed in the fp32 accumulator), so the epilogue sees y to fp32 precision."""
    k = torch.arange(255, dtype=torch.float64)
    yv = torch.cat([(k + 0.25) / 127.5 - 1, torch.tensor([-3.0, 3.0], dtype=torch.float64)]).float()
    expect = torch.cat([k, torch.tensor([0.0, 255.0], dtype=torch.float64)]).to(torch.uint8)
    h, w, c = 16, 17, 32
    n = yv.numel()
    assert n <= h * w
    hi = yv.to(bf); mid = (yv - hi.float()).to(bf); lo = (yv - hi.float() - mid.float()).to(bf)
    assert (hi.float() + mid.float() + lo.float() - yv).abs().max().item() < 1e-6
    x = torch.zeros(h * w, c, dtype=bf)
    x[:n, 0], x[:n, 1], x[:n, 2] = hi, mid, lo
    wt = torch.zeros(3, 3, 3, c, dtype=bf)
    wt[:, 1, 1, 0:3] = 1.0
    y = torch.zeros(1, 3, h, w, device=dev); img = torch.zeros(1, h, w, 3, dtype=torch.uint8, device=dev)
    ops.conv_out_rgb(x.to(dev), wt.to(dev), torch.zeros(3, device=dev), y, img, 1, h, w, c).run()
    _sync(dev)
    assert (y.cpu().reshape(3, -1)[:, :n] - yv).abs().max().item() < 1e-6
    got = img.cpu().reshape(h * w, 3)[:n]
    for ch in range(3):
        assert torch.equal(got[:, ch], expect), (got[:, ch].int() - expect.int()).abs().max()


def test_conv_out_keeps_its_four_output_contract(dev):
    x = torch.zeros(64, 64, dtype=bf, device=dev); wt = torch.zeros(3, 3, 3, 64, dtype=bf, device=dev)
    with pytest.raises(hip.LecoError, match="Cout=4"):
        ops.conv_out(x, wt, torch.zeros(3, device=dev), torch.zeros(1, 3, 8, 8, device=dev), 1, 8, 8, 64, 3).run()


# ---- the largest launches of a 1024^2 decode ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conftest import _bind_hip
    _bind_hip()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(65)
    x = (torch.randn(128, 1024 * 1024 // 64, generator=g).repeat(1, 64)
         + torch.linspace(-1, 1, 1024 * 1024)[None, :]).to(bf)          # (C, hw): not periodic, cheap to draw
    return dev, x.t().contiguous().to(dev)                               # channels-last [hw][128]


@pytest.mark.gpu
def test_conv3x3_128_at_1024_squared(big):
    dev, x = big
    H = W = 1024
    C = 128
    torch.manual_seed(66)
    wt = (torch.randn(C, C, 3, 3) / (9 * C) ** 0.5).to(bf).to(dev); bias = (torch.randn(C) * 0.1).to(dev)
    wm = wt.permute(0, 2, 3, 1).reshape(C, 9 * C).contiguous()
    out = torch.zeros(H * W, C, dtype=bf, device=dev)
    g = hip.gemm_args(x, wm, out, m=H * W, n=C, k=9 * C, lda=C, a_mode=hip.A_CONV3_S1, conv=(1, H, W, H, W), bias=bias)
    ops.gemm(g).run()
    torch.cuda.synchronize()
    ref = F.conv2d(x.float().t().reshape(1, C, H, W), wt.float(), bias, padding=1)
    e = rel_err(out.float().t().reshape(1, C, H, W), ref)
    print(f"conv3x3 128->128 at 1024^2: rel {e:.3e}")
    assert e < TOLBF


@pytest.mark.gpu
def test_groupnorm_silu_128_at_1024_squared(big):
    dev, x = big
    HW, C, G = 1024 * 1024, 128, 32
    torch.manual_seed(67)
    gamma = torch.randn(C).to(dev); beta = torch.randn(C).to(dev)
    stats = torch.zeros(G * 2 * 257, device=dev); y = torch.zeros(HW, C, dtype=bf, device=dev)
    ops.groupnorm_fwd(x, C, None, 0, C, gamma, beta, 1, HW, C, G, 1e-6, hip.ACT_SILU, stats, y, C).run()
    torch.cuda.synchronize()
    ref = F.silu(F.group_norm(x.float().t().reshape(1, C, HW), G, gamma, beta, 1e-6))
    e = rel_err(y.float().t().reshape(1, C, HW), ref)
    print(f"GroupNorm+SiLU C=128 G=32 at hw=1024^2: rel {e:.3e}")
    assert e < TOLBF
