"""Kernels the VAE encoder adds: the bottom / right padded stride-2 gather of the implicit-GEMM convolution
(LECO_A_CONV3_S2_PAD01), the 3-channel image entry convolution (leco_conv_in_rgb) and the moments -> latents exit
(leco_conv_out_moments) -- each against fp32 PyTorch, on the host emulator of the kernel sources and (marked `gpu`) on
gfx950.  Bounds are the project's (tests/test_kernels.py)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from leco_amd import hip, ops

bf = torch.bfloat16
TOL32 = 1e-5          # fp32 outputs
TOLBF = 3e-3          # bf16 outputs


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


# ---- LECO_A_CONV3_S2_PAD01 ---------------------------------------------------------------------------------------------------------
def _conv_operands(B, H, W, Ci, Co, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci, H, W, generator=g).to(bf)
    wt = (torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5).to(bf)
    bias = torch.randn(Co, generator=g) * 0.1
    return x, wt, bias


def _run_conv(dev, amode, x, wt, bias, ho, wo):
    B, Ci, H, W = x.shape
    Co = wt.shape[0]
    xh = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wh = wt.permute(0, 2, 3, 1).contiguous().reshape(Co, 9 * Ci).to(dev)
    out = torch.zeros(B * ho * wo, Co, dtype=bf, device=dev)
    g = hip.gemm_args(xh, wh, out, m=B * ho * wo, n=Co, k=9 * Ci, lda=Ci, a_mode=amode, conv=(B, ho, wo, H, W), bias=bias.to(dev))
    hip.gemm(g, ops.default_stream())
    _sync(dev)
    return out.float().reshape(B, ho, wo, Co).permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("B,H,W,Ci,Co", [(2, 12, 12, 64, 128), (1, 8, 20, 128, 128)])
def test_conv3x3_s2_pad01(dev, B, H, W, Ci, Co):
    """M = 72 rows (a ragged tile that spans both images) and a non-square image.  On the same operands the symmetric pad-1
    stride-2 gather gives other numbers, and still its own."""
    x, wt, bias = _conv_operands(B, H, W, Ci, Co, 80)
    got = _run_conv(dev, hip.A_CONV3_S2_PAD01, x, wt, bias, H // 2, W // 2)
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), wt.float(), bias, stride=2)
    e = rel_err(got, ref)
    sym = _run_conv(dev, hip.A_CONV3_S2, x, wt, bias, H // 2, W // 2)
    e_sym = rel_err(sym, F.conv2d(x.float(), wt.float(), bias, stride=2, padding=1))
    print(f"conv3 s2 pad01 {B}x{H}x{W} {Ci}->{Co}: rel {e:.3e}; pad-1 form rel {e_sym:.3e}; distance {rel_err(got, sym):.3e}")
    assert got.shape == ref.shape
    assert e < TOLBF
    assert e_sym < TOLBF
    assert rel_err(got, sym) > 0.1


def test_conv3x3_s2_pad01_with_silu_residual_and_split_k(dev):
    """What the implicit-GEMM convolution carries works in the new mode: SiLU, a residual operand, a K split."""
    B, H, W, Ci, Co = 1, 8, 8, 128, 64
    x, wt, bias = _conv_operands(B, H, W, Ci, Co, 81)
    res = torch.randn(B * 16, Co, generator=torch.Generator().manual_seed(82)).to(bf)
    xh = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wh = wt.permute(0, 2, 3, 1).contiguous().reshape(Co, 9 * Ci).to(dev)
    out = torch.zeros(B * 16, Co, dtype=bf, device=dev)
    ws = torch.zeros(4 * 16 * Co, device=dev)
    g = hip.gemm_args(xh, wh, out, m=16, n=Co, k=9 * Ci, lda=Ci, a_mode=hip.A_CONV3_S2_PAD01, conv=(B, 4, 4, H, W),
                      bias=bias.to(dev), residual=res.to(dev), act=hip.ACT_SILU)
    hip.gemm(g, ops.default_stream(), tile=3, split_k=3, ws=ws)
    _sync(dev)
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), wt.float(), bias, stride=2)
    ref = F.silu(ref + res.float().reshape(B, 4, 4, Co).permute(0, 3, 1, 2))
    assert rel_err(out.float().reshape(B, 4, 4, Co).permute(0, 3, 1, 2).cpu(), ref) < TOLBF


@pytest.mark.parametrize("tile,split", [(-1, 1), (3, 2)])
def test_conv3x3_s2_pad01_column_statistics(dev, tile, split):
    """leco_gemm_args.col_stats in the new mode: {sum, sumsq} per (sample, atom of 4 columns) of the bf16 values stored, with
    36 rows per sample (a tile spans both samples), from the epilogue and from the split-K finish."""
    B, H, W, Ci, Co, atom = 2, 12, 12, 64, 128, 4
    hw = (H // 2) * (W // 2)
    x, wt, bias = _conv_operands(B, H, W, Ci, Co, 87)
    xh = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wh = wt.permute(0, 2, 3, 1).contiguous().reshape(Co, 9 * Ci).to(dev)
    out = torch.zeros(B * hw, Co, dtype=bf, device=dev)
    cs = torch.zeros(B, Co // atom, 2, device=dev)
    ws = torch.zeros(4 * B * hw * Co, device=dev)
    g = hip.gemm_args(xh, wh, out, m=B * hw, n=Co, k=9 * Ci, lda=Ci, a_mode=hip.A_CONV3_S2_PAD01, conv=(B, H // 2, W // 2, H, W),
                      bias=bias.to(dev), act=hip.ACT_SILU, col_stats=cs, stats_rows=hw, stats_atom=atom)
    hip.gemm(g, ops.default_stream(), tile=tile, split_k=split, ws=ws)
    _sync(dev)
    ref = F.silu(F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), wt.float(), bias, stride=2))
    assert rel_err(out.float().reshape(B, H // 2, W // 2, Co).permute(0, 3, 1, 2).cpu(), ref) < TOLBF
    y = out.float().cpu().reshape(B, hw, Co // atom, atom)
    assert rel_err(cs.cpu(), torch.stack([y.sum((1, 3)), (y * y).sum((1, 3))], dim=-1)) < TOL32


def test_conv3x3_s2_pad01_rejects_bad_geometry(dev):
    xa, wa, out = (torch.zeros(r, c, dtype=bf, device=dev) for r, c in ((64, 64), (64, 576), (32, 64)))     # live for every call

    def args(h_in, w_in, h_out, w_out):
        return hip.gemm_args(xa, wa, out, m=h_out * w_out, n=64, k=576, lda=64, a_mode=hip.A_CONV3_S2_PAD01,
                             conv=(1, h_out, w_out, h_in, w_in))
    for geo in [(7, 8, 3, 4), (8, 7, 4, 3), (8, 8, 3, 4), (8, 8, 4, 5)]:         # odd h_in / w_in; h_out / w_out != half
        with pytest.raises(hip.LecoError, match="LECO_A_CONV3_S2_PAD01"):
            hip.gemm(args(*geo), ops.default_stream())
    hip.gemm(args(8, 8, 4, 4), ops.default_stream())                             # the well-formed one is accepted
    _sync(dev)
    # the fp32 GEMM, the patch-staged convolution and the LoRA weight gradient refuse the mode by name
    f32 = ops._fn("leco_f32_gemm")
    g = args(8, 8, 4, 4)
    rc = f32(C.byref(g), ops.default_stream())
    assert rc == -22 and b"LECO_A_CONV3_S2_PAD01" in hip.lib().leco_last_error()
    with pytest.raises(hip.LecoError, match="LECO_A_CONV3_S2_PAD01"):
        hip.gemm(args(8, 8, 4, 4), ops.default_stream(), tile=9)
    wg = ops._fn("leco_lora_wgrad_conv")
    t = torch.zeros(64, 64, device=dev)
    rc = wg(t.data_ptr(), 4, t.data_ptr(), 64, t.data_ptr(), 64, 1, 16, 4, 64, 1.0, hip.A_CONV3_S2_PAD01, 4, 4, 8, 8, 0, 0,
            None, 0, ops.default_stream())
    assert rc == -22 and b"LECO_A_CONV3_S2_PAD01" in hip.lib().leco_last_error()


# ---- leco_conv_in_rgb ------------------------------------------------------------------------------------------------------------
def _ulp_bf16(t):
    """One bf16 unit in the last place at the magnitude of each element."""
    return torch.pow(2.0, torch.floor(torch.log2(t.abs().clamp_min(1e-30))) - 7)


@pytest.mark.parametrize("B,h,w,cout", [(2, 24, 40, 128), (1, 8, 8, 64)])
def test_conv_in_rgb(dev, B, h, w, cout):
    """Both image inputs against fp32 F.conv2d; the two descriptions of one image agree bit for bit (stricter than
    one bf16 ulp: identity is what the kernel promises and the plans rely on)."""
    g = torch.Generator().manual_seed(83)
    img = torch.randint(0, 256, (B, h, w, 3), generator=g, dtype=torch.uint8)
    x = (img.float() / 127.5 - 1).permute(0, 3, 1, 2).contiguous()
    wt = (torch.rand(cout, 3, 3, 3, generator=g) * 2 - 1) / 27 ** 0.5
    bias = (torch.rand(cout, generator=g) * 2 - 1) * 0.1
    ref = F.conv2d(x, wt, bias, padding=1)
    outs = []
    for kind in ("fp32", "uint8"):
        y = torch.zeros(B * h * w, cout, dtype=bf, device=dev)
        ops.conv_in_rgb(x.to(dev) if kind == "fp32" else None, img.to(dev) if kind == "uint8" else None, wt.to(dev),
                        bias.to(dev), y, B, h, w, cout).run()
        _sync(dev)
        got = y.float().reshape(B, h, w, cout).permute(0, 3, 1, 2).cpu()
        e = rel_err(got, ref)
        print(f"conv_in_rgb {kind} {B}x{h}x{w} -> {cout}: rel {e:.3e}")
        assert e < TOLBF
        outs.append(got)
    # the 8-bit pixel p is looked up as the split of the fp32 number p / 127.5 - 1, the one the fp32 input carries: the same bits
    assert torch.equal(outs[0], outs[1])
    # a second fp32 image that is NOT on the 8-bit grid (the hi + lo split of the fp32 input carries it)
    x2 = torch.rand(B, 3, h, w, generator=g) * 2 - 1
    y = torch.zeros(B * h * w, cout, dtype=bf, device=dev)
    ops.conv_in_rgb(x2.to(dev), None, wt.to(dev), bias.to(dev), y, B, h, w, cout).run()
    _sync(dev)
    ref2 = F.conv2d(x2, wt, bias, padding=1)
    got2 = y.float().reshape(B, h, w, cout).permute(0, 3, 1, 2).cpu()
    assert rel_err(got2, ref2) < TOLBF
    # ... to the rounding of the output alone: the fp32 result rounded to bf16, give or take one ulp on a rounding boundary.
    # Where the 27 terms cancel to (almost) nothing, kernel and reference differ by the rounding of their own fp32 sums,
    # which is bounded by the fp32 bound on the magnitude of what is summed: TOL32 * (sum |w| * max |x| + |bias|), |x| <= 1
    mag = (wt.abs().sum((1, 2, 3)) + bias.abs())[None, :, None, None]
    assert ((got2 - ref2.to(bf).float()).abs() <= _ulp_bf16(ref2) + TOL32 * mag).all()


def test_conv_in_rgb_border_is_exact(dev):
    """A white image (p = 255 -> +1), weights 1 / 8, no bias: every output is (taps inside the image) / 8, exact in bf16, so
    padding contributes exactly zero in the normalised space.  With the weights on one input channel the values are 4/8
    (corner), 6/8 (edge) and 9/8; with all 27 weights at 1/8 the three channels add up to 12/8, 18/8 and 27/8."""
    B, h, w, cout = 1, 8, 12, 32
    img = torch.full((B, h, w, 3), 255, dtype=torch.uint8)
    count = F.conv2d(torch.ones(1, 1, h, w), torch.ones(1, 1, 3, 3), padding=1)[0, 0]
    assert sorted(set(count.flatten().tolist())) == [4.0, 6.0, 9.0]
    one = torch.zeros(cout, 3, 3, 3); one[:, 1] = 1 / 8
    for wt, nch in ((one, 1), (torch.full((cout, 3, 3, 3), 1 / 8), 3)):
        expect = (nch * count / 8)[:, :, None].expand(h, w, cout)
        for kind in ("uint8", "fp32"):
            y = torch.zeros(h * w, cout, dtype=bf, device=dev)
            ops.conv_in_rgb(torch.ones(B, 3, h, w, device=dev) if kind == "fp32" else None,
                            img.to(dev) if kind == "uint8" else None, wt.to(dev), torch.zeros(cout, device=dev), y, B, h, w,
                            cout).run()
            _sync(dev)
            assert torch.equal(y.float().reshape(h, w, cout).cpu(), expect), (kind, nch)


def test_conv_in_rgb_rejects_bad_arguments(dev):
    x = torch.zeros(1, 3, 8, 8, device=dev); img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=dev)
    wt = torch.zeros(64, 27, device=dev); b = torch.zeros(64, device=dev); y = torch.zeros(64, 64, dtype=bf, device=dev)
    with pytest.raises(hip.LecoError, match="neither"):
        ops.conv_in_rgb(None, None, wt, b, y, 1, 8, 8, 64).run()
    with pytest.raises(hip.LecoError, match="both"):
        ops.conv_in_rgb(x, img, wt, b, y, 1, 8, 8, 64).run()
    with pytest.raises(hip.LecoError, match="32"):
        ops.conv_in_rgb(x, None, wt, b, y, 1, 8, 8, 48).run()


# ---- leco_conv_out_moments -----------------------------------------------------------------------------------------------------
def _moments_operands(B, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, c, h, w, generator=g).to(bf)
    wt = (torch.randn(8, c, 3, 3, generator=g) / (9 * c) ** 0.5).to(bf)
    bias = torch.randn(8, generator=g) * 0.1
    qw = torch.randn(8, 8, generator=g) / 8 ** 0.5
    qb = torch.randn(8, generator=g) * 0.1
    noise = torch.randn(B, 4, h, w, generator=g)
    return x, wt, bias, qw, qb, noise


def _run_moments(dev, x, wt, bias, qw, qb, noise, scale, want_moments=True, want_latents=True):
    B, c, h, w = x.shape
    xcl = x.permute(0, 2, 3, 1).reshape(B * h * w, c).contiguous().to(dev)
    wcl = wt.permute(0, 2, 3, 1).contiguous().to(dev)
    mom = torch.zeros(B, 8, h, w, device=dev) if want_moments else None
    lat = torch.zeros(B, 4, h, w, device=dev) if want_latents else None
    ops.conv_out_moments(xcl, wcl, bias.to(dev), qw.to(dev), qb.to(dev), None if noise is None else noise.to(dev), mom, lat, scale,
                         B, h, w, c).run()
    _sync(dev)
    return (None if mom is None else mom.cpu()), (None if lat is None else lat.cpu())


@pytest.mark.parametrize("B,h,w,c", [(2, 6, 10, 128), (1, 4, 4, 512)])
def test_conv_out_moments(dev, B, h, w, c):
    x, wt, bias, qw, qb, noise = _moments_operands(B, h, w, c, 84)
    scale = 0.18215
    mom, lat = _run_moments(dev, x, wt, bias, qw, qb, noise, scale)
    ref = F.conv2d(F.conv2d(x.float(), wt.float(), bias, padding=1), qw.reshape(8, 8, 1, 1), qb)
    e = rel_err(mom, ref)
    mean, logvar = mom.chunk(2, 1)
    e_lat = rel_err(lat, scale * (mean + torch.exp(0.5 * logvar.clamp(-30, 20)) * noise))
    print(f"conv_out_moments {B}x{h}x{w} C={c}: moments rel {e:.3e}  latents rel {e_lat:.3e}")
    assert e < TOL32
    assert e_lat < TOL32
    # noise = NULL: the mode
    mom0, lat0 = _run_moments(dev, x, wt, bias, qw, qb, None, scale)
    assert torch.equal(mom0, mom) and torch.equal(lat0, scale * mean)
    # each output alone agrees bitwise with both in one launch
    mom1, none = _run_moments(dev, x, wt, bias, qw, qb, noise, scale, want_latents=False)
    none2, lat1 = _run_moments(dev, x, wt, bias, qw, qb, noise, scale, want_moments=False)
    assert none is None and none2 is None
    assert torch.equal(mom1, mom) and torch.equal(lat1, lat)


@pytest.mark.parametrize("shift,std", [(50.0, math.exp(10.0)), (-50.0, math.exp(-15.0))])
def test_conv_out_moments_clamps_logvar(dev, shift, std):
    """A quant_conv bias that drives logvar to +-50: std = exp(0.5 * clamp(logvar, -30, 20)) = e^10 resp. e^-15."""
    B, h, w, c = 1, 4, 4, 32
    x, wt, bias, qw, qb, _ = _moments_operands(B, h, w, c, 85)
    qw = qw * 0.01                               # |logvar - shift| << 20
    qb = qb.clone(); qb[4:] = shift
    noise = torch.ones(B, 4, h, w)
    mom, lat = _run_moments(dev, x, wt, bias, qw, qb, noise, 1.0)
    mean, logvar = mom.chunk(2, 1)
    assert (logvar - shift).abs().max().item() < 5
    got_std = lat - mean                          # scale = 1, noise = 1
    if shift > 0:
        assert rel_err(got_std, torch.full_like(got_std, std)) < TOL32
    else:                                         # e^-15 sits below the fp32 spacing of the mean: compare through another noise level
        _, lat_big = _run_moments(dev, x, wt, bias, qw, qb, noise * 2.0 ** 40, 1.0)
        assert rel_err(lat_big - mean, torch.full_like(mean, std * 2.0 ** 40)) < TOL32


def test_conv_out_moments_rejects_bad_arguments(dev):
    x, wt, bias, qw, qb, noise = _moments_operands(1, 4, 4, 32, 86)
    with pytest.raises(hip.LecoError, match="neither"):
        _run_moments(dev, x, wt, bias, qw, qb, noise, 1.0, want_moments=False, want_latents=False)
    xcl = torch.zeros(16, 48, dtype=bf, device=dev)
    with pytest.raises(hip.LecoError, match="32"):
        ops.conv_out_moments(xcl, torch.zeros(8, 9 * 48, dtype=bf, device=dev), bias.to(dev), qw.to(dev), qb.to(dev), None,
                             torch.zeros(1, 8, 4, 4, device=dev), None, 1.0, 1, 4, 4, 48).run()
