"""`leco_image_compare` (csrc/image_metrics.hip) against a float64 torch statement of SSIM (Wang et al. 2004: per channel, the
11 x 11 window = outer product of the FLOAT64 Gaussian taps, biased moments, F.conv2d without padding, mean over the channels)
and an int64 statement of the squared error.  Runs on the host emulator (CPU tier) and on gfx950 (`-m gpu`).

Bound on a per-pixel SSIM value and on the mean SSIM: 5e-4 absolute.  The kernel forms the moments of the centred levels
x' = x - 128 (|x'| <= 128) and the SSIM formula in fp64; products and pair sums of levels are exact integers, so fp64 rounding
(2^-53 per operation, ~40 operations) is below 1e-11 and the error that is left comes from the taps, which the kernel gets
rounded to fp32: w32 = w64 (1 + e), |e| <= u = 2^-24, so a 2-D weight errs by 2u relative and, all weights being positive,
  |d mu'| <= 2u * 128 = 1.53e-5,   |d E[x' y']| <= 2u * 16384 = 1.95e-3,   |d (mu_a' mu_r')| <= 2 * 128 * 1.53e-5 = 3.9e-3,
so a (co)variance s = E[x' y'] - mu_a' mu_r' errs by at most 5.9e-3 and each of B1 = s_aa + s_rr + C2, B2 = 2 s_ar + C2 by
1.17e-2, which is 2.0e-4 of B1 >= C2 = 58.52.  The luminance factors A = 2 mu_a mu_r + C1 (mu = mu' + 128 in [0, 255]) err by
4 mu |d mu| / (2 mu^2 + C1) <= 8.5e-6 relative (the maximum is at mu^2 = C1 / 2).  With |A2 / A1| <= 1 and |B2 / B1| <= 1,
  |d ssim| <= eA1 + eA2 + eB1 + |d B2| / B1 <= 2 * 8.5e-6 + 2 * 2.0e-4 = 4.2e-4
to first order; the one rounding of the change map to fp32 adds 2^-24 * 2.  5e-4 leaves room for the second-order terms.
Measured: DESIGN.md, "Image metrics"."""
import pytest
import torch
import torch.nn.functional as F

from leco_amd import hip, image_metrics, ops

NAN = float("nan")
GUARD = 64                     # bytes of arbitrary levels around the pictures, NaN elements around the outputs
BOUND = 5e-4
TILE_W, TILE_H = 32, 16        # csrc/image_metrics.hip: IC_TW, IC_TH
#         batch, h, w
SHAPES = [(1, 11, 11), (2, 11, 40), (2, 40, 11), (3, 37, 53), (2, TILE_H + 1 + 10, TILE_W + 1 + 10), (2, 128, 128)]
KINDS = ["uniform", "gradient", "constant_self", "black_white", "patch"]
PATCH = (14, 17, 8)            # y, x, size of the replaced patch (shapes that hold it)


def _pictures(kind, batch, h, w, pairwise, seed=0):
    """(a uint8 [batch][h][w][3], ref uint8 [batch or 1][h][w][3])"""
    g = torch.Generator().manual_seed(seed + 7 * h + w)
    nref = batch if pairwise else 1

    def rnd(n):
        return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    if kind == "uniform":
        return rnd(batch), rnd(nref)
    if kind == "gradient":
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        ramp = (200.0 * (yy + xx) / max(h + w - 2, 1))[None, :, :, None]
        a = (ramp + torch.randint(0, 40, (batch, h, w, 3), generator=g)).clamp(0, 255).to(torch.uint8)
        r = (ramp + torch.randint(0, 40, (nref, h, w, 3), generator=g)).clamp(0, 255).to(torch.uint8)
        return a, r
    if kind == "constant_self":
        return torch.full((batch, h, w, 3), 77, dtype=torch.uint8), torch.full((nref, h, w, 3), 77, dtype=torch.uint8)
    if kind == "black_white":
        return torch.zeros((batch, h, w, 3), dtype=torch.uint8), torch.full((nref, h, w, 3), 255, dtype=torch.uint8)
    assert kind == "patch"
    r = rnd(1).repeat(nref, 1, 1, 1)
    a = r[:1].repeat(batch, 1, 1, 1).clone()
    y, x, s = PATCH
    if h >= y + s and w >= x + s:
        a[:, y:y + s, x:x + s] = 255 - a[:, y:y + s, x:x + s]
    else:                       # a picture too small for the patch: one pixel in the middle
        a[:, h // 2, w // 2] = 255 - a[:, h // 2, w // 2]
    return a, r


_oracle_cache = {}


def _oracle(key, a, ref):
    """float64: (ssim map [B][h - 10][w - 10], mean ssim [B], sse int64 [B]); computed once per case and shared."""
    if key not in _oracle_cache:
        taps = image_metrics.gaussian_taps()
        assert taps.dtype == torch.float64 and abs(taps.sum().item() - 1.0) < 1e-15
        win = torch.outer(taps, taps)[None, None]
        B = a.shape[0]
        x = a.double().permute(0, 3, 1, 2).reshape(B * 3, 1, *a.shape[1:3])
        y = ref.expand_as(a).double().permute(0, 3, 1, 2).reshape(B * 3, 1, *a.shape[1:3])
        mx, my = F.conv2d(x, win), F.conv2d(y, win)
        sxx, syy, sxy = F.conv2d(x * x, win) - mx * mx, F.conv2d(y * y, win) - my * my, F.conv2d(x * y, win) - mx * my
        c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
        s = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
        s = s.reshape(B, 3, *s.shape[2:]).mean(1)
        d = a.to(torch.int64) - ref.expand_as(a).to(torch.int64)
        _oracle_cache[key] = (s, s.mean(dim=(1, 2)), (d * d).sum(dim=(1, 2, 3)))
    return _oracle_cache[key]


class Launch:
    """Operands of one launch: both pictures between GUARD bytes of arbitrary levels (``guard_seed``), the change map and the
    stats between NaN guards."""

    def __init__(self, dev, a, ref, guard_seed=1, change=True):
        self.B, self.h, self.w = a.shape[:3]
        self.pairwise = ref.shape[0] == self.B and self.B > 1
        g = torch.Generator().manual_seed(guard_seed)

        def guarded(t):
            n = t.numel()
            buf = torch.randint(0, 256, (n + 2 * GUARD,), generator=g, dtype=torch.uint8)
            buf[GUARD:GUARD + n] = t.reshape(-1)
            return buf.to(dev)
        self.abuf, self.rbuf = guarded(a), guarded(ref)
        self.taps = image_metrics.gaussian_taps().float().to(dev)
        self.nmap = self.B * self.h * self.w
        self.cbuf = torch.full((self.nmap + 2 * GUARD,), NAN, dtype=torch.float32).to(dev) if change else None
        self.sbuf = torch.full((2 * self.B + 2 * GUARD,), NAN, dtype=torch.float64).to(dev)
        self.ws = torch.zeros(max(ops.image_compare_workspace(self.B, self.h, self.w) // 8, 1), dtype=torch.float64).to(dev)

    def op(self, batch=None, h=None, w=None, ref_stride=None, ws_bytes=None):
        B, hh, ww = self.B if batch is None else batch, self.h if h is None else h, self.w if w is None else w
        stride = (self.h * self.w * 3 if self.pairwise else 0) if ref_stride is None else ref_stride
        return ops.image_compare(self.abuf.data_ptr() + GUARD, self.rbuf.data_ptr() + GUARD, stride, B, hh, ww, self.taps,
                                 None if self.cbuf is None else self.cbuf.data_ptr() + 4 * GUARD, self.sbuf.data_ptr() + 8 * GUARD,
                                 self.ws, ws_bytes, keep=(self.abuf, self.rbuf, self.cbuf, self.sbuf))

    def change(self):
        return self.cbuf[GUARD:GUARD + self.nmap].cpu().clone().reshape(self.B, self.h, self.w)

    def stats(self):
        return self.sbuf[GUARD:GUARD + 2 * self.B].cpu().clone().reshape(self.B, 2)

    def guards_intact(self):
        s = self.sbuf.cpu()
        ok = bool(torch.isnan(s[:GUARD]).all() and torch.isnan(s[GUARD + 2 * self.B:]).all())
        if self.cbuf is not None:
            c = self.cbuf.cpu()
            ok = ok and bool(torch.isnan(c[:GUARD]).all() and torch.isnan(c[GUARD + self.nmap:]).all())
        return ok


def test_tile_straddle_shape_is_one_tile_plus_one():
    """The fifth shape: a valid region of exactly one tile plus one row and one column."""
    _, h, w = SHAPES[4]
    assert (h - 10, w - 10) == (TILE_H + 1, TILE_W + 1)


@pytest.mark.parametrize("pairwise", [False, True], ids=["one_baseline", "pairwise"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=["b%d-%dx%d" % s for s in SHAPES])
def test_ssim_and_sse_match_float64(dev, shape, kind, pairwise):
    batch, h, w = shape
    a, ref = _pictures(kind, batch, h, w, pairwise)
    ssim, mean, sse = _oracle((shape, kind, pairwise), a, ref)
    run = Launch(dev, a, ref)
    run.op().run()
    st, ch = run.stats(), run.change()
    assert run.guards_intact()
    assert torch.isfinite(st).all() and torch.isfinite(ch).all()
    e_px = (1.0 - ch[:, 5:h - 5, 5:w - 5].double() - ssim).abs().max().item()
    e_mean = (st[:, 0] - mean).abs().max().item()
    print(f"image_compare {shape} {kind} {'pairwise' if pairwise else 'one baseline'} [{dev.type}]: per-pixel ssim err {e_px:.3g}, "
          f"mean ssim err {e_mean:.3g}, ssim {mean.min().item():.4f}..{mean.max().item():.4f}")
    assert e_px <= BOUND, e_px
    assert e_mean <= BOUND, e_mean
    assert torch.equal(st[:, 1], sse.double()), (st[:, 1], sse)                      # an integer, exactly
    border = ch.clone()
    border[:, 5:h - 5, 5:w - 5] = 0.0
    assert torch.equal(border, torch.zeros_like(border))                             # the 5-pixel border is 0, exactly
    if kind == "constant_self":
        assert torch.equal(st[:, 0], torch.ones(batch, dtype=torch.float64)) and torch.equal(ch, torch.zeros_like(ch))
        assert torch.equal(st[:, 1], torch.zeros(batch, dtype=torch.float64))
    if kind == "patch" and h >= PATCH[0] + PATCH[2] and w >= PATCH[1] + PATCH[2]:
        y, x, s = PATCH
        far = ch.clone()
        far[:, max(y - 5, 0):y + s + 5, max(x - 5, 0):x + s + 5] = 0.0
        assert torch.equal(far, torch.zeros_like(far))                               # further than 5 pixels from the patch: 0
        inside = ch[:, max(y, 5):min(y + s, h - 5), max(x, 5):min(x + s, w - 5)]
        assert inside.numel() > 0 and bool((inside > 0).all())

    # a second launch on the same input, and one with other guard bytes around the pictures: equal bits
    run.op().run()
    assert torch.equal(run.stats(), st) and torch.equal(run.change(), ch)
    other = Launch(dev, a, ref, guard_seed=2)
    assert not torch.equal(other.abuf[:GUARD].cpu(), run.abuf[:GUARD].cpu())
    other.op().run()
    assert torch.equal(other.stats(), st) and torch.equal(other.change(), ch) and other.guards_intact()


@pytest.mark.parametrize("pairwise", [False, True], ids=["one_baseline", "pairwise"])
def test_a_picture_against_itself_is_exactly_one(dev, pairwise):
    """Random levels: the three second moments are the same operations on the same integers."""
    batch, h, w = 3, 37, 53
    g = torch.Generator().manual_seed(9)
    one = torch.randint(0, 256, (1, h, w, 3), generator=g, dtype=torch.uint8)
    a = one.repeat(batch, 1, 1, 1) if not pairwise else torch.randint(0, 256, (batch, h, w, 3), generator=g, dtype=torch.uint8)
    ref = one if not pairwise else a.clone()
    run = Launch(dev, a, ref)
    run.op().run()
    assert torch.equal(run.stats()[:, 0], torch.ones(batch, dtype=torch.float64))
    assert torch.equal(run.stats()[:, 1], torch.zeros(batch, dtype=torch.float64))
    assert torch.equal(run.change(), torch.zeros(batch, h, w)) and run.guards_intact()


def test_without_a_change_map_the_stats_are_the_same_bits(dev):
    a, ref = _pictures("gradient", 3, 37, 53, True)
    with_map, without = Launch(dev, a, ref), Launch(dev, a, ref, change=False)
    with_map.op().run()
    without.op().run()
    assert torch.equal(with_map.stats(), without.stats()) and without.guards_intact()


def test_sse_is_exact_past_2_to_the_24(dev):
    """0 against 255 on 128 x 128: 49152 * 65025 = 3,196,108,800 > 2^31."""
    a, ref = _pictures("black_white", 1, 128, 128, False)
    run = Launch(dev, a, ref)
    run.op().run()
    assert run.stats()[0, 1].item() == 128 * 128 * 3 * 255 * 255 > 2 ** 31


def test_window_agrees_with_scipy():
    """A second opinion on the window: scipy's Gaussian filter with the same radius."""
    ndimage = pytest.importorskip("scipy.ndimage")
    import numpy as np
    imp = np.zeros(21)
    imp[10] = 1.0
    ref = ndimage.gaussian_filter1d(imp, sigma=1.5, radius=5, mode="constant")[5:16]
    assert np.abs(ref - image_metrics.gaussian_taps().numpy()).max() < 1e-15


BAD = [dict(h=10), dict(w=10), dict(batch=0), dict(ref_stride=12), dict(ws_bytes=8)]


@pytest.mark.parametrize("bad", BAD, ids=["h10", "w10", "batch0", "ref_stride", "short_workspace"])
def test_bad_arguments_are_refused_and_nothing_is_written(dev, bad):
    a, ref = _pictures("uniform", 2, 37, 53, True)
    run = Launch(dev, a, ref)
    assert ops.image_compare_workspace(2, 37, 53) > 8
    before_c, before_s = run.cbuf.cpu().clone(), run.sbuf.cpu().clone()
    with pytest.raises(hip.LecoError) as ei:
        run.op(**bad).run()
    assert "image_compare" in str(ei.value) and "rc=-22" in str(ei.value)
    assert "%s=%d" % list(bad.items())[0] in str(ei.value).replace("workspace_bytes", "ws_bytes")
    assert torch.isnan(run.cbuf.cpu()).all() and torch.isnan(run.sbuf.cpu()).all()
    assert torch.equal(torch.isnan(before_c), torch.isnan(run.cbuf.cpu())) and torch.equal(torch.isnan(before_s), torch.isnan(run.sbuf.cpu()))
