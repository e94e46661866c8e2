"""The kernels of the cross-attention token heatmaps (csrc/attn_maps.hip) against torch statements of the same ops on the same
inputs: `leco_xattn_token_maps` (float64 softmax on the bf16 operands), `leco_attn_maps_merge` (F.interpolate) and
`leco_heat_overlay` (the formula of include/leco_hip.h).  Runs on the host emulator (CPU tier) and on gfx950 (`-m gpu`).

Token maps, bound: relative L2 <= 1e-4.  Products of bf16 pairs are exact in fp32; the fp32 accumulation over d <= 160 terms
errs by at most d 2^-24 ~ 1e-5 of sum |terms|; the inputs keep |scaled score| <= 10, so a probability errs by at most 1e-4
relative in the worst case.  Measured: see DESIGN.md, "Attention heatmaps"."""
import pytest
import torch
import torch.nn.functional as F

from leco_amd import hip, ops

bf = torch.bfloat16
NAN = float("nan")
GUARD = 3            # NaN rows in front of and behind every operand

#        head_dim, heads, sq, skv, batch, n_maps
SHAPES = [(40, 8, 256, 77, 2, 3), (64, 5, 72, 77, 2, 1), (80, 8, 16, 77, 1, 8), (160, 8, 64, 77, 2, 2), (64, 1, 1, 1, 1, 1),
          (40, 2, 33, 128, 2, 2)]
BOUND = 1e-4


class Case:
    """Operands of one launch: q with ld > C, k a column view of a [B * skv][2C] buffer, both between NaN guard rows (the rows
    directly behind the last key are NaN), the v half and q's spare columns NaN as well; maps preloaded, NaN guards around."""

    def __init__(self, dev, d, heads, sq, skv, batch, n_maps, peak=None, seed=0):
        g = torch.Generator().manual_seed(1000 * d + 10 * sq + skv + seed)
        self.dims = (d, heads, sq, skv, batch, n_maps)
        c = heads * d
        self.scale = d ** -0.5
        q = torch.randn(batch, sq, c, generator=g)
        k = torch.randn(batch, skv, c, generator=g)
        if peak is not None:      # scale q so that the largest |scaled score| is `peak`
            s = torch.einsum("bihd,bjhd->bhij", q.to(bf).double().reshape(batch, sq, heads, d),
                             k.to(bf).double().reshape(batch, skv, heads, d)) * self.scale
            q = q * (peak / s.abs().max().item())
        self.q, self.k = q.to(bf), k.to(bf)
        self.ldq, self.ldk = c + 8, 2 * c
        qbuf = torch.full((batch * sq + 2 * GUARD, self.ldq), NAN, dtype=bf)
        qbuf[GUARD:GUARD + batch * sq, :c] = self.q.reshape(batch * sq, c)
        kbuf = torch.full((batch * skv + 2 * GUARD, self.ldk), NAN, dtype=bf)
        kbuf[GUARD:GUARD + batch * skv, :c] = self.k.reshape(batch * skv, c)
        self.qbuf, self.kbuf = qbuf.to(dev), kbuf.to(dev)
        tw = torch.zeros(n_maps, skv)
        for m in range(n_maps):      # word m: 1 + m % 3 tokens (ones), the last map a fractional row as well
            for t in range(1 + m % 3):
                tw[m, (5 * m + 3 * t + 1) % skv] = 1.0
        if n_maps > 1:
            tw[-1] = torch.rand(skv, generator=g)
        self.tw = tw
        self.tw_dev = tw.to(dev)
        self.step = torch.ones(1, device=dev)
        n = batch * n_maps * sq
        self.preload = (0.01 * torch.sin(torch.arange(n, dtype=torch.float32))).reshape(batch, n_maps, sq)
        self.pad = 64
        mbuf = torch.full((n + 2 * self.pad,), NAN)
        mbuf[self.pad:self.pad + n] = self.preload.reshape(-1)
        self.mbuf = mbuf.to(dev)
        self.n = n

    def scores(self):
        d, heads, sq, skv, batch, _ = self.dims
        return torch.einsum("bihd,bjhd->bhij", self.q.double().reshape(batch, sq, heads, d),
                            self.k.double().reshape(batch, skv, heads, d)) * self.scale

    def delta(self):
        """float64: 1 / heads * sum_h sum_j tok_w[m][j] softmax_j(scores)[b][h][i][j] -> [b][m][i]"""
        p = torch.softmax(self.scores(), dim=-1)
        return torch.einsum("mj,bhij->bmi", self.tw.double(), p) / self.dims[1]

    def op(self, d=None, skv=None, n_maps=None):
        dd, heads, sq, kk, batch, mm = self.dims
        esz = 2
        return ops.xattn_token_maps(self.qbuf.data_ptr() + GUARD * self.ldq * esz, self.ldq, sq * self.ldq,
                                    self.kbuf.data_ptr() + GUARD * self.ldk * esz, self.ldk, kk * self.ldk, self.tw_dev,
                                    mm if n_maps is None else n_maps, self.step, self.mbuf.data_ptr() + 4 * self.pad, batch, heads, sq,
                                    kk if skv is None else skv, dd if d is None else d, self.scale,
                                    keep=(self.qbuf, self.kbuf, self.mbuf))

    def maps(self):
        return self.mbuf[self.pad:self.pad + self.n].cpu().clone().reshape(self.preload.shape)      # (a copy on the CPU tier too)

    def guards_intact(self):
        m = self.mbuf.cpu()
        return bool(torch.isnan(m[:self.pad]).all() and torch.isnan(m[self.pad + self.n:]).all())


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("shape", SHAPES, ids=["d%d-h%d-sq%d-skv%d-b%d-m%d" % s for s in SHAPES])
def test_token_maps_match_float64_softmax(dev, shape):
    c = Case(dev, *shape)
    assert c.scores().abs().max().item() <= 10.0          # the premise of the bound
    ref = c.delta()
    c.op().run()
    out1 = c.maps()
    assert c.guards_intact()
    assert torch.isfinite(out1).all()
    e1 = _rel(out1.double() - c.preload.double(), ref)
    c.step.fill_(0.25)                                     # read at launch: the same Op, another weight
    c.op().run()
    out2 = c.maps()
    e2 = _rel(out2.double() - out1.double(), 0.25 * ref)
    print(f"token maps {shape} [{dev.type}]: rel L2 {e1:.3g}, second call's share {e2:.3g}")
    assert c.guards_intact()
    assert e1 <= BOUND, e1
    # the share of the second call is the difference of two fp32 sums: their own rounding (2^-24 of |maps|) is added to the bound
    assert e2 <= BOUND + 2 ** -23 * out2.double().norm().item() / (0.25 * ref).norm().item(), e2
    # rows of the probabilities sum to one: with an all-ones token row the map is step_w (a sanity check of the reference)
    assert abs(torch.softmax(c.scores(), -1).sum(-1).mean().item() - 1.0) < 1e-12


def test_token_maps_peaked_scores_stay_finite_and_in_bound(dev):
    """Scores up to +-60: exp(60) is finite in fp32 but exp(60) * 77 terms next to exp(-60) is not a sum to form without the
    row maximum subtracted."""
    c = Case(dev, 64, 5, 72, 77, 2, 2, peak=60.0)
    assert 59.0 <= c.scores().abs().max().item() <= 61.0
    ref = c.delta()
    c.op().run()
    out = c.maps()
    e = _rel(out.double() - c.preload.double(), ref)
    print(f"token maps peaked [{dev.type}]: rel L2 {e:.3g}")
    assert torch.isfinite(out).all() and c.guards_intact()
    assert e <= BOUND, e


def test_token_maps_two_runs_are_bitwise_equal(dev):
    a, b = Case(dev, 40, 8, 256, 77, 2, 3), Case(dev, 40, 8, 256, 77, 2, 3)
    a.op().run()
    b.op().run()
    assert torch.equal(a.maps(), b.maps())


@pytest.mark.parametrize("bad", [dict(d=48), dict(skv=129), dict(n_maps=9)], ids=["d48", "skv129", "maps9"])
def test_token_maps_refuse_unsupported_shapes(dev, bad):
    c = Case(dev, 64, 2, 16, 77, 1, 2)
    before = c.mbuf.cpu().clone()
    with pytest.raises(hip.LecoError) as ei:
        c.op(**bad).run()
    assert "xattn_token_maps" in str(ei.value) and str(list(bad.values())[0]) in str(ei.value)
    after = c.mbuf.cpu()
    assert torch.equal(torch.isnan(before), torch.isnan(after)) and torch.equal(before.nan_to_num(0.0), after.nan_to_num(0.0))


# ---- leco_attn_maps_merge --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sources,size", [(((8, 8), (4, 4), (2, 2), (1, 1)), (64, 64)), (((8, 12), (4, 6)), (64, 96))],
                         ids=["square", "wide"])
def test_merge_matches_interpolate(dev, sources, size):
    g = torch.Generator().manual_seed(3)
    planes = 6                                             # 2 samples x 3 words
    maps = [torch.rand(planes, h, w, generator=g) for h, w in sources]
    weights = [0.4, 0.3, 0.2, 0.1][:len(sources)]
    ref = sum(wt * F.interpolate(m[None], size=size, mode="bilinear", align_corners=False)[0] for wt, m in zip(weights, maps))
    dmaps = [m.to(dev) for m in maps]
    table = ops.attn_map_layers([(m, h, w, wt) for m, (h, w), wt in zip(dmaps, sources, weights)], dev)
    pad = 64
    hbuf = torch.full((planes * size[0] * size[1] + 2 * pad,), NAN, device=dev)
    ops.attn_maps_merge(table, len(sources), hbuf.data_ptr() + 4 * pad, planes, size[0], size[1], keep=(dmaps, hbuf)).run()
    h = hbuf.cpu()
    out = h[pad:-pad].reshape(planes, *size)
    assert torch.isnan(h[:pad]).all() and torch.isnan(h[-pad:]).all()
    err = (out - ref).abs().max().item()
    print(f"merge {sources} -> {size} [{dev.type}]: max abs err {err:.3g} (values in [0, 1])")
    assert err <= 1e-6, err


# ---- leco_heat_overlay -----------------------------------------------------------------------------------------------------------
def test_overlay_matches_the_stated_formula(dev):
    from leco_amd import attn_maps
    g = torch.Generator().manual_seed(4)
    B, M, H, W = 2, 3, 9, 13
    heat = torch.rand(B, M, H, W, generator=g)
    heat[:, :, 0, :4] = 0.0                                # v = 0
    heat[:, :, 1, :4] = 0.5                                # v = 1 exactly (the full-heat value below)
    heat[:, :, 2, :4] = 3.0                                # above the maximum: clamped to 1
    heat[:, :, 3, :4] = -1.0                               # below zero: clamped to 0
    rmax = torch.full((B * M,), 2.0)                       # full heat at 0.5
    pic = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    lut = attn_maps.colour_table()
    assert lut.shape == (256, 3) and lut.dtype == torch.uint8
    alpha = 0.6
    for mi in range(M):
        out = torch.full((B, H, W, 3), 7, dtype=torch.uint8, device=dev)
        ops.heat_overlay(heat.to(dev), rmax.to(dev), pic.to(dev), lut.to(dev), out, B, M, mi, H, W, alpha).run()
        v = (heat[:, mi] * 2.0).clamp(0, 1)
        col = lut[(v * 255 + 0.5).floor().long()].float()
        av = (alpha * v)[..., None]
        ref = (pic.float() * (1 - av) + col * av + 0.5).floor().clamp(0, 255)
        diff = (out.cpu().float() - ref).abs().max().item()
        assert diff <= 1, diff
        assert torch.equal(out.cpu()[:, 0, :4], pic[:, 0, :4]) and torch.equal(out.cpu()[:, 3, :4], pic[:, 3, :4])      # v = 0: the picture
        full = (pic[:, 1, :4].float() * (1 - alpha) + lut[255].float() * alpha + 0.5).floor()
        assert (out.cpu()[:, 1, :4].float() - full).abs().max() <= 1
        assert (out.cpu()[:, 2, :4].float() - (pic[:, 2, :4].float() * (1 - alpha) + lut[255].float() * alpha + 0.5).floor()).abs().max() <= 1
    with pytest.raises(hip.LecoError):
        ops.heat_overlay(heat.to(dev), rmax.to(dev), pic.to(dev), lut.to(dev), out, B, M, M, H, W, alpha).run()
