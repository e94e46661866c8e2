"""Kernels added for the CLIP image tower and the CLIP score (csrc/vision.hip), each against a plain float64 / fp32 torch
statement of the same op on the same inputs, and `leco_attention_fwd` at the tower's own shape (257 tokens).  Runs on the
host emulator (CPU tier) and on the gfx950 build (`-m gpu`).  Bound: the project's one-bf16-rounding bound of
tests/test_clip_kernels.py (relative L2).  Output buffers carry NaN-filled guard rows in front and behind.

`leco_clip_preprocess` is checked twice: against a float64 statement of the same separable filter built from the same tap
tables, and against transformers' `CLIPImageProcessorPil` (PIL itself) per element in units of one 8-bit level.  The
second bound is computed from the table in use: PIL rounds to whole levels after its horizontal and after its vertical
pass, the kernel does not; the first rounding (<= 0.5) passes through the row taps (x sum |taps|), the second adds 0.5;
+ half an ulp of the kernel's bf16 result; + 1 level for PIL's fixed-point (2^-22, rounded) coefficients."""
import errno

import pytest
import torch

from conftest import rel_err
from leco_amd import clip_vision as CV
from leco_amd import hip, ops

bf = torch.bfloat16
TOLBF = 3e-3
GUARD = 2
MEAN, STD = CV.OPENAI_CLIP_MEAN, CV.OPENAI_CLIP_STD


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _last_error() -> str:
    return (hip.lib().leco_last_error() or b"").decode()


def _guarded(rows, cols, dev, dtype=bf):
    """[GUARD + rows + GUARD][cols] filled with NaN; returns the whole buffer and the view of the middle rows."""
    full = torch.full((rows + 2 * GUARD, cols), float("nan"), dtype=dtype, device=dev)
    return full, full[GUARD:GUARD + rows]


def _guards_untouched(full):
    return bool(torch.isnan(full[:GUARD].float()).all() and torch.isnan(full[-GUARD:].float()).all())


# ---- leco_clip_preprocess --------------------------------------------------------------------------------------------------------
def _picture(B, H, W, seed):
    """Smooth colour gradients + noise + saturated blocks (so that the cubic's overshoot meets the [0, 255] clamps)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([xx, yy, 1 - 0.5 * (xx + yy)], -1)[None] * 255
    img = base + 60 * torch.randn(B, H, W, 3, generator=g)
    img[:, : max(1, H // 4), : max(1, W // 3)] = 255 * (torch.rand(B, max(1, H // 4), max(1, W // 3), 3, generator=g) > 0.5)
    return img.round().clamp(0, 255).to(torch.uint8)


def _dense(tab, w, size):
    m = torch.zeros(tab.shape[0], size, dtype=torch.float64)
    for i in range(tab.shape[0]):
        s, n = int(tab[i, 0]), int(tab[i, 1])
        m[i, s:s + n] = w[i, :n].float().double()          # the fp32 weights the kernel reads
    return m


def _patch_rows(v, p, kp):
    """[B][3][S][S] -> [B * P][kp], column c p p + i p + j of row b P + py g + px; the padding columns zero."""
    B, _, S, _ = v.shape
    g = S // p
    out = torch.zeros(B * g * g, kp, dtype=v.dtype)
    for b in range(B):
        for py in range(g):
            for px in range(g):
                out[(b * g + py) * g + px, :3 * p * p] = v[b, :, py * p:(py + 1) * p, px * p:(px + 1) * p].reshape(-1)
    return out


def _preprocess_ref(img, S, p):
    """float64: column taps along every row, clamp, row taps, clamp, 1/255, mean / std, patch rows."""
    B, H, W, _ = img.shape
    (rt, rw, _), (ct, cw, _) = CV.preprocess_tables(H, W, S)
    R, Cm = _dense(rt, rw, H), _dense(ct, cw, W)
    x = img.double().permute(0, 3, 1, 2)
    hor = (x @ Cm.T).clamp(0, 255)
    ver = (R @ hor).clamp(0, 255)
    v = (ver / 255 - torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    return _patch_rows(v, p, -(-3 * p * p // 64) * 64), float(R.abs().sum(1).max())


def _preprocess_run(dev, img, S, p, ld_extra=0):
    B, H, W, _ = img.shape
    kp = -(-3 * p * p // 64) * 64
    P = (S // p) ** 2
    (rt, rw, rk), (ct, cw, ck) = CV.preprocess_tables(H, W, S)
    full, out = _guarded(B * P, kp + ld_extra, dev)
    ms = torch.tensor(MEAN + STD, dtype=torch.float32, device=dev)
    ops.clip_preprocess(img.to(dev), B, H, W, rt.to(dev), rw.float().to(dev), rk, ct.to(dev), cw.float().to(dev), ck, ms, S, p,
                        out, kp + ld_extra).run()
    _sync(dev)
    return full.cpu(), out.cpu(), kp


_pil_cache = {}


def _pil_levels(img, S):
    """transformers' CLIPImageProcessorPil on the same pixels, as 8-bit levels [B][3][S][S] (computed once per case)."""
    key = (tuple(img.shape), S, int(img.long().sum()))
    if key not in _pil_cache:
        tr = pytest.importorskip("transformers")
        pytest.importorskip("PIL")
        proc = tr.CLIPImageProcessorPil(size={"shortest_edge": S}, crop_size={"height": S, "width": S})
        pv = proc(images=[im.numpy() for im in img], return_tensors="pt", input_data_format="channels_last").pixel_values.double()
        _pil_cache[key] = (pv * torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
                           + torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)) * 255
    return _pil_cache[key]


PREP_CASES = [
    ("28x28 no resampling", 1, 28, 28, 28, 14),
    ("64x48 antialiased downscale + crop offset", 1, 64, 48, 28, 14),
    ("20x23 upscale, clamped border windows", 1, 20, 23, 28, 14),
    ("1x1", 1, 1, 1, 28, 14),
    ("batch of 2", 2, 40, 33, 28, 14),
    ("512x512 at S=224", 1, 512, 512, 224, 14),
]


@pytest.mark.parametrize("label,B,H,W,S,p", PREP_CASES, ids=[c[0].split()[0] for c in PREP_CASES])
def test_clip_preprocess(dev, label, B, H, W, S, p):
    img = _picture(B, H, W, 100 + H)
    ref, row_abs = _preprocess_ref(img, S, p)
    full, out, kp = _preprocess_run(dev, img, S, p)
    assert _guards_untouched(full)
    assert torch.isfinite(out.float()).all()
    assert (out[:, 3 * p * p:] == 0).all() and kp % 64 == 0 and kp - 3 * p * p < 64
    err = rel_err(out, ref)
    print(f"preprocess {label}: rel vs float64 filter {err:.3e}")
    assert err < TOLBF
    if (H, W) == (S, S):         # no resampling: exactly normalise + patchify, rounded once
        x = img.double().permute(0, 3, 1, 2)
        v = (x / 255 - torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
        assert rel_err(out, _patch_rows(v, p, kp)) < TOLBF
    # ---- against PIL, in 8-bit levels
    pil = _patch_rows(_pil_levels(img, S), p, kp)[:, :3 * p * p]
    std = torch.tensor(STD, dtype=torch.float64).repeat_interleave(p * p)
    mean = torch.tensor(MEAN, dtype=torch.float64).repeat_interleave(p * p)
    got = out[:, :3 * p * p].double()
    mine = (got * std + mean) * 255
    half_ulp = got.abs() * 2.0 ** -8 * std * 255
    bound = 0.5 * row_abs + 0.5 + 1.0 + half_ulp
    diff = (mine - pil).abs()
    print(f"preprocess {label}: max |kernel - PIL| {diff.max():.3f} levels, bound {bound.min():.3f} .. {bound.max():.3f} "
          f"(max sum |row taps| {row_abs:.3f})")
    assert (diff <= bound).all(), float((diff - bound).max())


def test_clip_preprocess_row_stride_and_batch_order(dev):
    """ldo > Kp: the columns past Kp are not written; picture 1 of a batch equals the same picture alone."""
    img = _picture(2, 31, 45, 7)
    full, out, kp = _preprocess_run(dev, img, 28, 14, ld_extra=8)
    assert _guards_untouched(full) and torch.isnan(out[:, kp:].float()).all() and torch.isfinite(out[:, :kp].float()).all()
    _, alone, _ = _preprocess_run(dev, img[1:], 28, 14)
    assert torch.equal(out[4:, :kp].view(torch.int16), alone.view(torch.int16))


# ---- leco_vit_embed -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cw", [128, 72])
def test_vit_embed(dev, Cw):
    torch.manual_seed(50 + Cw)
    B, T = 2, 4
    patches = torch.randn(B * T, Cw).to(bf)
    cls, pos = torch.randn(Cw).to(bf), torch.randn(T + 1, Cw).to(bf)
    full, out = _guarded(B * (T + 1), Cw, dev)
    ops.vit_embed(patches.to(dev), Cw, cls.to(dev), pos.to(dev), Cw, out, Cw, B, T, Cw).run()
    _sync(dev)
    tok = torch.cat([cls.float().expand(B, 1, Cw), patches.float().view(B, T, Cw)], 1) + pos.float()
    assert _guards_untouched(full.cpu())
    assert torch.equal(out.cpu().view(torch.int16), tok.to(bf).view(B * (T + 1), Cw).view(torch.int16))      # one rounding: exact


# ---- leco_cosine_scores -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,Dm", [(3, 2, 64), (1, 1, 768), (9, 3, 1024)])
def test_cosine_scores(dev, B, T, Dm):
    torch.manual_seed(60 + Dm)
    x, y = torch.randn(B, Dm).to(bf), (torch.randn(T, Dm) * 3).to(bf)
    if B > 1:
        x[1] = 0                  # an all-zero row: 0, not NaN
    ref = torch.nn.functional.normalize(x.double(), dim=1, eps=1e-12) @ torch.nn.functional.normalize(y.double(), dim=1, eps=1e-12).T
    for scale in (1.0, 100.0):
        full, out = _guarded(B, T, dev, torch.float32)
        ops.cosine_scores(x.to(dev), Dm, y.to(dev), Dm, out, T, B, T, Dm, scale).run()
        _sync(dev)
        assert _guards_untouched(full.cpu())
        err = (out.cpu().double() / scale - ref).abs().max().item()
        print(f"cosine scores B={B} T={T} D={Dm} scale={scale}: max abs {err:.3e}")
        assert err <= 1e-5
        if B > 1:
            assert (out.cpu()[1] == 0).all()
    assert ref.abs().max() <= 1 + 1e-12


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def _rc(op):
    return op.fn(*op.args, ops.default_stream())


def test_argument_errors_launch_nothing(dev):
    S, p, kp = 28, 14, 640
    img = _picture(1, 9, 9, 1).to(dev)
    (rt, rw, rk), (ct, cw, ck) = CV.preprocess_tables(9, 9, S)
    rt, rw, ct, cw = rt.to(dev), rw.float().to(dev), ct.to(dev), cw.float().to(dev)
    ms = torch.tensor(MEAN + STD, dtype=torch.float32, device=dev)
    full, out = _guarded(4, kp, dev)

    def prep(batch=1, S=S, p=p, ldo=kp, img=img, rk=rk):
        return _rc(ops.clip_preprocess(img, batch, 9, 9, rt, rw, rk, ct, cw, ck, ms, S, p, out, ldo))
    assert prep(S=30) == -errno.EINVAL and "multiple of patch_size" in _last_error()
    assert prep(batch=0) == -errno.EINVAL and "empty" in _last_error()
    assert prep(ldo=kp - 8) == -errno.EINVAL and "ldo" in _last_error()
    assert prep(ldo=kp + 4) == -errno.EINVAL and "ldo" in _last_error()
    assert prep(img=None) == -errno.EINVAL and "(img)" in _last_error()
    assert prep(rk=0) == -errno.EINVAL and "row_taps" in _last_error()

    Cw = 64
    t = torch.zeros(8, Cw, dtype=bf, device=dev)

    def emb(c=Cw, ldp=Cw, ldo=kp, batch=1, cls=t):
        return _rc(ops.vit_embed(t, ldp, cls, t, Cw, out, ldo, batch, 3, c))
    assert emb(c=60) == -errno.EINVAL and "c=60" in _last_error()
    assert emb(ldp=68) == -errno.EINVAL and "strides" in _last_error()
    assert emb(ldo=Cw + 4) == -errno.EINVAL and "strides" in _last_error()
    assert emb(batch=0) == -errno.EINVAL and "empty" in _last_error()
    assert emb(cls=None) == -errno.EINVAL and "(cls)" in _last_error()

    fo = torch.full((4, 4), float("nan"), device=dev)

    def cos(d=Cw, ldx=Cw, nb=2, y=t):
        return _rc(ops.cosine_scores(t, ldx, y, Cw, fo, 4, nb, 2, d, 1.0))
    assert cos(d=60) == -errno.EINVAL and "d=60" in _last_error()
    assert cos(ldx=68) == -errno.EINVAL and "strides" in _last_error()
    assert cos(nb=0) == -errno.EINVAL and "empty" in _last_error()
    assert cos(y=None) == -errno.EINVAL and "(y)" in _last_error()
    _sync(dev)
    assert torch.isnan(full.float()).all() and torch.isnan(fo).all()      # nothing was launched
    assert prep() == 0 and emb() == 0 and cos() == 0
    _sync(dev)


# ---- leco_attention_fwd at the tower's shape ----------------------------------------------------------------------------------
@pytest.mark.parametrize("Dh", [64, 80])
def test_attention_at_257_tokens(dev, Dh):
    """B = 1, 16 heads, sq = skv = 257 (not a multiple of the 64-key tile: the masked path) on column views of a fused
    q|k|v buffer, as the tower launches it."""
    torch.manual_seed(70 + Dh)
    B, H, S = 1, 16, 257
    Cw = H * Dh
    qkv = torch.randn(B, S, 3 * Cw).to(bf)
    sp = lambda t: t.float().reshape(B, S, H, Dh).permute(0, 2, 1, 3)      # noqa: E731
    q, k, v = (sp(qkv[..., i * Cw:(i + 1) * Cw]) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2) * Dh ** -0.5, -1) @ v).permute(0, 2, 1, 3).reshape(B * S, Cw)
    d = qkv.to(dev)
    full, out = _guarded(B * S, Cw, dev)
    lse = torch.zeros(B * H * S, device=dev)
    q0, ld = d.data_ptr(), 3 * Cw
    ops.attention_fwd(q0, ld, S * ld, q0 + 2 * Cw, ld, S * ld, q0 + 4 * Cw, ld, S * ld, out.data_ptr(), Cw, S * Cw, lse, B, H, S, S,
                      Dh, Dh ** -0.5).run()
    _sync(dev)
    assert _guards_untouched(full.cpu())
    err = rel_err(out.cpu(), ref)
    print(f"attention 257 tokens d={Dh}: rel {err:.3e}")
    assert err < TOLBF
