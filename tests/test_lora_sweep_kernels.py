"""`leco_lora_rowscale` (csrc/elementwise.hip): the per-sample strength applied to the low-rank image T of a LoRA site, in
place -- against ``(T.float() * s[row // rows_per_sample]).to(bf16)``, BIT-equal (one fp32 multiply and one rounding leave no
room for a tolerance), on the host emulator of the kernel sources and (marked `gpu`) on gfx950."""
import pytest
import torch

from leco_amd import hip, ops

bf = torch.bfloat16
SENTINEL = -1234.0                      # exactly representable in bf16; no product below comes near it
POOL = [0.0, -1.5, 1.0, 2.0 ** -20, 0.7]
GUARD = 3                               # guard rows in front of and behind T


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _case(dev, cols, ld, rps, samples, shift):
    rows = rps * samples
    g = torch.Generator().manual_seed(1000 * cols + 10 * rps + samples)
    buf = torch.full((GUARD + rows + GUARD, ld), SENTINEL, dtype=bf)
    buf[GUARD:GUARD + rows, :cols] = (torch.randn(rows, cols, generator=g) * 3).to(bf)
    s = torch.tensor((POOL[shift % 5:] + POOL[:shift % 5])[:samples], dtype=torch.float32)
    want = buf.clone()
    want[GUARD:GUARD + rows, :cols] = (buf[GUARD:GUARD + rows, :cols].float() * s.repeat_interleave(rps)[:, None]).to(bf)
    got = buf.to(dev)
    sd = s.to(dev)
    ops.lora_rowscale(got.data_ptr() + 2 * GUARD * ld, ld, rows, cols, rps, sd, keep=got).run()
    _sync(dev)
    return got.cpu(), want, s


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("cols", [32, 64, 128])
def test_lora_rowscale_is_bit_equal_and_stays_inside_its_columns(dev, cols, pad):
    """Every (rows_per_sample, samples) of {1, 77, 96, 256} x {1, 2, 5} -- sample boundaries inside a wave, several blocks --
    with the strengths 0, -1.5, 1, 2^-20 and 0.7 rotated through the samples; guard rows in front of and behind the buffer
    and the guard columns cols..ld hold a sentinel and must come back untouched."""
    ld = cols + pad
    used = set()
    for i, (rps, samples) in enumerate((r, n) for r in (1, 77, 96, 256) for n in (1, 2, 5)):
        got, want, s = _case(dev, cols, ld, rps, samples, i)
        used.update(s.tolist())
        inner = (slice(GUARD, GUARD + rps * samples), slice(0, cols))
        assert torch.equal(got[inner].view(torch.int16), want[inner].view(torch.int16)), (cols, ld, rps, samples)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), ("guards", cols, ld, rps, samples)
    assert {0.0, -1.5, 1.0, 2.0 ** -20} <= used


def test_lora_rowscale_reads_the_strengths_at_launch(dev):
    """The same Op run again after the strength vector changed on the device scales by the new values."""
    rows, cols, rps = 6, 32, 3
    t0 = (torch.randn(rows, cols, generator=torch.Generator().manual_seed(5)) * 2).to(bf)
    t = t0.clone().to(dev)
    s = torch.tensor([2.0, -1.0], device=dev)
    op = ops.lora_rowscale(t, cols, rows, cols, rps, s)
    op.run()
    s.copy_(torch.tensor([0.5, 3.0]))
    op.run()
    _sync(dev)
    want = (t0.float() * torch.tensor([2.0, -1.0]).repeat_interleave(rps)[:, None]).to(bf)
    want = (want.float() * torch.tensor([0.5, 3.0]).repeat_interleave(rps)[:, None]).to(bf)
    assert torch.equal(t.cpu().view(torch.int16), want.view(torch.int16))


def test_lora_rowscale_rejects_bad_arguments(dev):
    t = torch.zeros(8, 64, dtype=bf, device=dev)
    s = torch.ones(8, device=dev)
    for ld, rows, cols, rps in [(64, 8, 32, 3), (64, 8, 32, 0), (64, 8, 12, 1), (60, 8, 32, 1), (32, 8, 64, 1)]:
        with pytest.raises(hip.LecoError, match="lora_rowscale"):
            ops.lora_rowscale(t, ld, rows, cols, rps, s).run()
    with ops.f32_mode(True):
        with pytest.raises(NotImplementedError, match="bf16"):
            ops.lora_rowscale(t, 64, 8, 32, 1, s)
