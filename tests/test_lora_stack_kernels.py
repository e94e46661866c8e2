"""`leco_lora_rowscale_stack` (csrc/elementwise.hip): the per-sample, per-FILE strength applied to the low-rank image T of a
LoRA site of a stacked network, in place -- against ``(T.float() * S[row // rps][col_file[c % period]]).to(bf16)``, BIT-equal
(one fp32 multiply and one rounding leave no room for a tolerance), on the host emulator of the kernel sources and (marked
`gpu`) on gfx950."""
import pytest
import torch

from leco_amd import hip, ops

bf = torch.bfloat16
SENTINEL = -1234.0                      # exactly representable in bf16; no product below comes near it
SPECIAL = [0.0, -1.5, 1.0, 2.0 ** -20]  # every case uses these; the rest of its strengths are distinct fillers
GUARD = 3                               # guard rows in front of and behind T
# ranks of the stacked files -> period = their sum (None: one file whose block is the whole of `cols`)
LAYOUTS = [(4, 8),          # block boundary at 4: vectors straddle the two files and wrap the period of 12
           (4, 4, 12),      # three files, period 20: no multiple of 8
           (8, 16),         # aligned blocks
           (5, 3),          # odd boundary
           None]            # degenerate: one file, period = cols


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _table(ranks, cols):
    ranks = (cols,) if ranks is None else ranks
    return [j for j, r in enumerate(ranks) for _ in range(r)], len(ranks)


def _strengths(samples, files, shift):
    """[samples][files], all distinct within the case: the special values first (rotated by ``shift`` so that they meet
    different samples and files from case to case), then 0.7, 0.95, 1.2, ..."""
    n = samples * files
    vals = (SPECIAL + [0.7 + 0.25 * i for i in range(n)])[:max(n, len(SPECIAL))]
    vals = vals[shift % len(vals):] + vals[:shift % len(vals)]
    vals = vals[:n]
    assert len(set(vals)) == n
    return torch.tensor(vals, dtype=torch.float32).reshape(samples, files)


def _want(t, s, table, rps):
    rows, cols = t.shape
    f = torch.tensor([table[c % len(table)] for c in range(cols)])
    return (t.float() * s.repeat_interleave(rps, 0)[:, f]).to(bf)


def _case(dev, cols, ld, rps, samples, ranks, shift):
    rows = rps * samples
    table, files = _table(ranks, cols)
    g = torch.Generator().manual_seed(1000 * cols + 10 * rps + samples + 7 * len(table))
    buf = torch.full((GUARD + rows + GUARD, ld), SENTINEL, dtype=bf)
    buf[GUARD:GUARD + rows, :cols] = (torch.randn(rows, cols, generator=g) * 3).to(bf)
    s = _strengths(samples, files, shift)
    want = buf.clone()
    want[GUARD:GUARD + rows, :cols] = _want(buf[GUARD:GUARD + rows, :cols], s, table, rps)
    got = buf.to(dev)
    ops.lora_rowscale_stack(got.data_ptr() + 2 * GUARD * ld, ld, rows, cols, rps, s.to(dev), files, table, len(table), keep=got).run()
    _sync(dev)
    return got.cpu(), want, s


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("cols", [32, 64, 128])
def test_lora_rowscale_stack_is_bit_equal_and_stays_inside_its_columns(dev, cols, pad):
    """Every layout of LAYOUTS at every (rows_per_sample, samples) of {1, 77, 96, 256} x {1, 2, 5}; the strengths of a case
    are all distinct, so a strength taken from the wrong sample or the wrong file changes bits.  Guard rows in front of and
    behind the buffer and the guard columns cols..ld hold a sentinel and must come back untouched."""
    ld = cols + pad
    used = set()
    i = 0
    for ranks in LAYOUTS:
        for rps in (1, 77, 96, 256):
            for samples in (1, 2, 5):
                got, want, s = _case(dev, cols, ld, rps, samples, ranks, i)
                i += 1
                used.update(s.flatten().tolist())
                inner = (slice(GUARD, GUARD + rps * samples), slice(0, cols))
                assert torch.equal(got[inner].view(torch.int16), want[inner].view(torch.int16)), (cols, ld, rps, samples, ranks)
                assert torch.equal(got.view(torch.int16), want.view(torch.int16)), ("guards", cols, ld, rps, samples, ranks)
    assert {0.0, -1.5, 1.0, 2.0 ** -20} <= used


@pytest.mark.parametrize("cols", [32, 128])
def test_one_file_equals_lora_rowscale(dev, cols):
    """One file: the same bits as the existing `leco_lora_rowscale` on the same input, whatever the period."""
    rps, samples = 77, 5
    rows = rps * samples
    t0 = (torch.randn(rows, cols + 64, generator=torch.Generator().manual_seed(cols)) * 3).to(bf)
    s = torch.tensor([0.0, -1.5, 1.0, 2.0 ** -20, 0.7])
    a, b, c = t0.clone().to(dev), t0.clone().to(dev), t0.clone().to(dev)
    ops.lora_rowscale(a, cols + 64, rows, cols, rps, s.to(dev)).run()
    ops.lora_rowscale_stack(b, cols + 64, rows, cols, rps, s.reshape(samples, 1).to(dev), 1, [0] * cols, cols).run()
    ops.lora_rowscale_stack(c, cols + 64, rows, cols, rps, s.reshape(samples, 1).to(dev), 1, [0] * 12, 12).run()
    _sync(dev)
    assert torch.equal(a.cpu().view(torch.int16), b.cpu().view(torch.int16))
    assert torch.equal(a.cpu().view(torch.int16), c.cpu().view(torch.int16))
    assert not torch.equal(a.cpu().view(torch.int16), t0.view(torch.int16))


def test_lora_rowscale_stack_reads_the_strengths_at_launch(dev):
    """The same Op run again after the strength matrix changed on the device scales by the new values."""
    rows, cols, rps = 6, 32, 3
    table, _ = _table((4, 8), cols)
    t0 = (torch.randn(rows, cols, generator=torch.Generator().manual_seed(5)) * 2).to(bf)
    t = t0.clone().to(dev)
    s1, s2 = torch.tensor([[2.0, -1.0], [0.5, 3.0]]), torch.tensor([[0.25, 1.5], [-2.0, 0.75]])
    s = s1.clone().to(dev)
    op = ops.lora_rowscale_stack(t, cols, rows, cols, rps, s, 2, table, 12)
    op.run()
    s.copy_(s2)
    op.run()
    _sync(dev)
    want = _want(_want(t0, s1, table, rps), s2, table, rps)
    assert torch.equal(t.cpu().view(torch.int16), want.view(torch.int16))
    assert not torch.equal(want.view(torch.int16), _want(_want(t0, s1, table, rps), s1, table, rps).view(torch.int16))


def test_lora_rowscale_stack_rejects_bad_arguments(dev):
    t = torch.zeros(8, 64, dtype=bf, device=dev)
    s = torch.ones(8, 8, device=dev)
    table = torch.zeros(64, dtype=torch.int32, device=dev)
    good = dict(ld=64, rows=8, cols=32, rps=1, files=2, period=12)
    for bad in [dict(files=0), dict(files=9), dict(period=0), dict(cols=12), dict(ld=60), dict(ld=32, cols=64), dict(rps=3),
                dict(rps=0)]:
        a = dict(good, **bad)
        with pytest.raises(hip.LecoError, match="lora_rowscale_stack"):
            ops.lora_rowscale_stack(t, a["ld"], a["rows"], a["cols"], a["rps"], s, a["files"], table, a["period"]).run()
    ops.lora_rowscale_stack(t, 64, 8, 32, 1, s, 2, table, 12).run()          # (the base case itself is accepted)
    _sync(dev)
    for host_table in ([0, 1, 2], [0, -1, 1], [0, 1]):                            # an entry >= files, a negative one, a wrong length
        with pytest.raises(ValueError, match="col_file"):
            ops.lora_rowscale_stack(t, 64, 8, 32, 1, s, 2, host_table, 3)
    with ops.f32_mode(True):
        with pytest.raises(NotImplementedError, match="bf16"):
            ops.lora_rowscale_stack(t, 64, 8, 32, 1, s, 2, table, 12)
