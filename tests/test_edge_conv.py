"""The three conv_out exits (csrc/edge_conv.hip: `leco_conv_out`, `leco_conv_out_rgb`, `leco_conv_out_moments`) share one
loop: an output row depends only on its own weight row and on the summation order, so on the same input and the same weight
rows the exits agree bit for bit -- on the host emulator of the kernel sources and (marked `gpu`) on gfx950."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from leco_amd import ops

bf = torch.bfloat16
TOL32 = 1e-5          # fp32 outputs: the project's bound (tests/test_kernels.py)


# (1, 1, 1, 32): one pixel of a group of 16, only the centre tap inside the image, 3 units -- wave 3 loads nothing and adds zeros;
# (2, 3, 5, 160): 30 pixels -- a group across both images, a ragged last group -- and 15 units, one short of a full round;
# (1, 2, 9, 192): 18 units -- a second round with two live units
@pytest.mark.parametrize("B,h,w,c", [(1, 1, 1, 32), (2, 3, 5, 160), (1, 2, 9, 192)])
def test_conv_out_exits_share_one_loop(dev, B, h, w, c):
    g = torch.Generator().manual_seed(91)
    x = torch.randn(B, c, h, w, generator=g).to(bf)
    w8 = (torch.randn(8, c, 3, 3, generator=g) / (9 * c) ** 0.5).to(bf)
    bias = torch.randn(8, generator=g) * 0.1
    xcl = x.permute(0, 2, 3, 1).reshape(B * h * w, c).contiguous().to(dev)
    wcl = w8.permute(0, 2, 3, 1).contiguous().to(dev)               # [8][3][3][C]: the first rows are the other exits' weights
    bd = bias.to(dev)
    out4 = torch.zeros(B, 4, h, w, device=dev)
    rgb = torch.zeros(B, 3, h, w, device=dev)
    mom = torch.zeros(B, 8, h, w, device=dev)
    ops.conv_out(xcl, wcl[:4].contiguous(), bd[:4].contiguous(), out4, B, h, w, c, 4).run()
    ops.conv_out_rgb(xcl, wcl[:3].contiguous(), bd[:3].contiguous(), rgb, None, B, h, w, c).run()
    ops.conv_out_moments(xcl, wcl, bd, torch.eye(8, device=dev), torch.zeros(8, device=dev), None, mom, None, 1.0, B, h, w, c).run()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    out4, rgb, mom = out4.cpu(), rgb.cpu(), mom.cpu()
    ref = F.conv2d(x.float(), w8.float(), bias, padding=1)
    errs = rel_err(out4, ref[:, :4]), rel_err(rgb, ref[:, :3]), rel_err(mom, ref)
    print(f"conv_out exits {B}x{h}x{w} C={c}: rel conv_out {errs[0]:.3e}  rgb {errs[1]:.3e}  moments {errs[2]:.3e}")
    assert torch.equal(rgb[:, :3], out4[:, :3])
    assert torch.equal(mom[:, :4], out4)
    assert max(errs) < TOL32
