"""Picture against picture on the device: SSIM, PSNR and a change map -- what ELSE a LoRA changed, the preservation half of a
concept-erasure evaluation.  `compare` puts 8-bit pictures where the VAE left them (`decode_to_uint8`) against a baseline
through `leco_image_compare` (csrc/image_metrics.hip): the mean SSIM of Wang et al. 2004 (11 x 11 Gaussian window, sigma 1.5,
valid region), the exact squared error, from which MSE and PSNR follow on the host, and optionally the map 1 - ssim, which
`overlay_change` blends over the pictures with the heat colours of the attention maps (`attn_maps.overlay`)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import attn_maps, ops

WINDOW, SIGMA = 11, 1.5


def gaussian_taps() -> torch.Tensor:
    """The normalised 11-tap Gaussian window (sigma = 1.5) as float64 [11]; the kernel takes it rounded once to fp32."""
    x = torch.arange(WINDOW, dtype=torch.float64) - (WINDOW - 1) / 2
    g = torch.exp(-(x * x) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


@dataclass
class Comparison:
    """``ssim`` float64 [B] (mean over the valid region), ``sse`` int64 [B], ``mse`` / ``psnr`` float64 [B] (dB, peak 255; inf
    for identical pictures) on the host; ``change`` fp32 [B][H][W] = 1 - ssim on the pictures' device, 0 on the 5-pixel
    border (None unless asked for)."""
    ssim: torch.Tensor
    sse: torch.Tensor
    mse: torch.Tensor
    psnr: torch.Tensor
    change: Optional[torch.Tensor] = None


def compare(img_u8: torch.Tensor, ref_u8: torch.Tensor, change_map: bool = False) -> Comparison:
    """``img_u8`` uint8 [B][H][W][3] against ``ref_u8`` uint8 [H][W][3] or [1][H][W][3] (one baseline for every picture) or
    [B][H][W][3] (pairwise), on the same device; H, W >= 11."""
    if not isinstance(img_u8, torch.Tensor) or not isinstance(ref_u8, torch.Tensor):
        raise ValueError("compare: the pictures must be tensors")
    if img_u8.dtype != torch.uint8 or ref_u8.dtype != torch.uint8:
        raise ValueError(f"compare: the pictures must be uint8, got {img_u8.dtype} and {ref_u8.dtype}")
    if img_u8.dim() != 4 or img_u8.shape[-1] != 3 or img_u8.shape[0] < 1:
        raise ValueError(f"compare: the pictures must be [B][H][W][3] with B >= 1, got {tuple(img_u8.shape)}")
    B, H, W, _ = img_u8.shape
    if ref_u8.dim() == 3:
        ref_u8 = ref_u8[None]
    if tuple(ref_u8.shape) not in ((1, H, W, 3), (B, H, W, 3)):
        raise ValueError(f"compare: the baseline {tuple(ref_u8.shape)} must be [{H}][{W}][3], [1][{H}][{W}][3] or [{B}][{H}][{W}][3]")
    if ref_u8.device != img_u8.device:
        raise ValueError(f"compare: the pictures are on {img_u8.device}, the baseline on {ref_u8.device}")
    if H < WINDOW or W < WINDOW:
        raise ValueError(f"compare: pictures of {W}x{H} are smaller than the {WINDOW}x{WINDOW} SSIM window")
    img_u8, ref_u8 = img_u8.contiguous(), ref_u8.contiguous()
    dev = img_u8.device
    stride = H * W * 3 if ref_u8.shape[0] == B and B > 1 else 0
    taps = gaussian_taps().float().to(dev)
    stats = torch.empty((B, 2), dtype=torch.float64, device=dev)
    change = torch.empty((B, H, W), dtype=torch.float32, device=dev) if change_map else None
    ops.image_compare(img_u8, ref_u8, stride, B, H, W, taps, change, stats).run()
    st = stats.cpu()
    sse = st[:, 1].round().to(torch.int64)
    mse = st[:, 1] / float(H * W * 3)
    psnr = torch.tensor([math.inf if v == 0 else 10.0 * math.log10(255.0 * 255.0 / v) for v in mse.tolist()], dtype=torch.float64)
    return Comparison(ssim=st[:, 0].clone(), sse=sse, mse=mse, psnr=psnr, change=change)


def overlay_change(change: torch.Tensor, img_u8: torch.Tensor, full: Optional[float] = None, alpha: float = 0.6) -> torch.Tensor:
    """The pictures ``img_u8`` (uint8 [B][H][W][3]) with their change maps (fp32 [B][H][W], `compare(..., change_map=True)`)
    blended over them: uint8 [B][H][W][3].  ``full``: the value of 1 - ssim drawn as full heat, ONE scale for all pictures
    (default: the largest value of any map, or 1e-3 if all are smaller).  The blend is `attn_maps.overlay`."""
    if change.dim() != 3:
        raise ValueError(f"overlay_change: the change maps must be [B][H][W], got {tuple(change.shape)}")
    if full is None:
        full = max(float(change.amax()), 1e-3)
    if not full > 0:
        raise ValueError(f"overlay_change: full={full} must be > 0")
    peak = torch.full((1, 1), float(full), dtype=torch.float32, device=change.device)
    return attn_maps.overlay(change[:, None], img_u8, alpha, peak=peak)[0]
