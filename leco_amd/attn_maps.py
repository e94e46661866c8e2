"""Cross-attention token heatmaps: where in the picture a prompt word acts (DAAM: the softmax column of the word's tokens,
averaged over heads, layers and denoising steps, upsampled to the picture).

The UNet side is `UNet2DConditionModel.set_attention_maps` / `attention_maps` (leco_amd/unet.py): a plan variant that launches
`leco_xattn_token_maps` behind every cross-attention's `to_q` / `kv`.  This module holds what surrounds it: the token weights
of the words (`token_weights`), the colour table (`colour_table`) and the blend over the decoded pictures (`overlay`,
`leco_heat_overlay`)."""
from __future__ import annotations

import re
from typing import List, Sequence, Tuple

import torch

from . import ops

_RAW = re.compile(r"^#(\d+)(?:-(\d+))?$")


def _ids(tokenizer, text: str, whole: bool) -> List[int]:
    """Token ids of ``text``: the padded, truncated row the text encoder sees (``whole``) or the bare tokens of a word."""
    if whole:
        out = tokenizer(text, padding="max_length", max_length=tokenizer.model_max_length, truncation=True)
    else:
        out = tokenizer(text, add_special_tokens=False)
    ids = out.input_ids
    if isinstance(ids, torch.Tensor):
        ids = ids.reshape(-1).tolist()
    if ids and isinstance(ids[0], (list, tuple)):
        ids = list(ids[0])
    if not all(isinstance(i, int) for i in ids):
        raise ValueError("this tokenizer gives no token ids (a synthetic:* model): name raw token positions, '#3' or '#3-5'")
    return list(ids)


def token_weights(tokenizer, prompt: str, words: Sequence[str], length: int = 77) -> Tuple[torch.Tensor, List[List[int]]]:
    """(fp32 [len(words)][length] token weights, the token positions per word) for `set_attention_maps`.

    A word is looked up as the token-id subsequence of its own tokenization inside the tokenized prompt (every occurrence
    counts; a word of several tokens gives a row with several ones).  ``"#3"`` and ``"#3-5"`` name raw positions of the
    token row (0 = the start token), so models without a real tokenizer (`synthetic:*`) work.  A word that is not in the
    prompt, or a position outside the row, raises ValueError."""
    if not 1 <= len(words) <= ops.TOKEN_MAPS_MAX:
        raise ValueError(f"attention maps: {len(words)} words given, 1..{ops.TOKEN_MAPS_MAX} are supported")
    tw = torch.zeros(len(words), length)
    where: List[List[int]] = []
    row = None
    for m, word in enumerate(words):
        raw = _RAW.match(word.strip())
        if raw:
            lo = int(raw.group(1))
            hi = lo if raw.group(2) is None else int(raw.group(2))
            if not lo <= hi < length:
                raise ValueError(f"attention maps: {word!r} names positions outside the {length}-token row")
            pos = list(range(lo, hi + 1))
        else:
            if row is None:
                row = _ids(tokenizer, prompt, True)[:length]
            sub = _ids(tokenizer, word, False)
            pos = [] if not sub else [i + t for i in range(len(row) - len(sub) + 1) if row[i:i + len(sub)] == sub
                                      for t in range(len(sub))]
            if not pos:
                raise ValueError(f"attention maps: the word {word!r} does not occur in the prompt {prompt!r}")
            pos = sorted(set(pos))
        tw[m, pos] = 1.0
        where.append(pos)
    return tw, where


def colour_table() -> torch.Tensor:
    """The fixed 256-entry heat colour table, uint8 [256][3]: black - blue - cyan - green - yellow - red ("jet" without the
    dark ends), piecewise linear in five segments."""
    stops = torch.tensor([[0, 0, 128], [0, 0, 255], [0, 255, 255], [255, 255, 0], [255, 0, 0], [128, 0, 0]], dtype=torch.float32)
    x = torch.linspace(0, len(stops) - 1, 256)
    i = x.floor().clamp(max=len(stops) - 2).long()
    f = (x - i.float())[:, None]
    return (stops[i] * (1 - f) + stops[i + 1] * f + 0.5).floor().clamp(0, 255).to(torch.uint8)


def overlay(heat: torch.Tensor, img_u8: torch.Tensor, alpha: float = 0.6, peak: torch.Tensor = None) -> torch.Tensor:
    """The pictures ``img_u8`` (uint8 [B][H][W][3], on the device) with the heat maps ``heat`` (fp32 [B][M][H][W]) blended over
    them: uint8 [M][B][H][W][3], one set of pictures per word.  Each map is normalised by ``peak`` (fp32 [B][M] or broadcastable;
    default: the map's own maximum), so full heat is the hottest pixel.  The blend is `leco_heat_overlay`."""
    B, M, H, W = heat.shape
    if tuple(img_u8.shape) != (B, H, W, 3) or img_u8.dtype != torch.uint8:
        raise ValueError(f"overlay: pictures {tuple(img_u8.shape)} {img_u8.dtype} do not match heat {tuple(heat.shape)}")
    heat = heat.float().contiguous()
    img_u8 = img_u8.contiguous()
    top = heat.amax(dim=(2, 3)) if peak is None else peak.to(heat.device, torch.float32).expand(B, M)
    rmax = torch.where(top > 0, 1.0 / top.clamp_min(1e-30), torch.zeros_like(top)).reshape(-1).contiguous()
    lut = colour_table().to(heat.device)
    out = torch.empty((M, B, H, W, 3), dtype=torch.uint8, device=heat.device)
    for m in range(M):
        ops.heat_overlay(heat, rmax, img_u8, lut, out[m], B, M, m, H, W, alpha).run()
    return out
