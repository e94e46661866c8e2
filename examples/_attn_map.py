"""The heatmap side of `infer.py` and `infer_xl.py`: `--attn_map WORD` (repeatable, needs `--image`) shows where in the picture
a prompt word acts -- the cross-attention probabilities of the word's tokens, averaged over heads, layers and denoising steps
(DAAM), collected on the device while the pictures are sampled (`UNet2DConditionModel.set_attention_maps`) and blended over
the decoded pictures (`leco_amd.attn_maps.overlay`, `--attn_map_alpha`).

WORD is looked up in the tokenized prompt (SDXL: the first tokenizer's positions); `#3` or `#3-5` name raw token positions
(0 = the start token), which is what `synthetic:*` models take.  `<image stem>.attn.png` repeats the layout of `--image` -- the
picture, or the contact sheet of `--lora_scales` -- once per word, top to bottom; `<image stem>.attn.json` holds the words,
their token positions, the strengths per cell (the cell order of `.scores.json`) and, per cell and word, the mean heat before
normalisation: the scalar that moves along a slider.  Every word is coloured on one scale across the cells (full heat = the
hottest pixel of that word in any cell), so the panels of a sheet compare."""
import json
import os

import torch

from leco_amd import attn_maps


def add_arguments(ap):
    ap.add_argument("--attn_map", action="append", default=None, metavar="WORD",
                    help="heatmap of where WORD of the prompt acts (cross-attention, DAAM); '#3' / '#3-5' = raw token positions; "
                         "repeat the flag for several words; writes <image stem>.attn.png and .attn.json")
    ap.add_argument("--attn_map_alpha", type=float, default=0.6, help="opacity of full heat over the picture (0..1)")


def check(ap, args):
    """The flags against each other, before anything is loaded."""
    if not args.attn_map:
        return
    if not args.image:
        ap.error("--attn_map needs --image: the heat is drawn over the decoded pictures")
    if len(args.attn_map) > 8:
        ap.error(f"--attn_map: {len(args.attn_map)} words given, at most 8 are supported")
    if not 0.0 <= args.attn_map_alpha <= 1.0:
        ap.error(f"--attn_map_alpha must be in [0, 1], got {args.attn_map_alpha}")


def start(args, unet, tokenizer, prompt):
    """Before sampling: the words' token weights into the UNet (None without `--attn_map`).  A word that is not in the prompt
    raises here, before a step is run."""
    if not args.attn_map:
        return None
    tok_w, where = attn_maps.token_weights(tokenizer, prompt, args.attn_map)
    unet.set_attention_maps(tok_w)
    unet.reset_attention_maps()
    return {"words": list(args.attn_map), "where": where}


def hook(args, scales, unet, state, cols=None, also=None):
    """The callable `write_image` / `write_sheet` hand the uint8 [n][H][W][3] pictures (``also``: another such callable, run
    first: `--clip_score`); ``also`` itself without `--attn_map`."""
    if state is None:
        return also
    cells = [None] if scales is None else [list(s) if isinstance(s, (tuple, list)) else [s] for s in scales]

    def draw(img):
        if also is not None:
            also(img)
        n, H, W, _ = img.shape
        heat = unet.attention_maps((H, W))                                   # [n][M][H][W]
        unet.set_attention_maps(None)
        if heat.shape[0] != len(cells) or n != len(cells):
            raise RuntimeError(f"--attn_map: {heat.shape[0]} heat maps, {n} pictures, {len(cells)} cells")
        peak = heat.amax(dim=(0, 2, 3))[None]                                # one scale per word across the cells
        over = attn_maps.overlay(heat, img, args.attn_map_alpha, peak=peak)  # [M][n][H][W][3]
        per_row = n if cols is None else cols
        blocks = []
        for m in range(over.shape[0]):
            rows = [torch.cat(list(over[m, i:i + per_row]), dim=1) for i in range(0, n, per_row)]
            blocks.append(torch.cat(rows, dim=0))
        from leco_amd.vae import save_png
        stem = os.path.splitext(args.image)[0]
        save_png(torch.cat(blocks, dim=0).contiguous(), stem + ".attn.png")
        mean = heat.mean(dim=(2, 3)).cpu()
        for cell, row in zip(cells, mean.tolist()):
            at = "" if cell is None else " strengths " + ",".join(f"{v:g}" for v in cell)
            print("mean heat" + at + ": " + "  ".join(f"{w!r} {v:.5f}" for w, v in zip(state["words"], row)))
        with open(stem + ".attn.json", "w") as f:
            json.dump({"prompt": args.prompt, "words": state["words"], "token_positions": state["where"], "strengths": cells,
                       "mean_heat": mean.tolist()}, f, indent=1)
        print(f"attention maps {len(state['words'])} words x {n} pictures -> {stem}.attn.png, {stem}.attn.json")
    return draw
