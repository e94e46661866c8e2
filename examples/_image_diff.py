"""The preservation side of `infer.py` and `infer_xl.py`: `--image_diff [BASE]` (needs `--image`) says what ELSE changed -- every
decoded picture against a baseline picture, on the device, where the VAE left the 8-bit pictures
(`leco_amd.image_metrics.compare`: SSIM with the 11 x 11 Gaussian window, PSNR, MSE, and the change map 1 - ssim).

With `--lora_scales` BASE defaults to the cell whose strengths are all 0 (an error if the sweep has none); `-1`, or `0,1` for a
stack of two files, names another cell by its strengths.  BASE may also be a PNG of the pictures' size (`vae.load_png`), and
has to be one without `--lora_scales`.  One line per cell is printed; `<image stem>.diff.json` holds the baseline, the
strengths per cell (the cell order of `.scores.json`), `ssim`, `psnr` (null where the pictures are identical) and `mse`;
`<image stem>.diff.png` repeats the layout of `--image` with each cell's change map blended over it, all cells on ONE scale
(full heat = the largest 1 - ssim of any cell, or 1e-3 if all are smaller), so the cells compare by eye."""
import json
import math
import os

import torch

from leco_amd import image_metrics


def add_arguments(ap):
    ap.add_argument("--image_diff", nargs="?", const="", default=None, metavar="BASE",
                    help="SSIM / PSNR of every picture of --image against a baseline: the all-zero cell of --lora_scales "
                         "(default), another cell named by its strengths (-1, or 0,1 for a stack), or a PNG of the same size; "
                         "writes <image stem>.diff.json and .diff.png (the change maps over the pictures)")


def join_base(argv):
    """`--image_diff -1` / `--image_diff -1,0`: a BASE that starts with `-` would be taken for an option, so the flag and a
    following value that is no `--option` are joined into `--image_diff=-1,0` before parsing (cf. `_lora_sweep.join_scales`,
    which has already turned ``argv`` into a list)."""
    out, argv = [], list(argv)
    while argv:
        a = argv.pop(0)
        if a == "--image_diff" and argv and not argv[0].startswith("--"):
            a += "=" + argv.pop(0)
        out.append(a)
    return out


def _strengths(text):
    try:
        vals = [float(v) for v in text.split(",") if v.strip()]
    except ValueError:
        return None
    return vals or None


def check(ap, args, scales):
    """The flags against each other and the baseline resolved, before anything is loaded: leaves ``args.image_diff_base`` =
    ("cell", index) or ("png", uint8 [H][W][3])."""
    args.image_diff_base = None
    if args.image_diff is None:
        return
    if not args.image:
        ap.error("--image_diff needs --image: the decoded pictures are what is compared")
    if min(args.height, args.width) < image_metrics.WINDOW:
        ap.error(f"--image_diff: pictures of {args.width}x{args.height} are smaller than the SSIM window")
    cells = None if scales is None else [list(s) if isinstance(s, (tuple, list)) else [s] for s in scales]
    want = _strengths(args.image_diff) if args.image_diff else None
    if args.image_diff == "" or want is not None:
        if cells is None:
            ap.error("--image_diff without --lora_scales needs a baseline PNG: --image_diff BASE.png")
        want = [0.0] * len(cells[0]) if want is None else want
        if len(want) != len(cells[0]):
            ap.error(f"--image_diff {args.image_diff}: {len(want)} strengths name no cell of a sweep over {len(cells[0])} --lora")
        if want not in cells:
            ap.error("--image_diff: the sweep has no cell with strengths " + ",".join(f"{v:g}" for v in want)
                     + " to serve as the baseline; add it to --lora_scales, name another cell or give a PNG")
        args.image_diff_base = ("cell", cells.index(want))
        return
    from leco_amd.vae import load_png
    try:
        png = load_png(args.image_diff)
    except (OSError, ValueError) as e:
        ap.error(f"--image_diff {args.image_diff}: neither strengths nor a readable PNG ({e})")
    if tuple(png.shape[:2]) != (args.height, args.width):
        ap.error(f"--image_diff {args.image_diff} is {png.shape[1]}x{png.shape[0]} (width x height); --width x --height is "
                 f"{args.width}x{args.height}")
    args.image_diff_base = ("png", png)


def hook(args, scales, cols=None, also=None):
    """The callable `write_image` / `write_sheet` hand the uint8 [n][H][W][3] pictures (``also``: another such callable, run
    first: `--clip_score` / `--attn_map`); ``also`` itself without `--image_diff`."""
    if args.image_diff_base is None:
        return also
    cells = [None] if scales is None else [list(s) if isinstance(s, (tuple, list)) else [s] for s in scales]
    kind, base = args.image_diff_base

    def diff(img):
        if also is not None:
            also(img)
        n = img.shape[0]
        if n != len(cells):
            raise RuntimeError(f"--image_diff: {n} pictures for {len(cells)} cells")
        ref = img[base:base + 1] if kind == "cell" else base.to(img.device)[None]
        res = image_metrics.compare(img, ref, change_map=True)
        over = image_metrics.overlay_change(res.change, img)      # one scale for all cells
        per_row = n if cols is None else cols
        rows = [torch.cat(list(over[i:i + per_row]), dim=1) for i in range(0, n, per_row)]
        from leco_amd.vae import save_png
        stem = os.path.splitext(args.image)[0]
        save_png(torch.cat(rows, dim=0).contiguous(), stem + ".diff.png")
        ssim, psnr, mse = res.ssim.tolist(), res.psnr.tolist(), res.mse.tolist()
        for cell, s, p in zip(cells, ssim, psnr):
            at = "" if cell is None else " strengths " + ",".join(f"{v:g}" for v in cell)
            print(f"image diff{at}: ssim {s:.4f} psnr " + ("inf (identical)" if math.isinf(p) else f"{p:.2f} dB"))
        baseline = {"cell": base, "strengths": cells[base]} if kind == "cell" else {"png": args.image_diff}
        with open(stem + ".diff.json", "w") as f:
            json.dump({"baseline": baseline, "strengths": cells, "ssim": ssim, "psnr": [None if math.isinf(p) else p for p in psnr],
                       "mse": mse}, f, indent=1)
        print(f"image diff {n} pictures -> {stem}.diff.json, {stem}.diff.png")
    return diff
