"""The LoRA side of `infer.py` and `infer_xl.py`: `--lora FILE` (rank, alpha and coverage read from the file; `--rank` /
`--alpha` override), and the slider sweep `--lora_scales -2,-1,0,1,2`: one seed and one initial latent repeated for every
strength, all strengths through each denoising step as ONE batch (`LoRANetwork.set_strengths`), one contact-sheet PNG.

`--lora` may be given several times: the files are stacked (`LoRANetwork.from_files`).  `--lora_multipliers a,b,...` sets one
fixed multiplier per file; `--lora_scales`, given once per `--lora` in the same order, sweeps the cross product of the lists
(first file slowest) in one batched pass -- the contact sheet then has the last file's strengths left to right and all other
combinations top to bottom."""
import itertools

import torch

from leco_amd import model_util
from leco_amd.lora import LoRANetwork


def add_arguments(ap):
    ap.add_argument("--lora", action="append", default=None,
                    help="LoRA weights saved by train_lora.py / train_lora_xl.py; repeat the flag to stack several files")
    ap.add_argument("--rank", type=int, default=None, help="override the rank read from the --lora file (one --lora only)")
    ap.add_argument("--alpha", type=float, default=None, help="override the alpha read from the --lora file (one --lora only)")
    ap.add_argument("--lora_multipliers", default=None,
                    help="comma list of fixed multipliers, one per --lora (default: all 1)")
    ap.add_argument("--lora_scales", action="append", default=None,
                    help="comma list of LoRA strengths, e.g. -2,-1,0,1,2: the same seed at every strength in one batched pass "
                         "(needs --lora); --image becomes a contact sheet, left to right.  With several --lora: once per file, "
                         "in the same order -- the cross product is sampled, the last file's strengths run left to right")


def join_scales(argv):
    """`--lora_scales -2,-1,0,1,2` (and `--lora_multipliers -1,2`): argparse takes a value that starts with `-` and is no
    plain number for an option, so the flag and its value are joined into `--lora_scales=-2,-1,0,1,2` before parsing.
    ``argv`` None: the command line."""
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    out = []
    while argv:
        a = argv.pop(0)
        if a in ("--lora_scales", "--lora_multipliers") and argv:
            a += "=" + argv.pop(0)
        out.append(a)
    return out


def _floats(ap, flag, text):
    try:
        vals = [float(v) for v in text.split(",") if v.strip()]
    except ValueError:
        ap.error(f"{flag}: expected a comma list of numbers, got {text!r}")
    if not vals:
        ap.error(f"{flag}: no numbers given")
    return vals


def parse_scales(ap, args):
    """The strengths of `--lora_scales` (None without the flag): one --lora: the floats; several: the cross product of the
    lists as tuples, first file slowest.  Also checks the other LoRA flags against the number of files and leaves
    ``args.lora_multipliers`` as floats and ``args.sheet_cols`` = the pictures per contact-sheet row."""
    files = len(args.lora or ())
    if files > 1 and (args.rank is not None or args.alpha is not None):
        ap.error("--rank / --alpha override what ONE --lora file says; they cannot be used with several")
    if args.lora_multipliers is not None:
        if not files:
            ap.error("--lora_multipliers needs --lora")
        args.lora_multipliers = _floats(ap, "--lora_multipliers", args.lora_multipliers)
        if len(args.lora_multipliers) != files:
            ap.error(f"--lora_multipliers: {len(args.lora_multipliers)} multipliers for {files} --lora")
    args.sheet_cols = None
    if args.lora_scales is None:
        return None
    if not files:
        ap.error("--lora_scales needs --lora")
    if len(args.lora_scales) != files:
        ap.error(f"--lora_scales was given {len(args.lora_scales)} times for {files} --lora: give it once per file, in the same order")
    lists = [_floats(ap, "--lora_scales", text) for text in args.lora_scales]
    args.sheet_cols = len(lists[-1])
    return lists[0] if files == 1 else list(itertools.product(*lists))


def load_network(unet, args, scales):
    """The network of `--lora` (None without it), with the fixed multipliers and the sweep's strengths set."""
    if not args.lora:
        return None
    if len(args.lora) == 1 and args.lora_multipliers is None:
        network = LoRANetwork.from_file(unet, args.lora[0], multiplier=1.0, rank=args.rank, alpha=args.alpha)
    else:
        if args.rank is not None or args.alpha is not None:
            raise ValueError("--rank / --alpha cannot be combined with --lora_multipliers")
        network = LoRANetwork.from_files(unet, args.lora, multipliers=args.lora_multipliers)
    if scales is not None:
        network.set_strengths(scales)
    return network


def write_sheet(latents, vae_path, png_path, dev, use_graphs=False, cols=None, on_pictures=None):
    """Decode every latent and save the pictures as one PNG: ``cols`` per row, left to right, rows top to bottom (None: one
    row of width n * W).  ``on_pictures``: called with the uint8 [n][H][W][3] pictures before the sheet is assembled
    (`--clip_score`)."""
    from leco_amd.vae import save_png
    vae = model_util.load_vae(vae_path).to(dev)
    vae.use_graphs = use_graphs
    img = vae.decode_to_uint8(latents.float())          # [n][H][W][3]
    if on_pictures is not None:
        on_pictures(img)
    cols = img.shape[0] if cols is None else cols
    rows = [torch.cat(list(img[i:i + cols]), dim=1) for i in range(0, img.shape[0], cols)]
    sheet = torch.cat(rows, dim=0).contiguous()
    save_png(sheet, png_path)
    vae.release()
    print(f"contact sheet {img.shape[0]} x {img.shape[2]}x{img.shape[1]} -> {png_path}")
