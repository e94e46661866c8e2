"""The LoRA side of `infer.py` and `infer_xl.py`: `--lora FILE` (rank, alpha and coverage read from the file; `--rank` /
`--alpha` override), and the slider sweep `--lora_scales -2,-1,0,1,2`: one seed and one initial latent repeated for every
strength, all strengths through each denoising step as ONE batch (`LoRANetwork.set_strengths`), one contact-sheet PNG."""
import torch

from leco_amd import model_util
from leco_amd.lora import LoRANetwork


def add_arguments(ap):
    ap.add_argument("--lora", default=None, help="LoRA weights saved by train_lora.py / train_lora_xl.py")
    ap.add_argument("--rank", type=int, default=None, help="override the rank read from the --lora file")
    ap.add_argument("--alpha", type=float, default=None, help="override the alpha read from the --lora file")
    ap.add_argument("--lora_scales", default=None,
                    help="comma list of LoRA strengths, e.g. -2,-1,0,1,2: the same seed at every strength in one batched pass "
                         "(needs --lora); --image becomes a contact sheet, left to right")


def join_scales(argv):
    """`--lora_scales -2,-1,0,1,2`: argparse takes a value that starts with `-` and is no plain number for an option, so
    the flag and its value are joined into `--lora_scales=-2,-1,0,1,2` before parsing.  ``argv`` None: the command line."""
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    out = []
    while argv:
        a = argv.pop(0)
        if a == "--lora_scales" and argv:
            a += "=" + argv.pop(0)
        out.append(a)
    return out


def parse_scales(ap, args):
    """The strengths of `--lora_scales` as floats (None without the flag)."""
    if args.lora_scales is None:
        return None
    if not args.lora:
        ap.error("--lora_scales needs --lora")
    try:
        scales = [float(v) for v in args.lora_scales.split(",") if v.strip()]
    except ValueError:
        ap.error(f"--lora_scales: expected a comma list of numbers, got {args.lora_scales!r}")
    if not scales:
        ap.error("--lora_scales: no strengths given")
    return scales


def load_network(unet, args, scales):
    """The network of `--lora` (None without it), with the sweep's strengths set."""
    if not args.lora:
        return None
    network = LoRANetwork.from_file(unet, args.lora, multiplier=1.0, rank=args.rank, alpha=args.alpha)
    if scales is not None:
        network.set_strengths(scales)
    return network


def write_sheet(latents, vae_path, png_path, dev, use_graphs=False):
    """Decode every latent and save the pictures side by side, left to right, as one PNG of width n * W."""
    from leco_amd.vae import save_png
    vae = model_util.load_vae(vae_path).to(dev)
    vae.use_graphs = use_graphs
    img = vae.decode_to_uint8(latents.float())          # [n][H][W][3]
    sheet = torch.cat(list(img), dim=1).contiguous()
    save_png(sheet, png_path)
    vae.release()
    print(f"contact sheet {img.shape[0]} x {img.shape[2]}x{img.shape[1]} -> {png_path}")
