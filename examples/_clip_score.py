"""The CLIP-score side of `infer.py` and `infer_xl.py`: `--clip_score TEXT` (repeatable, needs `--image`) scores every decoded
picture against every TEXT with the native CLIP image tower (`leco_amd.clip_vision`): the cosine between the picture's image
embedding and the prompt's text embedding.  The 8-bit pictures are scored where the VAE left them, on the device, before
the sheet is assembled.  One line per picture is printed -- with a sweep or a grid it carries that cell's strengths, in the
sheet's order -- and the same table goes to `<image stem>.scores.json`: prompts, strengths per cell, cosines.

`--clip_model` names the CLIP model: a local transformers `CLIPModel` folder or `synthetic:vit_tiny` / `synthetic:vit_l`
(random weights: the numbers mean nothing, the path is the real one).  For `synthetic:*` models it defaults to
`synthetic:vit_tiny`; for real models it has to be given."""
import json
import os

from leco_amd import model_util


def add_arguments(ap):
    ap.add_argument("--clip_score", action="append", default=None, metavar="TEXT",
                    help="score every picture of --image against TEXT (CLIP cosine); repeat the flag for several prompts")
    ap.add_argument("--clip_model", default=None,
                    help="CLIP model of --clip_score: a local transformers CLIPModel folder or synthetic:vit_tiny | "
                         "synthetic:vit_l (default for synthetic:* models: synthetic:vit_tiny)")


def check(ap, args):
    """The flags against each other, before anything is loaded; leaves ``args.clip_model`` resolved."""
    if not args.clip_score:
        if args.clip_model is not None:
            ap.error("--clip_model needs --clip_score")
        return
    if not args.image:
        ap.error("--clip_score needs --image: the decoded pictures are what is scored")
    if args.clip_model is None:
        if not args.model.startswith("synthetic:"):
            ap.error("--clip_score needs --clip_model for a real model (a local transformers CLIPModel folder)")
        args.clip_model = "synthetic:vit_tiny"
    m = args.clip_model         # fail before sampling, not after it
    if m.startswith("synthetic:") and m.split(":", 1)[1] not in model_util.SYNTHETIC_CLIP_SCORER \
            or not m.startswith("synthetic:") and not os.path.isfile(os.path.join(m, "config.json")):
        raise FileNotFoundError(f"--clip_model {m}: not a local transformers CLIPModel folder and not synthetic:vit_tiny | "
                                f"synthetic:vit_l")


def hook(args, scales, dev, use_graphs=False):
    """None without `--clip_score`; otherwise the callable `write_image` / `write_sheet` hand the uint8 [n][H][W][3] pictures."""
    if not args.clip_score:
        return None
    prompts = list(args.clip_score)
    cells = [None] if scales is None else [list(s) if isinstance(s, (tuple, list)) else [s] for s in scales]

    def score(img):
        scorer = model_util.load_clip_scorer(args.clip_model, native_text_encoder=args.native_text_encoder).to(dev)
        scorer.vision.use_graphs = use_graphs
        cos = scorer.score(img, prompts).cpu()
        scorer.release()
        if cos.shape[0] != len(cells):
            raise RuntimeError(f"--clip_score: {cos.shape[0]} pictures for {len(cells)} cells")
        for cell, row in zip(cells, cos.tolist()):
            at = "" if cell is None else " strengths " + ",".join(f"{v:g}" for v in cell)
            print("clip score" + at + ": " + "  ".join(f"{p!r} {v:+.4f}" for p, v in zip(prompts, row)))
        path = os.path.splitext(args.image)[0] + ".scores.json"
        with open(path, "w") as f:
            json.dump({"clip_model": args.clip_model, "prompts": prompts, "strengths": cells, "cosines": cos.tolist()}, f, indent=1)
        print(f"clip scores {tuple(cos.shape)} -> {path}")
    return score
