"""The img2img start shared by `infer.py` and `infer_xl.py` (`--init_image PNG --strength S`)."""
import torch

from leco_amd import model_util
from leco_amd.vae import load_png


def init_latents(args, sched, dev, use_graphs=False):
    """img2img start, the rule of diffusers' img2img pipelines: encode the PNG with the HIP VAE encoder (scaled latents sampled
    from the posterior with the script's seed), t_start = steps - min(int(steps * strength), steps), noise the latents to
    `timesteps[t_start]`.  Returns (fp32 latents, t_start); `sched.set_timesteps` has been called."""
    img = load_png(args.init_image)
    if tuple(img.shape[:2]) != (args.height, args.width):
        raise ValueError(f"--init_image {args.init_image} is {img.shape[1]}x{img.shape[0]} (width x height); --width x --height "
                         f"is {args.width}x{args.height}")
    t_start = args.steps - min(int(args.steps * args.strength), args.steps)
    if t_start >= args.steps:
        raise ValueError(f"--strength {args.strength} with --steps {args.steps} leaves no denoising step to run")
    vae = model_util.load_vae(args.vae or args.model, encoder=True).to(dev)
    vae.use_graphs = use_graphs
    gen = torch.Generator(device=dev if dev.type == "cuda" else "cpu").manual_seed(args.seed)
    latents = vae.encode_to_latents(img[None].to(dev), generator=gen)
    vae.release()
    noise = torch.randn(latents.shape, generator=gen, device=latents.device, dtype=torch.float32)
    latents = sched.add_noise(latents, noise, sched.timesteps[t_start])
    print(f"img2img: {args.init_image} -> latents {tuple(latents.shape)}, strength {args.strength}: steps {t_start}..{args.steps - 1}")
    return latents, t_start
