"""leco_amd.graphs: the binding of the hipGraph entry points, the "replay from a graph?" rule on the emulator, and the
engine lifecycle the VAE shares with the CLIP text encoder.  (What a capture computes is covered where the plans are:
test_vae.py, test_vae_encoder.py, test_clip.py, test_lora_sweep.py, test_unet.py.)"""
import ctypes as C

import torch

import conftest
from leco_amd import clip as CL
from leco_amd import graphs, hip, unet
from leco_amd import vae as V

bf = torch.bfloat16


def test_graph_entry_points_are_declared_on_every_bound_library(dev):
    """ctypes argument types belong to one loaded-library object, and every GPU-tier test binds a new one: an entry point
    left undeclared would receive a 64-bit stream handle as a C int.  Captures nothing, launches nothing."""
    lib1 = graphs.api()
    (conftest._bind_hip if dev.type == "cuda" else conftest._bind_emu)()      # the same file, a new CDLL object
    lib2 = graphs.api()
    assert lib2 is hip.lib() and lib2 is not lib1
    assert sorted(graphs.SIGNATURES) == ["leco_graph_begin_capture", "leco_graph_destroy", "leco_graph_end_capture",
                                         "leco_graph_launch"]
    for name, argtypes in graphs.SIGNATURES.items():
        fn = getattr(lib2, name)
        assert list(fn.argtypes) == argtypes and fn.restype is C.c_int, name
    lib3 = unet._graph_api()
    assert lib3 is lib2
    for name, argtypes in graphs.SIGNATURES.items():
        assert list(getattr(lib3, name).argtypes) == argtypes and getattr(lib3, name).restype is C.c_int, name


def _tiny_vae(seed):
    vae = V.init_synthetic_vae_(V.AutoencoderKL(V.tiny_vae_config(0.18215)), seed)
    with torch.no_grad():           # bf16-representable weights: holding them in bf16 or fp32 is the same model
        for p in vae.parameters():
            p.copy_(p.to(bf).float())
    return vae


def _latents(seed):
    return torch.randn(1, 4, 4, 4, generator=torch.Generator().manual_seed(seed)) * 0.25


def test_emulated_models_never_capture():
    conftest._bind_emu()
    cfg = CL.CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2,
                            projection_dim=128, eos_token_id=999, bos_token_id=998)
    m = CL.init_synthetic_clip_(CL.CLIPTextModel(cfg), 5)
    ids = torch.tensor([[998, 3, 4, 5, 6, 999, 0, 0]])
    vae, lat = _tiny_vae(11), _latents(12)
    assert m.use_graphs is True and vae.use_graphs is False      # the defaults
    got = {}
    for on in (True, False):
        m.use_graphs = vae.use_graphs = on
        assert not graphs.enabled(m) and not graphs.enabled(vae)
        out = m(ids)
        got[on] = (out.last_hidden_state, out.pooler_output, vae.decode(lat).sample)
        assert m.engine().plans[(1, 8)].graph is None and vae.engine().plan(1, 4, 4).graph is None
        assert "_capture_stream" not in m.__dict__ and "_capture_stream" not in vae.__dict__
        m.release()
        vae.release()
    assert all(torch.equal(a, b) for a, b in zip(got[True], got[False]))


def test_vae_engine_follows_its_parameters():
    """A checkpoint loaded, or a cast, after the first decode reaches the next decode: the packed operands are rebuilt."""
    conftest._bind_emu()
    lat = _latents(21)
    vae = _tiny_vae(31).to(bf)
    vae.release()                                       # nothing built yet: a no-op
    first = vae.decode(lat).sample
    eng = vae._engine
    assert eng is not None and vae.engine() is eng       # unchanged parameters keep their engine
    other = _tiny_vae(32)
    vae.load_state_dict(other.state_dict())
    assert vae._engine is None and not eng.plans
    second = vae.decode(lat).sample
    assert torch.equal(second, other.decode(lat).sample) and not torch.equal(second, first)
    eng = vae._engine
    assert vae.to(torch.float32) is vae and vae._engine is None and not eng.plans
    assert vae.post_quant_conv.weight.dtype == torch.float32
    assert torch.equal(vae.decode(lat).sample, second)
    assert vae._engine is not eng
    vae.release()
    other.release()
