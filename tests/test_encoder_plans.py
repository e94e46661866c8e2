"""The launch lists of the two CLIP towers (leco_amd/clip.py, leco_amd/clip_vision.py), pinned label by label: both are built
from one encoder stack, and the measurement tools group launches by these labels.  Plans are only built here (on the host
emulator), never run."""
import torch

from conftest import _bind_emu
from leco_amd import clip as CL
from leco_amd import clip_vision as CV

LAYER = ["layernorm", "qkv", "attention", "out_proj", "layernorm", "fc1", "fc2"]
TEXT = ["embed"] + LAYER + LAYER + ["layernorm", "eos_gather"]
VISION = ["patch_embed", "embed", "layernorm"] + LAYER + LAYER + ["cls_gather", "layernorm", "projection"]


def _text_plan(projection):
    _bind_emu()
    cfg = CL.CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                            projection_dim=64, eos_token_id=999, bos_token_id=998)
    m = CL.init_synthetic_clip_((CL.CLIPTextModelWithProjection if projection else CL.CLIPTextModel)(cfg), 5).to(torch.bfloat16)
    return cfg, m.engine().plan(1, 8)


def test_text_plan_launch_names():
    cfg, plan = _text_plan(False)
    assert plan.names == TEXT and len(plan.names) == 1 + 7 * 2 + 2
    assert len(plan.ops) == len(plan.names) and plan.text_embeds is None
    assert len(plan.hidden) == len({h.data_ptr() for h in plan.hidden}) == cfg.num_hidden_layers + 1      # hidden_states keeps every layer
    cfg, plan = _text_plan(True)
    assert plan.names == TEXT + ["projection"] and len(plan.ops) == len(plan.names) == 1 + 7 * 2 + 3
    assert len(plan.hidden) == len({h.data_ptr() for h in plan.hidden}) == cfg.num_hidden_layers + 1


def test_vision_plan_launch_names():
    _bind_emu()
    cfg = CV.vit_tiny_config()
    assert cfg.num_hidden_layers == 2
    eng = CV.init_synthetic_clip_vision_(CV.CLIPVisionModelWithProjection(cfg), 5).to(torch.bfloat16).engine()
    plan = eng.plan(1)
    assert plan.names == VISION and len(plan.ops) == len(plan.names) == 3 + 7 * 2 + 3 and plan.img is None
    raw = eng.plan(1, (64, 48))
    assert raw.names == ["preprocess"] + VISION and len(raw.ops) == len(raw.names) and raw.img is not None
    assert sorted(eng.plans) == [(1,), (1, 64, 48)]
