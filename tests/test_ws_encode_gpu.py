"""-m gpu: clipmi_encode_image and clipmi_encode_text give the same bytes whatever their workspace and their output held
(tests/ws_cases.py: the table and the harness), equal to what CLIP.encode_image / CLIP.encode_text return for the same input; and
a workspace that larger and smaller batches have used before (CLIP._workspace keeps one per stream and tower) changes nothing.

Towers: the plain toy tower (width 128); toy-256 with 14-pixel patches (patch_k = 588 padded to 640: the padding columns must be
zero in a poisoned workspace; 101 tokens: the flash-style attention); ViT-B/32 as clipmi.CLIP packs it by default (LayerNorms folded,
the residual stream split); ViT-B/32 with FP8 weights (block scales padded to 256 rows). Images: B = 1, 2 (100 ViT-B/32 rows: the
skinny kernels and the statistics leaves), 6, 21 (1050 rows: the 256-row tiles, a ragged last tile, the scale padding)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import clip_case  # noqa: E402
import ws_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu

TOWERS = ["toy", "toy-256", "vitb32", "vitb32-fp8"]
BATCHES = [1, 2, 6, 21]
_models = {}


def _model(clipmi, gpu, name):
    if name not in _models:
        if name == "toy":
            sd, fmt = clip_case.state_dict("toy_seed0"), "bf16"
        elif name == "toy-256":
            sd, fmt = clipmi.weights.random_state_dict("toy-256", seed=6), "bf16"
        else:
            sd = _models.get("sd-b32")
            if sd is None:
                sd = _models["sd-b32"] = clip_case.state_dict("vitb32_seed0")
            fmt = "fp8" if name.endswith("fp8") else "bf16"
        _models[name] = clipmi.CLIP(sd, device=gpu, vision_weights=fmt)
    return _models[name]


def _pixels(model, B):
    g = torch.Generator(device=model.device)
    g.manual_seed(400 + B)
    R = model.dims["res"]
    return torch.randint(0, 256, (B, 3, R, R), generator=g, dtype=torch.uint8, device=model.device)


def _same_as(model_out, got, what):
    want = model_out.contiguous().cpu().numpy().view(np.uint8).reshape(-1)
    bad = np.flatnonzero(got["embeddings"] != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ from the wrapper's result, first at byte {bad[0]}"
    assert np.isfinite(got["embeddings"].view(np.float32)).all(), what


def test_the_towers_are_the_forms_the_docstring_names(clipmi, gpu):
    forms = {n: (_model(clipmi, gpu, n).vision.width, _model(clipmi, gpu, n).vision.ln_fold, _model(clipmi, gpu, n).vision.weight_format,
                 _model(clipmi, gpu, n).vision.patch_k, _model(clipmi, gpu, n).vision.tokens) for n in TOWERS}
    assert forms == {"toy": (128, 0, 0, 3072, 5), "toy-256": (256, 1, 0, 640, 101), "vitb32": (768, 1, 0, 3072, 50),
                     "vitb32-fp8": (768, 0, 1, 3072, 50)}, forms
    assert _model(clipmi, gpu, "vitb32").text.ln_fold == 1 and _model(clipmi, gpu, "toy").text.ln_fold == 0


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", TOWERS)
def test_encode_image(clipmi, gpu, name, B):
    model = _model(clipmi, gpu, name)
    px = _pixels(model, B)
    call, outputs, ws_bytes = W.encode_image_call(clipmi, model, px)
    got = W.run_independent(call, outputs, ws_bytes, device=gpu)
    _same_as(model.encode_image(px), got, f"{name} B={B}")


@pytest.mark.parametrize("Q", [1, 5])
@pytest.mark.parametrize("name", ["toy", "vitb32"])
def test_encode_text(clipmi, gpu, name, Q):
    """The tower trimmed to the longest prompt, as encode_text builds it; Q = 5: prompts of five lengths"""
    model = _model(clipmi, gpu, name)
    ids = W.prompts(model, Q)
    tower, ids_dev = W.text_tower(model, ids)
    assert tower.tokens < model.context_length
    call, outputs, ws_bytes = W.encode_text_call(clipmi, model, tower, ids_dev)
    got = W.run_independent(call, outputs, ws_bytes, device=gpu)
    _same_as(model.encode_text(ids), got, f"{name} text Q={Q}")


def _before(call, outputs, gpu):
    own = [torch.empty(nb, dtype=torch.uint8, device=gpu) for _, nb in outputs]
    return lambda ws, *_: call(ws, *own)


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name", TOWERS)
def test_image_batches_share_one_workspace(clipmi, gpu, name, order):
    """B = 21, then 2, then 1 through one workspace sized for 21 (every region of the smaller carve lies somewhere else in the bytes
    the larger one used) - and 1, 2, then 21"""
    model = _model(clipmi, gpu, name)
    seq = [W.encode_image_call(clipmi, model, _pixels(model, B)) for B in ((21, 2, 1) if order == "forward" else (1, 2, 21))]
    call, outputs, ws_bytes = seq[-1]
    alone = W.run_independent(call, outputs, ws_bytes, device=gpu)
    W.run_after([_before(c, o, gpu) for c, o, _ in seq[:-1]], call, outputs, max(w for _, _, w in seq), alone, device=gpu)


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name", ["toy", "vitb32"])
def test_prompt_batches_share_one_workspace(clipmi, gpu, name, order):
    model = _model(clipmi, gpu, name)
    seq = []
    for Q in ((5, 1) if order == "forward" else (1, 5)):
        tower, ids_dev = W.text_tower(model, W.prompts(model, Q))
        seq.append(W.encode_text_call(clipmi, model, tower, ids_dev) + (tower,))
    call, outputs, ws_bytes, _ = seq[-1]
    alone = W.run_independent(call, outputs, ws_bytes, device=gpu)
    W.run_after([_before(c, o, gpu) for c, o, _, _ in seq[:-1]], call, outputs, max(s[2] for s in seq), alone, device=gpu)
