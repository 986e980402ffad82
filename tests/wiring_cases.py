"""Cases for the wiring between the packed weight blob and the towers' launches (weights._pack_layers, ln_fold_terms*, LayerW
and the block forms of csrc/encode.hip): ONE tensor loud at a time. No tests here: tests/test_wiring.py (CPU, oracle only)
proves that every case tells the right state dict from every wrong one by a wide margin, tests/test_wiring_gpu.py (-m gpu)
holds the device towers to the oracle on the loud dicts.

A case is (key, part): a tensor of a tower's state dict, or one Q / K / V third of in_proj_weight / in_proj_bias. Its loud
dict is the form's seeded base dict with that tensor replaced by loud(): far away from its base value, from the same-named
tensor of every other layer and from its sibling, so that a dropped, stale, mis-layered or mis-sliced tensor moves the
embedding by many tolerances of the end-to-end rule (err <= 3 x bf16-emulation noise + 1e-3) instead of a fraction of one.
faults() lists the wrong dicts. The K third of in_proj_bias is no case: softmax does not see a per-query constant, so the
reference does not depend on it (test_wiring.py pins that)."""
import functools
import os
import sys
import zlib
from collections import namedtuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import clipmi  # noqa: E402
from oracle import clip_oracle  # noqa: E402

INPUT_SEED = 3
LOUD_SEED = 3            # every case's generator is seeded by this, the architecture and the case's name
# one parametrisation of the GPU test each. n: images / prompts of the device call; rows: the ones compared (the oracle runs
# on those only: a row does not depend on its batch, test_encode_image_batch_invariance_and_dtypes). leaves / tail_leaves /
# persistent: what the plan's queries must answer for the form's shapes (the block GEMMs hand the row statistics on as
# leaves; the pruned tail does; c_fc runs on the persistent FP8 kernel that emits MX rows itself).
FORMS = {
    # blocks_plain, tail_plain
    "plain-vision": dict(arch="toy", seed=0, tower="vision", n=4, rows=(0, 1, 2, 3), fold=0, fp8=False),
    # blocks_plain, causal, EOT row gather
    "plain-text": dict(arch="toy", seed=0, tower="text", eot=(3, 7, 11, 15), fold=0, fp8=False),
    # M = 101: blocks_ln with ln_leaf, tail_ln with leaves
    "fold-vision-leaves": dict(arch="toy-256", seed=5, tower="vision", n=1, rows=(0,), fold=1, fp8=False,
                               leaves=True, tail_leaves=True),
    # M = 202: blocks_ln on partials, tail_ln with leaves
    "fold-vision-partials": dict(arch="toy-256", seed=5, tower="vision", n=2, rows=(0, 1), fold=1, fp8=False,
                                 leaves=False, tail_leaves=True),
    # B = 130 > 128: tail_ln without leaves
    "fold-vision-wide-tail": dict(arch="toy-256", seed=5, tower="vision", n=130, rows=(0, 1, 128, 129), fold=1, fp8=False,
                                  leaves=False, tail_leaves=False),
    # M = 64: blocks_ln causal on leaves, split-residual head
    "fold-text-leaves": dict(arch="toy-t256", seed=1, tower="text", eot=(3, 7, 11, 15), fold=1, fp8=False, leaves=True),
    # M = 144: the same on partials
    "fold-text-partials": dict(arch="toy-t256", seed=1, tower="text", eot=(1, 2, 3, 5, 7, 9, 11, 13, 15), fold=1, fp8=False,
                               leaves=False),
    # blocks_fp8 on the non-persistent kernels
    "fp8-vision": dict(arch="toy-256", seed=5, tower="vision", n=2, rows=(0, 1), fold=0, fp8=True, persistent=False),
    # 700 images: blocks_fp8 with the MX-emitting persistent c_fc
    "fp8-vision-persistent": dict(arch="toy-256", seed=5, tower="vision", n=700, rows=(0, 1, 698, 699), fold=0, fp8=True,
                                  persistent=True),
}
BF16_FORMS = [f for f, d in FORMS.items() if not d["fp8"]]
FP8_FORMS = [f for f, d in FORMS.items() if d["fp8"]]

# what the CPU test requires of every fault, and the GPU tests rely on
BF16_MARGIN = 8.0        # a fault moves the oracle by >= this x the tolerance the GPU test applies to the case
FP8_MARGIN = 3.0         # ... separates the product emulations by >= this x |row-scale emulation - product emulation|

# loudness per tensor class (the s of loud()); raise one where a margin is missed, never lower a margin.
# q_bias (the Q third of in_proj_bias) and qk_weight (the Q and K thirds of in_proj_weight) reach the output through the
# softmax alone, and in a vision tower's last block through the class token's query alone: at 1.0 their weakest faults sat at
# 4.3 .. 7.9 tolerances (2.2 yardsticks in the FP8 emulation) for six seeds out of six. Louder scores also saturate the
# softmax and raise the emulation noise with them, so more than this gains nothing (measured up to 4.0).
LOUDNESS ={"matrix": 1.0, "gamma": 1.0, "vector": 1.0, "q_bias": 3.0, "qk_weight": 2.0}

Case = namedtuple("Case", "key part")          # part: None, or 0 / 1 / 2 = the Q / K / V third of in_proj_*

_MATRICES = ("conv1.weight", "in_proj_weight", "out_proj.weight", "c_fc.weight", "c_proj.weight", "visual.proj",
             "text_projection", "token_embedding.weight")
_GAMMAS = ("ln_1.weight", "ln_2.weight", "ln_pre.weight", "ln_post.weight", "ln_final.weight")
_LAYER_KEYS = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
               "attn.out_proj.bias", "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight",
               "mlp.c_proj.bias")
_TOWER_KEYS = {"vision": ("visual.conv1.weight", "visual.class_embedding", "visual.positional_embedding", "visual.ln_pre.weight",
                          "visual.ln_pre.bias", "visual.ln_post.weight", "visual.ln_post.bias", "visual.proj"),
               "text": ("token_embedding.weight", "positional_embedding", "ln_final.weight", "ln_final.bias", "text_projection")}
_PREFIX = {"vision": "visual.transformer", "text": "transformer"}
_SIBLINGS = {"attn.out_proj.bias": "mlp.c_proj.bias", "ln_1.weight": "ln_2.weight", "ln_1.bias": "ln_2.bias",
             "visual.ln_pre.weight": "visual.ln_post.weight", "visual.ln_pre.bias": "visual.ln_post.bias"}
_SIBLINGS.update({v: k for k, v in list(_SIBLINGS.items())})


def tensor_class(key):
    return "matrix" if key.endswith(_MATRICES) else "gamma" if key.endswith(_GAMMAS) else "vector"


def loudness(case):
    if case.part in (0, 1):
        return LOUDNESS["q_bias" if case.key.endswith("in_proj_bias") else "qk_weight"]
    return LOUDNESS[tensor_class(case.key)]


def loud(key, tensor, gen, s):
    """The loud version of a tensor (or of one third of it): vectors s randn, LayerNorm gammas 1 + s randn, matrices
    t + s std(t) randn."""
    r = torch.randn(tensor.shape, generator=gen, dtype=torch.float32)
    cls = tensor_class(key)
    if cls == "matrix":
        return tensor + s * tensor.std() * r
    return 1.0 + s * r if cls == "gamma" else s * r


@functools.lru_cache(maxsize=None)
def _base(arch, seed):
    return clipmi.weights.random_state_dict(arch, seed=seed)


def base_sd(form):
    """The form's seeded state dict. Shared: never written to."""
    return _base(FORMS[form]["arch"], FORMS[form]["seed"])


def n_layers(form):
    a = clipmi.weights.ARCHS[FORMS[form]["arch"]]
    return a["v_layers"] if FORMS[form]["tower"] == "vision" else a["t_layers"]


def _layer_key(form, l, rest):
    return f"{_PREFIX[FORMS[form]['tower']]}.resblocks.{l}.{rest}"


def _split_key(form, key):
    """-> (layer, rest) for a block tensor, (None, key) for a tensor of the tower"""
    p = _PREFIX[FORMS[form]["tower"]] + ".resblocks."
    if not key.startswith(p):
        return None, key
    l, rest = key[len(p):].split(".", 1)
    return int(l), rest


@functools.lru_cache(maxsize=None)
def cases(form):
    """Every tensor of the form's tower, every tensor of every layer, in_proj_weight by thirds, in_proj_bias by its Q and V thirds."""
    out = [Case(k, None) for k in _TOWER_KEYS[FORMS[form]["tower"]]]
    for l in range(n_layers(form)):
        for rest in _LAYER_KEYS:
            parts = (0, 1, 2) if rest == "attn.in_proj_weight" else (0, 2) if rest == "attn.in_proj_bias" else (None,)
            out += [Case(_layer_key(form, l, rest), part) for part in parts]
    return tuple(out)


def case_id(form, case):
    l, rest = _split_key(form, case.key)
    return (rest if l is None else f"L{l}.{rest}") + ("" if case.part is None else "." + "qkv"[case.part])


def _get(sd, key, part):
    t = sd[key]
    if part is None:
        return t
    n = t.shape[0] // 3
    return t[part * n:(part + 1) * n]


def _with(sd, key, part, value):
    """A copy of the dict (the tensors shared) with (key, part) set to value"""
    out = dict(sd)
    if part is None:
        out[key] = value
    else:
        t = sd[key].clone()
        n = t.shape[0] // 3
        t[part * n:(part + 1) * n] = value
        out[key] = t
    return out


def loud_sd(form, case):
    base = base_sd(form)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(zlib.crc32(f"{LOUD_SEED}/{FORMS[form]['arch']}/{case.key}/{case.part}".encode()))
    return _with(base, case.key, case.part, loud(case.key, _get(base, case.key, case.part), gen, loudness(case)))


def faults(form, case):
    """[(name, state dict)]: what a tower with one wiring fault would compute the case's embedding from.
    stale: the tensor keeps its base value (dropped, or read from a place the packer did not write).
    layerJ: layer l reads the same-named tensor of layer j.
    sibling: out_proj.bias <-> c_proj.bias, ln_1 <-> ln_2, ln_pre <-> ln_post exchanged; rot1 / rot2: the Q / K / V thirds rotated."""
    base, ld = base_sd(form), loud_sd(form, case)
    out = [("stale", base)]
    l, rest = _split_key(form, case.key)
    if l is not None:
        for j in range(n_layers(form)):
            if j != l:
                kj = _layer_key(form, j, rest)
                out.append((f"layer{j}", _with(ld, case.key, case.part, _get(base, kj, case.part))))
    sib = _SIBLINGS.get(rest)
    if sib is not None:
        ks = sib if l is None else _layer_key(form, l, sib)
        swapped = dict(ld)
        swapped[case.key], swapped[ks] = ld[ks], ld[case.key]
        out.append(("sibling", swapped))
    if case.part is not None:
        n = ld[case.key].shape[0] // 3
        out += [(f"rot{r}", _with(ld, case.key, None, torch.roll(ld[case.key], r * n, 0))) for r in (1, 2)]
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compared_inputs(form):
    """The compared rows of the form's input: f32 images [r][3][R][R] or token ids [r][ctx] (SOT, random tokens, EOT = the
    largest id at the form's positions, then zeros)."""
    f, a = FORMS[form], clipmi.weights.ARCHS[FORMS[form]["arch"]]
    g = torch.Generator(device="cpu")
    g.manual_seed(INPUT_SEED)
    if f["tower"] == "vision":
        return torch.randn(len(f["rows"]), 3, a["res"], a["res"], generator=g)
    ids = torch.zeros(len(f["eot"]), a["ctx"], dtype=torch.int64)
    for r, eot in enumerate(f["eot"]):
        ids[r, 0] = a["vocab"] - 2
        ids[r, 1:eot] = torch.randint(1, a["vocab"] - 2, (eot - 1,), generator=g)
        ids[r, eot] = a["vocab"] - 1
    return ids


def compared_rows(form):
    f = FORMS[form]
    return list(f["rows"]) if f["tower"] == "vision" else list(range(len(f["eot"])))


def full_inputs(form):
    """The device call's whole input: compared_inputs() at their rows, other seeded images around them"""
    f, x = FORMS[form], compared_inputs(form)
    if f["tower"] == "text" or f["n"] == len(f["rows"]):
        return x
    g = torch.Generator(device="cpu")
    g.manual_seed(INPUT_SEED + 1)
    full = torch.randn(f["n"], *x.shape[1:], generator=g)
    full[list(f["rows"])] = x
    return full


# ---- references ----------------------------------------------------------------------------------------------------------
def oracle(form, sd):
    """The fp32 oracle on the dict as the device sees it (GEMM weights rounded to bf16), on the compared rows"""
    fn = clip_oracle.encode_image if FORMS[form]["tower"] == "vision" else clip_oracle.encode_text
    return fn(clipmi.weights.bf16_round_state_dict(sd), compared_inputs(form))


def bf16_rule(form, sd):
    """tests/test_encode_gpu.py's rule on this dict -> (ref, noise, tolerance): the oracle, its own deviation with the
    matrix-product inputs rounded to bf16, and 3 x that + 1e-3"""
    fn = clip_oracle.encode_image if FORMS[form]["tower"] == "vision" else clip_oracle.encode_text
    sdr, x = clipmi.weights.bf16_round_state_dict(sd), compared_inputs(form)
    ref = fn(sdr, x)
    with clip_oracle.act_round(torch.bfloat16):
        emu = fn(sdr, x)
    noise = (emu - ref).abs().max().item()
    return ref, noise, 3 * noise + 1e-3


COS_MIN = 0.9995


def emulate_fp8(form, sd, act="product"):
    """The FP8 tower's emulation on the compared rows: clip_oracle.linear_fp8(act) under act_round(bfloat16)"""
    with clip_oracle.act_round(torch.bfloat16), clip_oracle.linear_fp8(act=act):
        return clip_oracle.encode_image(clipmi.weights.bf16_round_state_dict(sd), compared_inputs(form))


def dist(a, b):
    return (a - b).abs().max().item()
