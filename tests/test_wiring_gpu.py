"""-m gpu: every weight tensor of every layer reaches the embeddings, in every block form of csrc/encode.hip.

One tensor loud at a time (tests/wiring_cases.py): the device tower runs on the form's seeded state dict with exactly one
tensor - or one Q / K / V third of in_proj_* - replaced by a loud version, and is held to the reference on the same dict.

bf16 forms: tests/test_encode_gpu.py's own rule, evaluated on the loud dict - err <= 3 x the oracle's bf16-emulation noise
+ 1e-3 and row cosine >= 0.9995. No new tolerance: tests/test_wiring.py proves on the CPU that a tower which drops the
tensor, keeps a stale one, takes it from or gives it to another layer, exchanges it with its sibling or rotates the thirds
misses that rule by at least 7 tolerances.
FP8 forms: the fp32-oracle tolerance is too wide there, so a nearest-candidate rule without a constant - the device output
must be nearer (max-abs over the compared rows) to the product emulation of the loud dict than to the emulation of every
dict of faults(case); tests/test_wiring.py proves those emulations at least 3 yardsticks apart.

Every test asserts that its tower is in the form it is named for (tower.ln_fold, tower.weight_format and the plan's own
answers: entry 22 of clipmi_dbg_gemm_plan / clipmi_dbg_gemm_fp8_plan), prints err / tolerance (FP8: the two distances), and
the module prints each form's worst figure when it is done."""
import ctypes as C

import pytest
import torch

import wiring_cases as wc

pytestmark = pytest.mark.gpu

N_OUT = 23
EPI_QGELU, EPI_RESID_LN = 1, 7          # EPI_BIAS_QGELU_BF16, EPI_BIAS_RESID_LN_F32 (csrc/gemm.hpp)

_INPUTS = {}            # form -> the device call's input (images on the device, token ids on the host)
_WORST = {}             # form -> (figure, text)


def _params(forms):
    return [pytest.param(f, c, id=f"{f}-{wc.case_id(f, c)}") for f in forms for c in wc.cases(f)]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for form, (_, text) in _WORST.items():
        print(f"wiring worst of {form}: {text}")


def _writes_leaves(lib, M, N, K):
    out = (C.c_int32 * N_OUT)()
    lib.clipmi_dbg_gemm_plan(M, N, K, EPI_RESID_LN, 0, 1, 0, 0, out, N_OUT)
    return bool(out[22])


def _emits_mx(lib, M, N, K):
    out = (C.c_int32 * N_OUT)()
    lib.clipmi_dbg_gemm_fp8_plan(M, N, K, EPI_QGELU, 1, 0, 0, out, N_OUT)
    return bool(out[22])


def _assert_form(clipmi, tower, form, B):
    f, lib = wc.FORMS[form], clipmi._lib.lib()
    W, M = tower.width, B * tower.tokens
    assert tower.ln_fold == f["fold"] and tower.weight_format == int(f["fp8"]), (form, tower.ln_fold, tower.weight_format)
    if "leaves" in f:          # blocks_ln: the residual GEMMs hand the statistics on as leaves, or as partials
        assert (_writes_leaves(lib, M, W, W) and _writes_leaves(lib, M, W, 4 * W)) == f["leaves"], (form, M)
    if "tail_leaves" in f:     # tail_ln over the B class-token rows
        assert (_writes_leaves(lib, B, W, W) and _writes_leaves(lib, B, W, 4 * W)) == f["tail_leaves"], (form, B)
    if f["fp8"]:               # blocks_fp8: c_fc on the persistent kernel that emits the MX rows itself, or not
        assert _emits_mx(lib, M, 4 * W, W) == f["persistent"], (form, M)


def _device_rows(clipmi, gpu, form, sd):
    """The device tower on the form's input -> the compared rows, on the host"""
    f = wc.FORMS[form]
    if form not in _INPUTS:
        x = wc.full_inputs(form)
        _INPUTS[form] = x.to(gpu) if f["tower"] == "vision" else x      # host ids: EOT at the last position, nothing trimmed
    x = _INPUTS[form]
    model = clipmi.CLIP(sd, device=gpu, vision_weights="fp8" if f["fp8"] else "bf16")
    if f["tower"] == "vision":
        _assert_form(clipmi, model.vision, form, x.shape[0])
        got = model.encode_image(x)
    else:
        _assert_form(clipmi, model.text, form, x.shape[0])
        got = model.encode_text(x)
    assert got.shape[0] == x.shape[0]
    return got[wc.compared_rows(form)].cpu()


def _record(form, figure, text):
    if form not in _WORST or figure > _WORST[form][0]:
        _WORST[form] = (figure, text)


@pytest.mark.parametrize("form,case", _params(wc.BF16_FORMS))
def test_loud_tensor_reaches_the_embedding(clipmi, gpu, form, case):
    sd = wc.loud_sd(form, case)
    got = _device_rows(clipmi, gpu, form, sd)
    ref, noise, tol = wc.bf16_rule(form, sd)
    err = wc.dist(got, ref)
    cos = torch.nn.functional.cosine_similarity(got.double(), ref.double(), dim=-1).min().item()
    text = f"{wc.case_id(form, case)}: err {err:.4g} / tolerance {tol:.4g} = {err / tol:.3f} (bf16-emulation noise {noise:.4g}), min cosine {cos:.6f}"
    print(f"{form} {text}")
    _record(form, err / tol, text)
    assert torch.isfinite(got).all()
    assert err <= tol, f"{form} {text}"
    assert cos >= wc.COS_MIN, f"{form} {text}"


@pytest.mark.parametrize("form,case", _params(wc.FP8_FORMS))
def test_loud_tensor_reaches_the_fp8_embedding(clipmi, gpu, form, case):
    sd = wc.loud_sd(form, case)
    got = _device_rows(clipmi, gpu, form, sd)
    right = wc.dist(got, wc.emulate_fp8(form, sd))
    wrong, name = min((wc.dist(got, wc.emulate_fp8(form, bad)), name) for name, bad in wc.faults(form, case))
    text = f"{wc.case_id(form, case)}: {right:.4g} from the emulation of the loud dict, {wrong:.4g} from the nearest wrong one ({name}): ratio {right / wrong:.3f}"
    print(f"{form} {text}")
    _record(form, right / wrong, text)
    assert torch.isfinite(got).all()
    assert right < wrong, f"{form} {text}"
