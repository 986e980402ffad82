"""-m gpu: the plan is what runs. A ViT-B/32 tower at the smallest batches that reach the 128 x 128, the 256 x 256 and the
persistent kernel; the measurement probe (clipmi_dbg_encode_image_probe3_ms, one pass) reports which kernel and epilogue each of
the four block GEMMs was launched with, and that must be what clipmi_dbg_gemm_plan (csrc/gemm_plan.hpp) says for the shape.

Two packings of the same weights: the product's LN-folded tower and the one with stand-alone LayerNorm passes (CLIPMI_LN_FOLD=0
when the tower is packed, as tests/encode_tail_child.py does). The second is there because the probe cannot report every GEMM
of the first: a folded tower's residual GEMM that is not on the persistent kernel runs as an EPI_F32 launch into the scratch
rows, which the probe files under epilogue 3 and the entry point's filter for the residual epilogue (2) then passes over ("no
launch matched", as before this file existed). Those cases - the plan says `scratch` - are asked of the unfolded tower alone,
where out_proj and c_proj carry the plain residual epilogue at every batch size; every other case is asked of both."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clip_case  # noqa: E402
from test_gemm_plan import K128, K256, K256P, plan  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def b32(clipmi, gpu):
    models, saved = {}, os.environ.get("CLIPMI_LN_FOLD")
    try:
        for fold in ("1", "0"):
            os.environ["CLIPMI_LN_FOLD"] = fold                  # read by weights.py when the tower is packed
            models[fold] = clipmi.CLIP(clip_case.state_dict("vitb32_realstats"), device=gpu)
            assert models[fold].vision.ln_fold == int(fold)
    finally:
        os.environ.pop("CLIPMI_LN_FOLD") if saved is None else os.environ.__setitem__("CLIPMI_LN_FOLD", saved)
    g = torch.Generator(device="cpu")
    g.manual_seed(51)
    return models, torch.randint(0, 256, (435, 3, 224, 224), generator=g, dtype=torch.uint8).to(gpu)


@pytest.mark.parametrize("fold", ["1", "0"])
@pytest.mark.parametrize("B,reaches", [(3, K128), (82, K256), (435, K256P)])
def test_probe_reports_the_planned_kernel(clipmi, gpu, b32, B, reaches, fold):
    model, pool = b32[0][fold], b32[1]
    L = clipmi._lib.lib()
    W, M = 768, B * 50
    folded = fold == "1"
    need = int(L.clipmi_encode_image_workspace_bytes(model.vision, B))
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    out = torch.empty((B, model.embed_dim), dtype=torch.float32, device=gpu)
    seen = set()
    # (probe_epi, the GEMM's N, K, its epilogue): qkv, c_fc, out_proj and c_proj (the K filter tells the last two apart)
    for probe_epi, N, K, epi in ((0, 3 * W, W, 5 if folded else 0), (1, 4 * W, W, 6 if folded else 1),
                                 (2 | (W << 8), W, W, 7 if folded else 2), (2 | (4 * W << 8), W, 4 * W, 7 if folded else 2)):
        err, parts = plan(M, N, K, epi)
        assert err == 0 and len(parts) == 1, (B, N, K, epi, parts)               # no split GEMM at these batch sizes
        if parts[0][3]:
            assert folded and epi == 7        # the scratch detour, which the probe cannot report: see above
            continue
        ms3, nl, kind, ran = (C.c_float * 3)(), C.c_int(0), C.c_int(-1), C.c_int(-1)
        rc = L.clipmi_dbg_encode_image_probe3_ms(model.vision, model._vblob.data_ptr(), pool.data_ptr(), clipmi._lib.U8, B,
                                                 out.data_ptr(), ws.data_ptr(), ws.numel(), clipmi._lib.stream_ptr(gpu), probe_epi, 1,
                                                 ms3, C.byref(nl), C.byref(kind), C.byref(ran))
        assert rc == 0, clipmi._lib.last_error()
        assert (kind.value, ran.value) == (parts[0][1], parts[0][2]), (B, N, K, epi, kind.value, ran.value, parts)
        assert plan(M, N, K, ran.value)[1][0][1] == kind.value                   # and the plan of the epilogue that ran
        assert nl.value >= model.vision.layers - 1
        seen.add(kind.value)
    assert reaches in seen, (B, seen)
