"""Child process of tests/test_encode_tail_gpu.py: encode the test's cases with whatever library and knobs the environment
selects (CLIPMI_DEV_LIB / CLIPMI_ENCODE_TAIL are read once per process) and write every embedding into one .npz.

    python tests/encode_tail_child.py OUT.npz

Cases (key = "<case>/B<B>/<u8|f32>/<n0|n1>"): the LN-folded ViT-B/32 towers `vitb32_realstats` and `vitb32_outlier` at
B in {1, 7, 129, 435, 870, 1025}; the same geometry with stand-alone LayerNorm passes (CLIPMI_LN_FOLD=0, the f32 residual) and
the width-128 toy with 101 tokens (never folded, flash attention) at smaller B; LN-folded ViT-B/16 (197 tokens, flash
attention) at B in {1, 3, 7}. Inputs come from seeded CPU generators, so every child sees the same pixels.

The child also proves which path its library took: "probe_launches" = the number of c_fc launches that
clipmi_dbg_encode_image_probe3_ms stamped in PROBE_REPS passes at B = 870 (12 per pass when the last block runs over all rows, 11
with the tail, whose launches carry no stamp).
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import clipmi  # noqa: E402
import clip_case  # noqa: E402

B_FOLDED = (1, 7, 129, 435, 870, 1025)
PROBE_REPS = 2
CASES = (
    # name, state dict, CLIPMI_LN_FOLD the tower is packed with, batch sizes
    ("vitb32_realstats", lambda: clip_case.state_dict("vitb32_realstats"), "1", B_FOLDED),
    ("vitb32_outlier", lambda: clip_case.state_dict("vitb32_outlier"), "1", B_FOLDED),
    ("vitb32_nofold", lambda: clip_case.state_dict("vitb32_seed0"), "0", (1, 7, 129, 435)),
    ("toy_l14", lambda: clipmi.weights.random_state_dict("toy-l14", seed=3), "0", (1, 7, 129, 300)),
    ("vitb16", lambda: clipmi.weights.random_state_dict("ViT-B/16", seed=2), "1", (1, 3, 7)),
)


def pixels(n, res, seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randint(0, 256, (n, 3, res, res), generator=g, dtype=torch.uint8)


def main():
    out_path = sys.argv[1]
    dev = torch.device("cuda:0")
    mean = torch.tensor(clipmi.model.CLIP_MEAN, device=dev).reshape(1, 3, 1, 1)
    std = torch.tensor(clipmi.model.CLIP_STD, device=dev).reshape(1, 3, 1, 1)
    out = {}
    for k, (name, make_sd, fold, sizes) in enumerate(CASES):
        os.environ["CLIPMI_LN_FOLD"] = fold                  # read by weights.py when the tower is packed
        model = clipmi.CLIP(make_sd(), device=dev)
        assert model.vision.ln_fold == (1 if fold == "1" and model.dims["v_width"] % 256 == 0 else 0), name
        pool = pixels(max(sizes), model.dims["res"], 40 + k).to(dev)
        for B in sizes:
            u8 = pool[max(sizes) - B:]
            f32 = (u8.float() / 255.0 - mean) / std
            for tag, x in (("u8", u8), ("f32", f32)):
                for nrm in (0, 1):
                    out[f"{name}/B{B}/{tag}/n{nrm}"] = model.encode_image(x, normalize=bool(nrm)).cpu().numpy()
        if name == "vitb32_realstats":
            L = clipmi._lib.lib()
            B = 870
            ws = torch.empty(int(L.clipmi_encode_image_workspace_bytes(model.vision, B)), dtype=torch.uint8, device=dev)
            eout = torch.empty((B, model.embed_dim), dtype=torch.float32, device=dev)
            ms3, nl, kind, kepi = (C.c_float * 3)(), C.c_int(0), C.c_int(-1), C.c_int(-1)
            x = pool[max(sizes) - B:].contiguous()
            clipmi._lib.check(L.clipmi_dbg_encode_image_probe3_ms(model.vision, model._vblob.data_ptr(), x.data_ptr(), clipmi._lib.U8, B,
                                                                  eout.data_ptr(), ws.data_ptr(), ws.numel(), clipmi._lib.stream_ptr(dev),
                                                                  1, PROBE_REPS, ms3, C.byref(nl), C.byref(kind), C.byref(kepi)),
                              "encode_image_probe3")
            torch.cuda.synchronize(dev)
            out["probe_launches"] = np.array([nl.value], dtype=np.int64)
        del model, pool
    np.savez(out_path, **out)
    print(f"lib={'dev' if clipmi._lib.DEV_LIB else 'product'} tail={os.environ.get('CLIPMI_ENCODE_TAIL', 'default')} "
          f"arrays={len(out)} c_fc_launches_per_pass={int(out['probe_launches'][0]) / PROBE_REPS:g}", flush=True)


if __name__ == "__main__":
    main()
