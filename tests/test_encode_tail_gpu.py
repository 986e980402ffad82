"""-m gpu: the vision tower's last block on the class-token rows only (encode.hip, "the pruned tail").

encode_image reads one row per image behind the last block, and everything behind that block's attention is row-wise, so the
tail runs on B rows instead of B * L. Because a row's bits depend neither on the batch size nor on the kernel that computes
it, the change is held to BIT-IDENTICAL embeddings - no tolerance anywhere in this file:

1. pruned == unpruned: tests/encode_tail_child.py in child processes of the development library with CLIPMI_ENCODE_TAIL=2
   (the tail at every batch size) and =0 (the last block over all rows), and of the product library (its own rule), must
   write the same f32 bits for every case: the LN-folded ViT-B/32 fixtures at B in {1, 7, 129, 435, 870, 1025}, uint8 and f32
   pixels, with and without normalize; the stand-alone-LayerNorm towers; ViT-B/16 (flash attention). Each child shows the path
   its library took by the number of launches the measurement probe stamps (12 c_fc launches per pass without the tail, 11 with).
2. clipmi_encode_image_workspace_bytes is sufficient: a workspace of exactly that size, poisoned guards on both sides.
3. bench.py's measurement probe still brackets persistent-kernel launches of one shape: 11 per pass at B = 870.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clip_case  # noqa: E402
import encode_tail_child  # noqa: E402

pytestmark = pytest.mark.gpu

CASE_KEYS = [f"{name}/B{B}/{tag}/n{nrm}" for name, _, _, sizes in encode_tail_child.CASES for B in sizes
             for tag in ("u8", "f32") for nrm in (0, 1)]


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    """The three children, one after the other: {"tail2" | "tail0" | "product": {key: f32 array}}."""
    d = tmp_path_factory.mktemp("encode_tail")
    base = {k: v for k, v in os.environ.items() if k not in ("CLIPMI_DEV_LIB", "CLIPMI_ENCODE_TAIL", "CLIPMI_LN_FOLD")}
    envs = {"tail2": dict(base, CLIPMI_DEV_LIB="1", CLIPMI_ENCODE_TAIL="2"),
            "tail0": dict(base, CLIPMI_DEV_LIB="1", CLIPMI_ENCODE_TAIL="0"),
            "product": base}
    out = {}
    for name, env in envs.items():
        path = os.path.join(str(d), name + ".npz")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "encode_tail_child.py"), path], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"{name}: {r.stdout[-1000:]}\n{r.stderr[-3000:]}"
        want = ("lib=product tail=default" if name == "product" else f"lib=dev tail={name[-1]}")
        assert want in r.stdout, (name, r.stdout)
        with np.load(path) as z:
            out[name] = {k: z[k] for k in z.files}
        assert sorted(out[name]) == sorted(CASE_KEYS + ["probe_launches"]), name
        # the knob was honoured: the full last block is a 12th stamped c_fc launch per pass
        per_pass = 12 if name == "tail0" else 11
        assert int(out[name]["probe_launches"][0]) == per_pass * encode_tail_child.PROBE_REPS, (name, out[name]["probe_launches"])
    return out


@pytest.mark.parametrize("case", [c[0] for c in encode_tail_child.CASES])
def test_pruned_tail_equals_the_full_last_block_bitwise(runs, case):
    keys = [k for k in CASE_KEYS if k.startswith(case + "/")]
    assert keys
    for k in keys:
        full = runs["tail0"][k]
        B = int(k.split("/")[1][1:])
        assert full.dtype == np.float32 and full.shape[0] == B and np.isfinite(full).all(), k
        for other in ("tail2", "product"):
            got = runs[other][k]
            assert got.shape == full.shape, (k, other)
            bad = (got.view(np.uint32) != full.view(np.uint32)).any(axis=1)
            assert not bad.any(), f"{k}: {other} differs from the unpruned block in {int(bad.sum())} of {B} rows, first {np.flatnonzero(bad)[:10].tolist()}"
    # the cases are not vacuous: different images give different embeddings
    big = runs["tail0"][keys[-1]]
    assert big.shape[0] == 1 or not np.array_equal(big[0], big[-1])


@pytest.fixture(scope="module")
def b32(clipmi, gpu):
    model = clipmi.CLIP(clip_case.state_dict("vitb32_realstats"), device=gpu)
    g = torch.Generator(device="cpu")
    g.manual_seed(50)
    pool = torch.randint(0, 256, (870, 3, 224, 224), generator=g, dtype=torch.uint8).to(gpu)
    return model, pool


@pytest.mark.parametrize("B", [1, 435, 870])
def test_workspace_bytes_is_sufficient(clipmi, gpu, b32, B):
    """clipmi_encode_image with a workspace of exactly clipmi_encode_image_workspace_bytes, carved out of a poisoned buffer:
    the guards in front of and behind it stay intact and the embeddings are encode_image's own."""
    model, pool = b32
    L = clipmi._lib.lib()
    need = int(L.clipmi_encode_image_workspace_bytes(model.vision, B))
    assert need > 0
    guard = 1 << 20
    buf = torch.full((guard + need + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    x = pool[:B]
    want = {n: model.encode_image(x, normalize=bool(n)) for n in (0, 1)}
    for normalize in (0, 1):
        out = torch.full((B + 1, model.embed_dim), float("nan"), device=gpu)
        rc = L.clipmi_encode_image(model.vision, model._vblob.data_ptr(), x.data_ptr(), clipmi._lib.U8, B, out.data_ptr(),
                                   normalize, buf.data_ptr() + guard, need, clipmi._lib.stream_ptr(gpu))
        clipmi._lib.check(rc, "clipmi_encode_image")
        torch.cuda.synchronize(gpu)
        assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + need:] == 0xA5).all()), f"B={B}: wrote outside the workspace"
        assert torch.isnan(out[B]).all(), "wrote past row B of the output"
        assert torch.equal(out[:B].view(torch.int32), want[normalize].view(torch.int32)), f"B={B} normalize={normalize}"
    rc = L.clipmi_encode_image(model.vision, model._vblob.data_ptr(), x.data_ptr(), clipmi._lib.U8, B, out.data_ptr(), 0,
                               buf.data_ptr() + guard, need - 1, clipmi._lib.stream_ptr(gpu))
    assert rc != 0 and "workspace" in clipmi._lib.last_error()


def test_probe_brackets_eleven_persistent_launches_per_pass(clipmi, gpu, b32):
    """clipmi_dbg_encode_image_probe3_ms (bench.py --full) at B = 870: the tail's GEMMs and the pruned block's attention carry
    no stamps, so c_fc, c_proj (K = 3072) and out_proj (K = 768) are each 11 launches of the persistent kernel per pass and
    every estimator, completion-to-completion included, is an average over launches of one shape."""
    model, pool = b32
    L = clipmi._lib.lib()
    B, reps = 870, 2
    need = int(L.clipmi_encode_image_workspace_bytes(model.vision, B))
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    out = torch.empty((B, model.embed_dim), dtype=torch.float32, device=gpu)
    times = {}
    for epi, want_epi in ((1, 6), (2 | (3072 << 8), 7), (2 | (768 << 8), 7)):
        ms3, nl, kind, kepi = (C.c_float * 3)(), C.c_int(0), C.c_int(-1), C.c_int(-1)
        rc = L.clipmi_dbg_encode_image_probe3_ms(model.vision, model._vblob.data_ptr(), pool.data_ptr(), clipmi._lib.U8, B,
                                                 out.data_ptr(), ws.data_ptr(), ws.numel(), clipmi._lib.stream_ptr(gpu), epi, reps,
                                                 ms3, C.byref(nl), C.byref(kind), C.byref(kepi))
        assert rc == 0, clipmi._lib.last_error()
        assert kind.value == 2 and kepi.value == want_epi, (epi, kind.value, kepi.value)
        assert nl.value == 11 * reps, (epi, nl.value)
        assert all(v > 0 for v in ms3), (epi, list(ms3))
        times[epi] = [round(float(v), 4) for v in ms3]
    print(f"probe3 at B=870 (ms per launch: begin-end, event-in-front, completion-to-completion): {times}")
    torch.cuda.synchronize(gpu)
    got = out.clone()
    assert torch.equal(got, model.encode_image(pool, normalize=True))      # the probed passes computed the real thing
