"""-m gpu: include/clipmi.h promises that every entry point "never allocates, frees or synchronises: all work is enqueued on
`stream` and is graph-capturable". Here one call of clipmi_topk_ip, clipmi_topk_ip_coarse_i8 (Q <= 64), clipmi_encode_text (Q = 1,
the REPL's case), clipmi_encode_image (B = 2) and clipmi_jpeg_decode_transform_rgb8 is captured on one non-default stream (a
linear chain: no parallel branches), replayed twice with its input buffers rewritten in place - other queries, other pixels, another
prompt, other files of the same record geometry - and each replay must leave the bytes the eager call leaves for the same inputs.
An eager call comes first: it takes the LDS opt-ins (hipFuncSetAttribute). A capture the runtime refuses is a failure that
carries the library's and HIP's message, never a skip."""
import numpy as np
import pytest
import torch

import jpeg_layouts as jl
import ws_cases as W
from conftest import unit_rows

pytestmark = pytest.mark.gpu


def _capture_and_replay(clipmi, gpu, call, outputs, ws_bytes, set_inputs, consumes_inputs=False):
    """call(ws, *outs): the library call alone (no allocation, no copy). set_inputs: three callables that rewrite the call's input
    buffers in place on the current stream - the first for the eager call and the capture, the others for the two replays.
    consumes_inputs: the entry rewrites its inputs (the baseline JPEG decoder): they are set again in front of every call."""
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        ws, ws2 = (torch.empty(ws_bytes, dtype=torch.uint8, device=gpu) for _ in range(2))
        outs, outs2 = ([torch.empty(nb, dtype=torch.uint8, device=gpu) for _, nb in outputs] for _ in range(2))
        set_inputs[0]()
        call(ws, *outs)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=s):
            call(ws, *outs)
    except Exception as e:                                   # noqa: BLE001 - whatever the runtime or the library raises
        pytest.fail(f"the runtime refused to capture the call: {type(e).__name__}: {e}; library: {clipmi._lib.last_error()!r}")
    seen = []
    for k in (1, 2):
        with torch.cuda.stream(s):
            set_inputs[k]()
            ws.fill_(0xFF)
            for o in outs + outs2:
                o.fill_(0xFF)
            g.replay()
            got = [o.clone() for o in outs]
            if consumes_inputs:
                set_inputs[k]()
            call(ws2, *outs2)
        s.synchronize()
        for (name, _), a, b in zip(outputs, got, outs2):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            bad = np.flatnonzero(a != b)
            assert bad.size == 0, f"replay {k}: output '{name}' differs from the eager call at byte {bad[0]} ({bad.size} bytes)"
        seen.append([x.cpu().numpy() for x in got])
    assert not np.array_equal(seen[0][0], seen[1][0]), "the two replays saw the same inputs"
    return seen


@pytest.mark.parametrize("entry,kind", [("clipmi_topk_ip", None), ("clipmi_topk_ip_coarse_i8", "int8")])
def test_search_is_capturable(clipmi, gpu, entry, kind):
    import test_ws_search_gpu as S
    E, Q, K = 512, 17, 51
    idx = S._index(clipmi, gpu, E, kind=kind)
    rng = np.random.default_rng(61)
    qs = [torch.from_numpy(unit_rows(rng, Q, E)).to(gpu) for _ in range(3)]
    s = S.Search(clipmi, gpu, entry, idx, qs[0].cpu().numpy(), K)
    _capture_and_replay(clipmi, gpu, s, s.outputs, s.ws_bytes, [lambda q=q: s.qd.copy_(q) for q in qs])


def _b32(clipmi, gpu):
    import test_ws_encode_gpu as T
    return T._model(clipmi, gpu, "vitb32")


def test_encode_text_one_prompt_is_capturable(clipmi, gpu):
    model = _b32(clipmi, gpu)
    ids = W.prompts(model, 1)
    tower, ids_dev = W.text_tower(model, ids)
    others = []
    for seed in (1, 2):                                     # other prompts of the same length: the trimmed tower is the captured one
        o = ids.clone()
        g = torch.Generator(device="cpu")
        g.manual_seed(seed)
        o[0, 1:5] = torch.randint(1, model.dims["vocab"] - 2, (4,), generator=g)
        others.append(o[:, :tower.tokens].to(device=gpu, dtype=torch.int32))
    first = ids_dev.clone()
    call, outputs, ws_bytes = W.encode_text_call(clipmi, model, tower, ids_dev)
    _capture_and_replay(clipmi, gpu, call, outputs, ws_bytes, [lambda v=v: ids_dev.copy_(v) for v in [first] + others])


def test_encode_image_two_images_is_capturable(clipmi, gpu):
    import test_ws_encode_gpu as T
    model = _b32(clipmi, gpu)
    px = T._pixels(model, 2)
    variants = [px.clone(), T._pixels(model, 3)[1:], T._pixels(model, 5)[3:]]
    call, outputs, ws_bytes = W.encode_image_call(clipmi, model, px)
    _capture_and_replay(clipmi, gpu, call, outputs, ws_bytes, [lambda v=v: px.copy_(v) for v in variants])


def test_jpeg_decode_transform_is_capturable(clipmi, gpu):
    """Three batches of the same shapes, samplings and tables (Pillow's standard ones) but other pixels: the records, the jobs and
    the counts the call was captured with stay valid, the streams and their lengths in the records change"""
    J, lib, L = clipmi.jpeg, clipmi._lib, clipmi._lib.lib()
    n_px = 224
    shapes = [(200, 320, 2), (123, 77, 0), (96, 128, 1), (65, 130, 2)]
    staged = []
    for seed in (71, 72, 73):
        rng = np.random.default_rng(seed)
        staged.append(J.stage_transform([jl.encode(jl.smooth(rng, h, w), quality=85, subsampling=s) for h, w, s in shapes], n_px, gpu))
    g0 = staged[0].groups[0]
    geometry = lambda g: (g["n"], g["ntables"], g["total_blocks"], g["max_blocks"], g["max_rows"], tuple(g["offs"]))  # noqa: E731
    assert all(len(st.groups) == 1 and geometry(st.groups[0]) == geometry(g0) for st in staged)
    hosts = [st.keep[0] for st in staged]
    dev = torch.empty(max(h.numel() for h in hosts), dtype=torch.uint8, device=gpu)
    n, base, o = g0["n"], dev.data_ptr(), g0["offs"]
    head = (base + o[-1], base, n, base + o[1], g0["ntables"], g0["total_blocks"], g0["max_blocks"], base + o[-3], g0["max_rows"],
            base + o[-2], n_px)
    scratch = torch.empty(g0["scratch"].numel(), dtype=torch.uint8, device=gpu)

    def call(ws, pixels, status):
        lib.check(L.clipmi_jpeg_decode_transform_rgb8(*head, pixels.data_ptr(), scratch.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                                      g0["ws_bytes"], lib.stream_ptr(gpu)), "clipmi_jpeg_decode_transform_rgb8")
    # (the entry rewrites its records and unstuffs its streams in place: an upload goes in front of every call)
    uploads = [lambda h=h: dev[:h.numel()].copy_(h, non_blocking=True) for h in hosts]
    seen = _capture_and_replay(clipmi, gpu, call, [("pixels", n * 3 * n_px * n_px), ("status", 4 * n)], g0["ws_bytes"], uploads,
                               consumes_inputs=True)
    assert all(got[1].view(np.int32).tolist() == [0] * n for got in seen)
