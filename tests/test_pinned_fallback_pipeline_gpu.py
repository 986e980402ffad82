"""pipeline.encode_files when the pool's shared-memory segments cannot be page-locked (a locked-memory limit): a batch whose files
sit in regions of the big segment then travels through a pinned copy of the segment (device_stage.DeviceStage.run), the batches
decoded after it take the host path, and the n_px x n_px slots go through the pinned staging ring. The vectors, the good files and
the failed files have to be the host path's, in that call and in the next one on the same pool, which starts with regions again.
Runs in a child process with the product's start order (decode workers before the GPU)."""
import os

import numpy as np
import pytest
from PIL import Image

import png_cases
from test_jpeg import smooth

pytestmark = pytest.mark.gpu


def _fallback_worker(tmp):
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import torch
    import clipmi
    rng = np.random.default_rng(53)

    def put_img(name, img, **kw):
        p = os.path.join(tmp, name)
        img.save(p, **kw)
        return p

    sizes = [(240, 320), (200, 150), (225, 223), (230, 300), (120, 310)]              # (h, w), none above 320 x 240
    base = [put_img(f"base{k}.jpg", Image.fromarray(smooth(rng, h, w)), quality=80 + k, subsampling=k % 3) for k, (h, w) in enumerate(sizes)]
    prog = [put_img(f"prog{k}.jpg", Image.fromarray(smooth(rng, h, w)), quality=75 + k, subsampling=k % 3, progressive=True)
            for k, (h, w) in enumerate(sizes)]
    pngs = [put_img(f"png{k}.png", Image.fromarray(png_cases.screenshot(rng, h, w, 3))) for k, (h, w) in enumerate(sizes)]
    bmp = put_img("full.bmp", Image.fromarray(smooth(rng, 230, 310)))
    files = [f for trio in zip(base, prog, pngs) for f in trio]
    files.insert(3, bmp)                                                              # formats alternate within each batch of 8
    assert len(files) == 16 and Image.open(bmp).mode == "RGB" and all(Image.open(p).size[0] <= 320 and Image.open(p).size[1] <= 240 for p in files)
    import warnings
    warnings.simplefilter("ignore")
    with clipmi.pipeline.DecodePool(3) as pool:
        assert not torch.cuda.is_initialized()
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        host = list(clipmi.pipeline.encode_files(model, files, batch=8, pool=pool, device_resize_mb=0, device_jpeg_kb=0))
        asked = []

        def refuse(which):
            asked.append(which)
            return False

        pool.pin_segment = refuse
        kw = dict(batch=8, pool=pool, device_resize_mb=8, device_jpeg_kb=2048, device_progressive=True, device_png=True)
        st = {}
        first = list(clipmi.pipeline.encode_files(model, files, stats=st, **kw))
        second = list(clipmi.pipeline.encode_files(model, files, **kw))
    assert [len(h[0]) for h in host] == [8, 8] and not any(h[2] for h in host)
    assert any(which >= 2 for which in asked), asked            # a big segment was refused: the fallback ran
    assert st["jpeg_files"] + st["jpeg_progressive_files"] + st["png_files"] > 0, st
    for other in (first, second):
        assert [h[0] for h in host] == [d[0] for d in other] and [h[2] for h in host] == [d[2] for d in other]
        for h, d in zip(host, other):
            assert np.array_equal(h[1], d[1])
    open(os.path.join(tmp, "ok"), "w").write("1")


def test_unpinnable_segments_give_the_host_paths_vectors_twice(tmp_path):
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r}); " \
           f"import test_pinned_fallback_pipeline_gpu as t; t._fallback_worker({str(tmp_path)!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "ok").read_text() == "1"
