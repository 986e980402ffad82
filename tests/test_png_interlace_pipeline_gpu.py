"""pipeline.encode_files with Adam7-interlaced PNG files on the device (device_png_interlaced=True / CLIPMI_DEVICE_PNG_INTERLACED=1
beside device_png and device_png_modes): the vectors, the ok files and the failed files of the all-Pillow path, bit for bit, and
the files counted where the switches say. Runs in a child process with the product's start order (decode workers before the GPU),
as test_png_pipeline_gpu.py does."""
import os

import numpy as np
import pytest
from PIL import Image

import png_cases
import png_interlace_cases as A
import png_mode_cases as M

pytestmark = pytest.mark.gpu


def _png_interlace_pipeline_worker(tmp):
    """Own process. Interlaced grey, RGB, RGBA, grey + alpha, palette and low-depth files beside files that are not interlaced, an
    interlaced file whose stream is cut, a 16-bit interlaced file (Pillow's) and a JPEG file; each small enough for the pipeline's
    first region size, so that every one takes the device in every run that allows it."""
    import sys
    import warnings
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import torch
    import clipmi
    from clipmi import decode_worker
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(45)
    paths, laced_rgb, laced_modes, rgb_pngs, mode_pngs = [], [], [], [], []

    def put(name, blob):
        p = os.path.join(tmp, name)
        with open(p, "wb") as f:
            f.write(blob)
        paths.append(p)
        return p

    # (colour type, depth, h, w, tRNS, content: samples_for's k - screenshot-like where the file is large, so that it fits)
    for i, (ctype, depth, h, w, t, k) in enumerate([(2, 8, 224, 224, False, 2), (0, 8, 300, 260, False, 2), (2, 8, 90, 70, False, 1),
                                                    (2, 8, 225, 223, False, 2), (0, 8, 37, 500, False, 0)]):
        laced_rgb.append(put(f"a{i:02d}_c{ctype}.png", A.lace_file(rng, ctype, depth, h, w, k, level=(1, 6, 9)[i % 3])))
    for i, (ctype, depth, h, w, t, k) in enumerate([(6, 8, 224, 224, False, 8), (6, 8, 37, 70, False, 0), (4, 8, 225, 223, False, 8),
                                                    (3, 8, 230, 300, True, 5), (3, 4, 300, 260, False, 5), (3, 1, 600, 230, True, 5),
                                                    (0, 1, 240, 320, False, 2), (0, 2, 225, 223, False, 2), (0, 4, 33, 33, False, 1)]):
        laced_modes.append(put(f"b{i:02d}_c{ctype}d{depth}.png", A.lace_file(rng, ctype, depth, h, w, k, with_trns=t, level=(1, 6, 9)[i % 3])))
    for i, (h, w, ch) in enumerate([(224, 224, 3), (300, 260, 1), (90, 70, 3)]):
        rgb_pngs.append(put(f"c{i:02d}.png", png_cases.write(png_cases.screenshot(rng, h, w, ch), "cycle", level=(1, 6, 9)[i % 3])))
    for i, (ctype, depth, h, w, t, k) in enumerate([(6, 8, 224, 224, False, 8), (3, 4, 224, 224, True, 5), (0, 2, 225, 223, False, 2)]):
        mode_pngs.append(put(f"d{i:02d}_c{ctype}d{depth}.png", M.mode_file(rng, ctype, depth, h, w, k, "cycle", with_trns=t)))
    s = png_cases.screenshot(rng, 240, 320, 3)
    z = png_cases.deflate(A.scanlines(s, 2, 8))
    cut = put("e_cut_interlaced.png", png_cases.assemble(320, 240, 3, z[:len(z) * 2 // 3], lace=1))       # the stream ends early: status 2
    raw16 = b"".join(r for _, r, _ in A.pass_pieces(rng.integers(0, 256, (30, 40, 2), dtype=np.uint8), 4, 8))   # 16-bit grey: 2 bytes a pixel
    put("e_16bit_interlaced.png", png_cases.assemble(40, 30, 1, png_cases.deflate(raw16), depth=16, ctype=0, lace=1))
    bad = put("g_broken.png", b"broken")
    Image.fromarray(png_cases.smooth(rng, 250, 350)).save(os.path.join(tmp, "h0.jpg"), quality=85)
    paths.append(os.path.join(tmp, "h0.jpg"))
    files = paths[9:] + paths[:9]
    scratch = np.zeros(4 << 20, np.uint8)
    for p in laced_rgb + laced_modes + [cut] + rgb_pngs + mode_pngs:
        assert 0 < decode_worker.stage_png(p, 224, scratch, modes=True, interlaced=True)[2] <= 65536, p      # fits the first region size
        assert (Image.open(p).info.get("interlace") == 1) == (p not in rgb_pngs + mode_pngs)
    for name in ("CLIPMI_DEVICE_PNG", "CLIPMI_DEVICE_PNG_MODES", "CLIPMI_DEVICE_PNG_INTERLACED"):
        os.environ.pop(name, None)
    with clipmi.pipeline.DecodePool(3) as pool:
        assert not torch.cuda.is_initialized()
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        kw = dict(batch=8, pool=pool, device_resize_mb=0, device_jpeg_kb=2048)
        st_pil, st_off, st_on, st_rgb, st_alone, st_env = {}, {}, {}, {}, {}, {}
        pil = list(clipmi.pipeline.encode_files(model, files, stats=st_pil, device_png=False, **kw))
        off = list(clipmi.pipeline.encode_files(model, files, stats=st_off, device_png=True, device_png_modes=True, **kw))
        on = list(clipmi.pipeline.encode_files(model, files, stats=st_on, device_png=True, device_png_modes=True, device_png_interlaced=True, **kw))
        rgb = list(clipmi.pipeline.encode_files(model, files, stats=st_rgb, device_png=True, device_png_interlaced=True, **kw))
        alone = list(clipmi.pipeline.encode_files(model, files, stats=st_alone, device_png=False, device_png_modes=True,
                                                  device_png_interlaced=True, **kw))
        os.environ.update(CLIPMI_DEVICE_PNG="1", CLIPMI_DEVICE_PNG_MODES="1", CLIPMI_DEVICE_PNG_INTERLACED="1")
        env = list(clipmi.pipeline.encode_files(model, files, stats=st_env, **kw))
    for other in (off, on, rgb, alone, env):
        assert [h[0] for h in pil] == [d[0] for d in other] and [h[2] for h in pil] == [d[2] for d in other]
        for h, d in zip(pil, other):
            assert (h[1] is None and d[1] is None) or np.array_equal(h[1], d[1])
    failed = [p for h in pil for p in h[2]]
    assert bad in failed and cut in failed, failed
    n_laced = len(laced_rgb) + len(laced_modes)
    assert st_on["png_interlaced_files"] == st_env["png_interlaced_files"] == n_laced, (st_on, st_env)
    assert st_rgb["png_interlaced_files"] == len(laced_rgb), st_rgb      # without device_png_modes: the grey and RGB ones only
    for st in (st_pil, st_off, st_alone):                     # the switch off, or on without device_png: none
        assert st.get("png_interlaced_files", 0) == 0, st
    assert st_off["png_interlaced_files"] == 0                # (the key is there with the switch off)
    for st in (st_off, st_on, st_rgb, st_env):                # the files that are not interlaced count as before
        assert st["png_files"] == len(rgb_pngs), st
    for st in (st_off, st_on, st_env):
        assert st["png_mode_files"] == len(mode_pngs), st
    assert st_rgb.get("png_mode_files", 0) == 0 and st_pil.get("png_files", 0) == 0 and st_alone.get("png_files", 0) == 0
    for st in (st_off, st_on, st_rgb, st_alone, st_env):
        assert st["jpeg_files"] == st_pil["jpeg_files"] == 1
    open(os.path.join(tmp, "ok"), "w").write("1")


def test_pipeline_interlaced_png_on_device_gives_the_same_vectors(tmp_path):
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r}); " \
           f"import test_png_interlace_pipeline_gpu as t; t._png_interlace_pipeline_worker({str(tmp_path)!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "ok").read_text() == "1"
