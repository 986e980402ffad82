"""pipeline.encode_files with alpha, palette and low-depth PNG files on the device (device_png=True, device_png_modes=True /
CLIPMI_DEVICE_PNG_MODES=1): the vectors, the ok files and the failed files of the all-Pillow path, bit for bit. Runs in a child
process with the product's start order (decode workers before the GPU), as test_png_pipeline_gpu.py does."""
import os

import numpy as np
import pytest
from PIL import Image

import png_cases
import png_mode_cases as M

pytestmark = pytest.mark.gpu


def adam7(img, ctype):
    """a valid interlaced file (Pillow's encoder writes none): the seven passes' scanlines with filter None"""
    import zlib
    h, w, ch = img.shape
    raw = b""
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = img[y0::dy, x0::dx]
        if sub.size:
            raw += b"".join(b"\0" + row.tobytes() for row in sub)
    return png_cases.assemble(w, h, ch, zlib.compress(raw), ctype=ctype, lace=1)


def _png_modes_pipeline_worker(tmp):
    """Own process. Grey and RGB PNG files mixed with RGBA, grey + alpha, palette files with and without tRNS, 1-bit and low-depth
    grey files (each small enough for the pipeline's first region size, so that every one of them takes the device in every run
    that allows it), an interlaced RGBA file, 16-bit files, a palette file with an index beyond its palette, a cut stream, a
    broken file and two JPEG files."""
    import sys
    import warnings
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import torch
    import clipmi
    from clipmi import decode_worker
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(44)
    paths, rgb_pngs, mode_pngs = [], [], []

    def put(name, blob):
        p = os.path.join(tmp, name)
        with open(p, "wb") as f:
            f.write(blob)
        paths.append(p)
        return p

    for i, (h, w, ch) in enumerate([(224, 224, 3), (300, 260, 1), (90, 70, 3), (225, 223, 3), (224, 500, 1)]):
        rgb_pngs.append(put(f"a{i:02d}.png", png_cases.write(png_cases.screenshot(rng, h, w, ch), "cycle", level=(1, 6, 9)[i % 3])))
    # (colour type, depth, h, w, tRNS, content: png_mode_cases.samples_for's k - screenshot-like with a binary alpha plane where the
    # file is large, so that it fits the first region size; noise and smooth alpha at the small sizes)
    specs = [(6, 8, 224, 224, False, 8), (6, 8, 300, 260, False, 8), (6, 8, 37, 70, False, 0), (6, 8, 70, 37, False, 4), (4, 8, 225, 223, False, 8),
             (4, 8, 224, 500, False, 8), (4, 8, 33, 33, False, 1), (3, 8, 480, 640, False, 5), (3, 8, 230, 600, True, 5), (3, 4, 300, 260, True, 5),
             (3, 4, 224, 224, False, 5), (3, 2, 70, 37, False, 0), (3, 1, 600, 230, True, 5), (0, 1, 240, 320, False, 2), (0, 2, 225, 223, False, 2),
             (0, 4, 33, 33, False, 1), (6, 8, 500, 224, False, 8)]
    for i, (ctype, depth, h, w, t, k) in enumerate(specs):
        blob = M.mode_file(rng, ctype, depth, h, w, k, "cycle", with_trns=t, level=(1, 6, 9)[i % 3])
        mode_pngs.append(put(f"m{i:02d}_c{ctype}d{depth}.png", blob))
    for i, what in enumerate(("RGBA", "LA", "P4t", "P8", "1")):                    # Pillow's own encoder
        mode_pngs.append(put(f"n{i}_{what}.png", M.pillow_mode_file(rng, what, 100, 140, 5)))
    put("d_interlaced_rgba.png", adam7(M.samples_for(rng, 6, 8, 230, 240, 1)[0], 6))
    laced = put("d_interlaced.png", adam7(png_cases.smooth(rng, 230, 240), 2))
    put("e_16bit.png", M.save(Image.fromarray(rng.integers(0, 65536, (230, 240)).astype(np.uint16))))
    put("e_16bit_rgba.png", png_cases.assemble(40, 30, 4, png_cases.deflate(b"".join(b"\0" + bytes(rng.integers(0, 256, 320, dtype=np.uint8)) for _ in range(30))),
                                               depth=16, ctype=6))
    pal = rng.integers(0, 256, (5, 3), dtype=np.uint8)
    idx = rng.integers(0, 5, (224, 224, 1), dtype=np.uint8)
    idx[100, 100, 0] = 9
    beyond = put("f_beyond_palette.png", M.write(idx, 3, 4, "cycle", palette=pal))      # the device reports it (status 5): Pillow's to judge
    s, _ = M.samples_for(rng, 6, 8, 240, 320, 8)
    z = png_cases.deflate(M.scanlines(s, 6, 8, "cycle"))
    cut = put("f_cut_rgba.png", png_cases.assemble(320, 240, 4, z[:len(z) * 2 // 3], depth=8, ctype=6))      # the stream ends early: status 2
    bad = put("g_broken.png", b"broken")
    rgb = Image.fromarray(png_cases.smooth(rng, 250, 350))
    for name, kw in (("h0.jpg", dict(quality=85)), ("h1.jpg", dict(quality=90, subsampling=0))):
        rgb.save(os.path.join(tmp, name), **kw)
        paths.append(os.path.join(tmp, name))
    files = paths[7:] + paths[:7]
    scratch = np.zeros(4 << 20, np.uint8)
    for p in rgb_pngs:
        assert 0 < decode_worker.stage_png(p, 224, scratch)[2] <= 65536, p      # fits the first region size in every run
    for p in mode_pngs + [cut, beyond]:
        assert 0 < decode_worker.stage_png(p, 224, scratch, modes=True)[2] <= 65536, p
    assert Image.open(laced).info.get("interlace") == 1
    os.environ.pop("CLIPMI_DEVICE_PNG", None)
    os.environ.pop("CLIPMI_DEVICE_PNG_MODES", None)
    with clipmi.pipeline.DecodePool(3) as pool:
        assert not torch.cuda.is_initialized()
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        kw = dict(batch=8, pool=pool, device_resize_mb=0, device_jpeg_kb=2048)
        st_off, st_png, st_on, st_grp, st_alone = {}, {}, {}, {}, {}
        off = list(clipmi.pipeline.encode_files(model, files, stats=st_off, device_png=False, **kw))
        only = list(clipmi.pipeline.encode_files(model, files, stats=st_png, device_png=True, **kw))
        on = list(clipmi.pipeline.encode_files(model, files, stats=st_on, device_png=True, device_png_modes=True, **kw))
        grp = list(clipmi.pipeline.encode_files(model, files, stats=st_grp, device_png=True, device_png_modes=True, jpeg_group_mb=1, **kw))
        alone = list(clipmi.pipeline.encode_files(model, files, stats=st_alone, device_png=False, device_png_modes=True, **kw))
    for other in (only, on, grp, alone):
        assert [h[0] for h in off] == [d[0] for d in other] and [h[2] for h in off] == [d[2] for d in other]
        for h, d in zip(off, other):
            assert (h[1] is None and d[1] is None) or np.array_equal(h[1], d[1])
    failed = [p for h in off for p in h[2]]
    assert bad in failed and cut in failed, failed
    # (f_beyond_palette.png: Pillow's behaviour for it is version-dependent - whatever it is, all runs agree)
    for st in (st_off, st_png, st_alone):                     # the flag off, or on without device_png: nothing of the new kinds
        assert st.get("png_mode_files", 0) == 0, st
    assert st_off.get("png_files", 0) == 0 and st_alone.get("png_files", 0) == 0
    for st in (st_png, st_on, st_grp):
        assert st["png_files"] == len(rgb_pngs), st
    assert st_on["png_mode_files"] == len(mode_pngs) and st_grp["png_mode_files"] == len(mode_pngs), (st_on, st_grp, len(mode_pngs))
    for st in (st_png, st_on, st_grp, st_alone):
        assert st["jpeg_files"] == st_off["jpeg_files"] == 2
    open(os.path.join(tmp, "ok"), "w").write("1")


def test_pipeline_png_modes_on_device_give_the_same_vectors(tmp_path):
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r}); " \
           f"import test_png_modes_pipeline_gpu as t; t._png_modes_pipeline_worker({str(tmp_path)!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "ok").read_text() == "1"
