"""pipeline.encode_files with the PNG decode on the device (device_png=True / CLIPMI_DEVICE_PNG=1): the vectors, the ok files and
the failed files of the all-Pillow path, bit for bit. Runs in a child process with the product's start order (decode workers
before the GPU), as the JPEG pipeline tests do."""
import os
import zlib

import numpy as np
import pytest
from PIL import Image

import png_cases

pytestmark = pytest.mark.gpu


def adam7(img):
    """a valid interlaced file (Pillow's encoder writes none): the seven passes' scanlines with filter None"""
    h, w, ch = img.shape
    raw = b""
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = img[y0::dy, x0::dx]
        if sub.size:
            raw += b"".join(b"\0" + row.tobytes() for row in sub)
    return png_cases.assemble(w, h, ch, zlib.compress(raw), lace=1)


def _png_pipeline_worker(tmp):
    """Own process. RGB and grey PNG files of several sizes (each small enough for the pipeline's first region size, so that every
    one of them takes the device in every run) beside RGBA, palette, interlaced and 16-bit files, two PNG files whose data is cut, a file
    that is no image, and two JPEG files."""
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import torch
    import clipmi
    from clipmi import decode_worker
    rng = np.random.default_rng(43)
    paths, device_pngs = [], []

    def put(name, blob):
        p = os.path.join(tmp, name)
        with open(p, "wb") as f:
            f.write(blob)
        paths.append(p)
        return p

    def put_img(name, img, **kw):
        p = os.path.join(tmp, name)
        img.save(p, **kw)
        paths.append(p)
        return p

    for i, (h, w, ch, gen) in enumerate([(224, 224, 3, png_cases.screenshot), (480, 640, 3, png_cases.screenshot), (90, 70, 3, png_cases.smooth),
                                         (300, 260, 1, png_cases.screenshot), (225, 223, 3, png_cases.screenshot), (60, 100, 1, png_cases.smooth),
                                         (600, 230, 3, png_cases.screenshot), (224, 500, 1, png_cases.screenshot)]):
        a = gen(rng, h, w, ch)
        if i % 2:
            device_pngs.append(put(f"a{i:02d}.png", png_cases.write(a, "cycle", level=(1, 6, 9)[i % 3])))
        else:
            device_pngs.append(put_img(f"a{i:02d}.png", Image.fromarray(a[..., 0] if ch == 1 else a)))
    rgb = Image.fromarray(png_cases.smooth(rng, 250, 350))
    put_img("b_rgba.png", rgb.convert("RGBA"))
    put_img("c_palette.png", rgb.convert("P"))
    put("d_interlaced.png", adam7(png_cases.smooth(rng, 230, 240)))
    put_img("e_16bit.png", Image.fromarray(rng.integers(0, 65536, (230, 240)).astype(np.uint16)))
    a = png_cases.screenshot(rng, 240, 320, 3)
    z = png_cases.deflate(png_cases.filter_rows(a, png_cases.filters_for("cycle", 240)))
    cut = put("f_cut.png", png_cases.assemble(320, 240, 3, z[:len(z) * 2 // 3]))     # the stream ends early: the device reports it
    blob = png_cases.write(a, "cycle")
    cut_file = put("f_cut_file.png", blob[:len(blob) * 2 // 3])                      # the file ends early: the parser refuses it
    behind = put("f_srgb_behind.png", png_cases.assemble(320, 240, 3, z, after=png_cases.chunk(b"sRGB", b"")))   # intact image data, but
    bad = put("g_broken.png", b"broken")                                      # Pillow refuses the empty sRGB behind it: the parser must too
    put_img("h0.jpg", rgb, quality=85)
    put_img("h1.jpg", Image.fromarray(png_cases.smooth(rng, 240, 320)), quality=90, subsampling=0)
    files = paths[3:] + paths[:3]
    scratch = np.zeros(4 << 20, np.uint8)
    for p in device_pngs + [cut]:
        assert 0 < decode_worker.stage_png(p, 224, scratch)[2] <= 65536, p      # fits the first region size in every run
    assert Image.open([p for p in paths if p.endswith('d_interlaced.png')][0]).info.get("interlace") == 1
    import warnings
    warnings.simplefilter("ignore")
    os.environ.pop("CLIPMI_DEVICE_PNG", None)
    with clipmi.pipeline.DecodePool(3) as pool:
        assert not torch.cuda.is_initialized()
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        kw = dict(batch=6, pool=pool, device_resize_mb=0, device_jpeg_kb=2048)
        st_off, st_unset, st_on, st_grp = {}, {}, {}, {}
        off = list(clipmi.pipeline.encode_files(model, files, stats=st_off, device_png=False, **kw))
        unset = list(clipmi.pipeline.encode_files(model, files, stats=st_unset, **kw))
        on = list(clipmi.pipeline.encode_files(model, files, stats=st_on, device_png=True, **kw))
        grp = list(clipmi.pipeline.encode_files(model, files, stats=st_grp, device_png=True, jpeg_group_mb=1, **kw))
    for other in (unset, on, grp):
        assert [h[0] for h in off] == [d[0] for d in other] and [h[2] for h in off] == [d[2] for d in other]
        for h, d in zip(off, other):
            assert (h[1] is None and d[1] is None) or np.array_equal(h[1], d[1])
    failed = [p for h in off for p in h[2]]
    assert sorted(failed) == sorted([bad, cut, cut_file, behind]), failed
    assert st_off.get("png_files", 0) == 0 and st_unset.get("png_files", 0) == 0
    assert st_on["png_files"] == len(device_pngs) and st_grp["png_files"] == len(device_pngs), (st_on, st_grp)
    for st in (st_on, st_grp, st_unset):
        assert st["jpeg_files"] == st_off["jpeg_files"] == 2
    open(os.path.join(tmp, "ok"), "w").write("1")


def test_pipeline_png_on_device_gives_the_same_vectors(tmp_path):
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r}); " \
           f"import test_png_pipeline_gpu as t; t._png_pipeline_worker({str(tmp_path)!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "ok").read_text() == "1"
