"""pipeline.encode_files with PNG files that carry metadata chunks and PNG files of depth 16 on the device (device_png_chunks=True /
CLIPMI_DEVICE_PNG_CHUNKS=1 and device_png_deep=True / CLIPMI_DEVICE_PNG_DEEP=1 beside device_png): the vectors, the ok files and
the failed files of the all-Pillow path, bit for bit, and the files counted where the switches say. Runs in a child process with
the product's start order (decode workers before the GPU), as test_png_modes_pipeline_gpu.py does."""
import os

import numpy as np
import pytest
from PIL import Image

import png_cases
import png_deep_cases as D
import png_mode_cases as M

pytestmark = pytest.mark.gpu


def _png_deep_pipeline_worker(tmp):
    """Own process. 8-bit files with and without metadata, 16-bit files of all four colour types (grey 16 stays with Pillow), an
    interlaced 16-bit file, a file with a 2 MiB profile and one with iCCP method 1 (Pillow fails both), a cut 16-bit file and a JPEG
    file; each small enough for the pipeline's first region size, so that every one takes the device in every run that allows it."""
    import sys
    import warnings
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import torch
    import clipmi
    from clipmi import decode_worker
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(330)
    paths, rgb_pngs, mode_pngs, chunk_rgb, chunk_modes, deep_rgb, deep_modes, deep_laced, both = [], [], [], [], [], [], [], [], []

    def put(name, blob):
        p = os.path.join(tmp, name)
        with open(p, "wb") as f:
            f.write(blob)
        paths.append(p)
        return p

    meta = dict(D.valid_chunks())
    for i, (h, w, ch) in enumerate([(224, 224, 3), (300, 260, 1), (90, 70, 3)]):
        rgb_pngs.append(put(f"a{i:02d}.png", png_cases.write(png_cases.screenshot(rng, h, w, ch), "cycle", level=(1, 6, 9)[i % 3])))
    for i, (ctype, depth, h, w, t, k) in enumerate([(6, 8, 224, 224, False, 8), (3, 4, 224, 224, True, 5), (0, 2, 225, 223, False, 2)]):
        mode_pngs.append(put(f"b{i:02d}_c{ctype}d{depth}.png", M.mode_file(rng, ctype, depth, h, w, k, "cycle", with_trns=t)))
    for i, (h, w, ch, name) in enumerate([(224, 224, 3, "screenshot"), (260, 300, 3, "iCCP"), (70, 90, 1, "zTXt"), (225, 223, 3, "iTXt_compressed")]):
        chunk_rgb.append(put(f"c{i:02d}_{name}.png", png_cases.write(png_cases.screenshot(rng, h, w, ch), "cycle", before=meta[name])))
    s = png_cases.screenshot(rng, 224, 224, 3)
    z = png_cases.deflate(png_cases.filter_rows(s, png_cases.filters_for("cycle1", 224)))
    chunk_rgb.append(put("c10_behind.png", png_cases.assemble(224, 224, 3, z, before=D.C(b"tRNS", b"\0\1\0\2\0\3"), after=meta["eXIf"] + meta["iTXt_plain"])))
    chunk_modes.append(put("d00_rgba_icc.png", M.mode_file(rng, 6, 8, 224, 224, 8, "cycle", before=meta["iCCP"])))
    chunk_modes.append(put("d01_p4_idot.png", M.mode_file(rng, 3, 4, 230, 300, 5, "cycle", before=meta["iDOT"])))
    for i, (h, w, k) in enumerate([(80, 90, 2), (60, 70, 1), (37, 100, 0)]):      # (the low bytes are noise: small files, so that they fit)
        deep_rgb.append(put(f"e{i:02d}_rgb16.png", D.deep_file(rng, 2, h, w, k, level=(1, 6, 9)[i % 3])))
    for i, (ctype, h, w, k) in enumerate([(6, 70, 80, 2), (4, 150, 60, 2), (6, 37, 70, 0), (4, 70, 37, 1)]):
        deep_modes.append(put(f"f{i:02d}_c{ctype}d16.png", D.deep_file(rng, ctype, h, w, k)))
    deep_laced.append(put("g00_rgb16_interlaced.png", D.deep_file(rng, 2, 90, 70, 1, lace=1)))
    both.append(put("g01_rgb16_icc_trns.png", D.deep_file(rng, 2, 80, 90, 2, before=meta["iCCP"] + D.C(b"tRNS", b"\0\1\0\2\0\3"))))
    grey16 = put("h00_grey16.png", png_cases.assemble(40, 30, 1, png_cases.deflate(png_cases.filter_rows(png_cases.noise(rng, 30, 40, 2), [1] * 30)),
                                                      depth=16, ctype=0))
    small = png_cases.smooth(rng, 40, 50, 3)
    fails = dict((n, c) for n, c, _ in D.failing_chunks())
    big_icc = put("i00_icc_2mib.png", png_cases.write(small, "cycle", before=fails["iCCP_2MiB"]))
    icc_m1 = put("i01_icc_method1.png", png_cases.write(small, "cycle", before=fails["iCCP_method_1"]))
    s16 = D.samples16(rng, 2, 80, 90, 2)
    z16 = png_cases.deflate(D.scanlines16(s16))
    cut = put("i02_cut16.png", png_cases.assemble(90, 80, 3, z16[:len(z16) * 2 // 3], depth=16, ctype=2))       # the stream ends early: status 2
    bad = put("j_broken.png", b"broken")
    Image.fromarray(png_cases.smooth(rng, 250, 350)).save(os.path.join(tmp, "k0.jpg"), quality=85)
    paths.append(os.path.join(tmp, "k0.jpg"))
    files = paths[11:] + paths[:11]
    scratch = np.zeros(4 << 20, np.uint8)
    new = chunk_rgb + chunk_modes + deep_rgb + deep_modes + deep_laced + both
    for p in rgb_pngs + mode_pngs + new + [cut]:
        assert 0 < decode_worker.stage_png(p, 224, scratch, modes=True, interlaced=True, chunks=True, deep=True)[2] <= 65536, p      # fits the first region size
    for p in new + [cut, grey16, big_icc, icc_m1]:            # none of them is a file for the device without the new switches
        with pytest.raises(decode_worker.png_parse.Unsupported):
            decode_worker.stage_png(p, 224, scratch, modes=True, interlaced=True)
    assert Image.open(grey16).mode == "I;16"
    for name in ("CLIPMI_DEVICE_PNG", "CLIPMI_DEVICE_PNG_MODES", "CLIPMI_DEVICE_PNG_INTERLACED", "CLIPMI_DEVICE_PNG_CHUNKS", "CLIPMI_DEVICE_PNG_DEEP"):
        os.environ.pop(name, None)
    with clipmi.pipeline.DecodePool(3) as pool:
        assert not torch.cuda.is_initialized()
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        kw = dict(batch=8, pool=pool, device_resize_mb=0, device_jpeg_kb=2048, jpeg_group_mb=1)
        base = dict(device_png=True, device_png_modes=True, device_png_interlaced=True)
        st_pil, st_off, st_on, st_chunks, st_deep, st_rgb, st_alone, st_env = ({} for _ in range(8))
        pil = list(clipmi.pipeline.encode_files(model, files, stats=st_pil, device_png=False, **kw))
        off = list(clipmi.pipeline.encode_files(model, files, stats=st_off, **base, **kw))
        on = list(clipmi.pipeline.encode_files(model, files, stats=st_on, device_png_chunks=True, device_png_deep=True, **base, **kw))
        chunks = list(clipmi.pipeline.encode_files(model, files, stats=st_chunks, device_png_chunks=True, **base, **kw))
        deep = list(clipmi.pipeline.encode_files(model, files, stats=st_deep, device_png_deep=True, **base, **kw))
        rgb = list(clipmi.pipeline.encode_files(model, files, stats=st_rgb, device_png=True, device_png_chunks=True, device_png_deep=True, **kw))
        alone = list(clipmi.pipeline.encode_files(model, files, stats=st_alone, device_png=False, device_png_chunks=True, device_png_deep=True, **kw))
        os.environ.update(CLIPMI_DEVICE_PNG="1", CLIPMI_DEVICE_PNG_MODES="1", CLIPMI_DEVICE_PNG_INTERLACED="1", CLIPMI_DEVICE_PNG_CHUNKS="1",
                          CLIPMI_DEVICE_PNG_DEEP="1")
        env = list(clipmi.pipeline.encode_files(model, files, stats=st_env, **kw))
    for other in (off, on, chunks, deep, rgb, alone, env):
        assert [h[0] for h in pil] == [d[0] for d in other] and [h[2] for h in pil] == [d[2] for d in other]
        for h, d in zip(pil, other):
            assert (h[1] is None and d[1] is None) or np.array_equal(h[1], d[1])
    failed = sorted(p for h in pil for p in h[2])
    assert failed == sorted([bad, cut, big_icc, icc_m1]), failed
    # each key counts the files its switch added and the device kept
    n_chunks, n_deep = len(chunk_rgb) + len(chunk_modes), len(deep_rgb) + len(deep_modes) + len(deep_laced)
    for st in (st_on, st_env):
        assert (st["png_chunk_files"], st["png_deep_files"]) == (n_chunks, n_deep + len(both)), st
    assert (st_chunks["png_chunk_files"], st_chunks["png_deep_files"]) == (n_chunks, 0), st_chunks
    assert (st_deep["png_chunk_files"], st_deep["png_deep_files"]) == (0, n_deep), st_deep
    # without device_png_modes and device_png_interlaced: the grey and RGB ones that are not interlaced
    assert (st_rgb["png_chunk_files"], st_rgb["png_deep_files"]) == (len(chunk_rgb), len(deep_rgb) + len(both)), st_rgb
    assert (st_off["png_chunk_files"], st_off["png_deep_files"]) == (0, 0)          # (the keys are there with the switches off)
    for st in (st_pil, st_alone):                             # on without device_png: none
        assert st.get("png_chunk_files", 0) == 0 and st.get("png_deep_files", 0) == 0, st
    for st in (st_off, st_on, st_chunks, st_deep, st_rgb, st_env):      # the old files count as before
        assert st["png_files"] == len(rgb_pngs) and st["png_interlaced_files"] == 0, st
    for st in (st_off, st_on, st_chunks, st_deep, st_env):
        assert st["png_mode_files"] == len(mode_pngs), st
    assert st_rgb.get("png_mode_files", 0) == 0 and st_pil.get("png_files", 0) == 0 and st_alone.get("png_files", 0) == 0
    for st in (st_off, st_on, st_chunks, st_deep, st_rgb, st_alone, st_env):
        assert st["jpeg_files"] == st_pil["jpeg_files"] == 1
    open(os.path.join(tmp, "ok"), "w").write("1")


def test_pipeline_png_chunks_and_deep_on_device_give_the_same_vectors(tmp_path):
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r}); " \
           f"import test_png_deep_pipeline_gpu as t; t._png_deep_pipeline_worker({str(tmp_path)!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "ok").read_text() == "1"
