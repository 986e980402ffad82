"""The fused JPEG transform path (clipmi_jpeg_decode_transform_rgb8, pipeline.encode_files(jpeg_fused=...)) as far as it can be
checked without a GPU: the exported symbols and their prototypes, the keyword, the environment switch, and what a file costs a
group of device_stage with and without the full-size RGB rows. tests/test_jpeg_fused_gpu.py has the pixels."""
import ctypes as C
import inspect
import io

import numpy as np
from PIL import Image

from clipmi import decode_worker as dw
from clipmi import device_stage, pipeline

vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
TRANSFORM = [vp, i32, vp, i32, vp, vp]                      # jobs, max_rows, coef, n_px, out, scratch


def test_library_exports_the_transform_entries_with_the_declared_prototypes(clipmi):
    L = clipmi._lib.lib()
    assert {"clipmi_jpeg_decode_transform_rgb8", "clipmi_jpeg_decode_progressive_transform_rgb8"} <= set(clipmi._lib.SYMBOLS)
    base, prog = L.clipmi_jpeg_decode_transform_rgb8, L.clipmi_jpeg_decode_progressive_transform_rgb8
    # the decode entries' arguments with the transform's in place of max_pixels and out_dev
    assert list(L.clipmi_jpeg_decode_rgb8.argtypes) == [vp, vp, i32, vp, i32, i64, i64, i64, vp, vp, vp, i64, vp]
    assert list(base.argtypes) == [vp, vp, i32, vp, i32, i64, i64] + TRANSFORM + [vp, vp, i64, vp]
    assert list(prog.argtypes) == [vp, vp, i32, vp, i32, vp, i32, i64, i64] + TRANSFORM + [vp, vp, i64, vp]
    assert base.restype is i32 and prog.restype is i32
    # argument validation answers without touching the device: nothing to do, then a missing pointer
    assert base(None, None, 0, None, 0, 0, 0, None, 0, None, 224, None, None, None, None, 0, None) == 0
    fake = C.c_void_p(256)
    assert base(fake, fake, 1, fake, 1, 1, 1, None, 1, fake, 224, fake, fake, fake, fake, 1 << 20, None) != 0
    assert "jpeg_decode_transform_rgb8" in clipmi._lib.last_error()
    assert prog(fake, fake, 1, fake, 1, fake, 1, 1, 1, fake, 0, fake, 224, fake, fake, fake, fake, 1 << 20, None) != 0
    assert "jpeg_decode_progressive_transform_rgb8" in clipmi._lib.last_error()


def test_encode_files_has_the_keyword_and_the_switch_is_off_when_unset(monkeypatch):
    p = inspect.signature(pipeline.encode_files).parameters
    assert "jpeg_fused" in p and p["jpeg_fused"].default is None
    monkeypatch.delenv("CLIPMI_DEVICE_JPEG_FUSED", raising=False)
    assert device_stage.jpeg_fused_default() is False
    for value, on in (("", False), ("0", False), ("1", True)):
        monkeypatch.setenv("CLIPMI_DEVICE_JPEG_FUSED", value)
        assert device_stage.jpeg_fused_default() is on
    assert device_stage.formats(False) is device_stage._FORMATS
    fused = device_stage.formats(True)
    assert set(fused) == set(device_stage._FORMATS)
    for kind in device_stage._FORMATS:
        changed = kind in (dw.KIND_BASELINE, dw.KIND_PROGRESSIVE)
        assert (fused[kind] != device_stage._FORMATS[kind]) == changed
        assert (fused[kind][4] is None) == changed            # no transform entry of its own: the decode entry transforms


def test_a_fused_file_needs_its_full_size_rows_less(tmp_path):
    """The header a worker writes for a 2 000 x 1 500 4:2:0 file: with the switch on its `need` is the unfused one minus the
    full-size RGB rows, for the baseline and for the progressive kind; the PNG kinds do not move."""
    w, h, n_px = 2000, 1500, 224
    a = np.zeros((h, w, 3), np.uint8)
    a[::7, ::5] = 200
    rows = (w * h * 3 + 15) // 16 * 16
    for kw, kind, stage in ((dict(), dw.KIND_BASELINE, dw.stage_jpeg), (dict(progressive=True), dw.KIND_PROGRESSIVE, dw.stage_jpeg_progressive)):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=90, subsampling=2, **kw)
        region = np.zeros(4 << 20, np.uint8)
        assert stage(None, n_px, region, data=buf.getvalue())[2] > 0
        hd = region[:4 * dw.JPEG_HDR_INTS].view(np.int32).astype(np.int64)[None, :]
        assert (hd[0, dw.HDR.W], hd[0, dw.HDR.H], hd[0, dw.HDR.HS], hd[0, dw.HDR.VS]) == (w, h, 2, 2)
        off = device_stage.file_need(hd, device_stage.formats(False)[kind], n_px)
        on = device_stage.file_need(hd, device_stage.formats(True)[kind], n_px)
        assert off.shape == (1,) and int(on[0]) == int(off[0]) - rows
        assert int(on[0]) == int(hd[0, dw.HDR.BLOCKS]) * 192 + int(hd[0, dw.HDR.NROWS]) * n_px * 3
    for kind in (dw.KIND_PNG, dw.KIND_PNG_ALPHA, dw.KIND_PNG_INDEX):
        assert device_stage.formats(True)[kind] is device_stage._FORMATS[kind]
