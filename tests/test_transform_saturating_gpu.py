"""The file-level transform entries on files whose resampled sums leave 0 .. 255 on both sides in both passes
(tests/transform_cases.py corpus(); tests/test_transform_tables.py asserts that condition per file on the CPU restatements, so
nothing here passes vacuously). Every output equals decode_worker.load_uint8 byte for byte, the fused JPEG path equals the
unfused one, every status is 0.

The smooth pictures of the other transform tests never clip (resampling one 400 -> 298 leaves 0 of 14 900 sums outside 0 .. 255),
so until here the clip of jpeg_color_resize_h_kernel's LDS path, of its tap-by-tap path, of the CMYK body and of the layouts
had no test."""
import numpy as np
import pytest

import transform_cases as T
from clipmi import jpeg, png

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def files_of(path, files=None):
    sel = [f for f in (T.corpus() if files is None else files) if f.path == path]
    assert sel, path
    return sel


def check_jpeg(files, n_px, **kw):
    blobs = [f.blob for f in files]
    ref = [T.load_uint8_blob(b, n_px) for b in blobs]
    st = jpeg.stage_transform(blobs, n_px, DEV, **kw)
    fused, fused_status = (t.cpu().numpy() for t in jpeg.run_transform(st, True))
    plain, plain_status = (t.cpu().numpy() for t in jpeg.run_transform(st, False))
    assert fused.shape == (len(files), 3, n_px, n_px)
    assert not fused_status.any() and not plain_status.any(), (fused_status, plain_status)
    for k, f in enumerate(files):
        assert np.array_equal(plain[k], ref[k]), f"unfused != load_uint8: {f.name} ({int((plain[k] != ref[k]).sum())} bytes)"
        assert np.array_equal(fused[k], plain[k]), f"fused != unfused: {f.name} ({int((fused[k] != plain[k]).sum())} bytes)"
        assert np.array_equal(fused[k], ref[k]), f"fused != load_uint8: {f.name}"


def test_jpeg_files_fused_and_unfused():
    """baseline 4:4:4 / 4:2:2 / 4:2:0 and grey, progressive, and the 600-wide file whose window spans two chunks of the fused kernel"""
    files = files_of("jpeg")
    assert len(files) >= 7
    check_jpeg(files, T.N_PX)


def test_jpeg_layouts_fused_and_unfused():
    """luma 1x2, 4x1, 1x4 and RGB-coded files: the fused kernel's other chroma forms and its colour function without the transform"""
    files = files_of("layouts")
    assert len(files) >= 5
    check_jpeg(files, T.N_PX, layouts=True)


def test_jpeg_cmyk_and_ycck():
    """four-component files through clipmi_jpeg_decode_cmyk8 and clipmi_resize_crop_cmyk8 (whatever `fused` says)"""
    files = files_of("cmyk")
    assert len(files) >= 3
    check_jpeg(files, T.N_PX, cmyk=True)


def test_jpeg_outputs_of_more_taps_than_a_chunk():
    """n_px 8 over 1100 x 1200: 553 and 603 taps an output, jp_pixel_clamped's tap-by-tap path of the fused kernel, with sums that clip"""
    check_jpeg(T.big_corpus(), T.BIG_N_PX)


@pytest.mark.parametrize("path", ["png", "interlaced"])
def test_png_files(path):
    """RGB, grey, RGBA and LA files (and an interlaced RGBA one): the 3-byte passes and the premultiplied 4-byte ones"""
    files = files_of(path)
    assert len(files) >= (5 if path == "png" else 1)
    got = png.transform_files([f.blob for f in files], T.N_PX, DEV, interlaced=path == "interlaced")
    for f, g in zip(files, got):
        assert g is not None, f"handed back: {f.name}"
        ref = T.load_uint8_blob(f.blob, T.N_PX)
        assert g.shape == ref.shape and np.array_equal(g, ref), f"{f.name}: {int((g != ref).sum())} bytes differ from load_uint8"
