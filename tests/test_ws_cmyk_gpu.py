"""-m gpu: clipmi_jpeg_decode_cmyk8 and clipmi_resize_crop_cmyk8 give the same statuses and the same pixels whatever their workspace,
their scratch rows, their outputs and their status tensor held on entry (tests/ws_cases.py: the harness; tests/test_ws_decode_gpu.py
does the same for the other decode and transform entries).

csrc/jpeg.hip, clipmi_jpeg_decode_cmyk8 (jpeg_baseline_planes over clipmi_jpeg_image4 records): luts, coef and planes are established
as for clipmi_jpeg_decode_rgb8 - jpeg_build_luts_kernel whole; zero_async, then jpeg_huffman_kernel and jpeg_dc_kernel; jpeg_idct_kernel
every block of an image's MCU grid, the fourth component's plane included. status_dev[i]: jpeg_huffman_kernel stores on every path
out. out_dev: jpeg_cmyk_kernel writes W H 4 bytes of each image. csrc/resize.hip, clipmi_resize_crop_cmyk8: no Arena; the scratch rows
of a job are written by the first pass before the second reads them; out block out_index whole."""
import numpy as np
import pytest
import torch

import jpeg_cmyk as jc
import ws_cases as W

pytestmark = pytest.mark.gpu
N_PX = 64


def _files():
    """Three small files: 2x2 CMYK with restart intervals, 1x1 YCCK that keeps its byte stuffing, 2x1 without an Adobe marker"""
    rng = np.random.default_rng(571)
    return [(jc.cmyk_file(jc.smooth4(rng, 70, 90), subsampling=2, restart_marker_blocks=4), {}),
            (jc.as_ycck(jc.cmyk_file(jc.smooth4(rng, 64, 61), subsampling=0, quality=95)), dict(keep_stuffing=True)),
            (jc.without_adobe(jc.cmyk_file(jc.smooth4(rng, 100, 64), subsampling=1)), {})]


def test_decode_cmyk8(clipmi, gpu):
    J, lib, L = clipmi.jpeg, clipmi._lib, clipmi._lib.lib()
    files = _files()
    items = [clipmi.jpeg_parse.parse(b, cmyk=True, **kw) for b, kw in files]
    assert items[0].ri and items[1].stuffed == 1 and {it.transform for it in items} == {2, 3}
    recs, tables, streams, out_bytes, blocks, max_blocks, max_pixels = J.pack(items, cmyk=True)
    ws_bytes = int(L.clipmi_jpeg_workspace_bytes(blocks, len(tables)))
    dev, offs, host = lib.to_device16([recs, tables, streams], gpu)
    base, n = dev.data_ptr(), len(items)

    def call(ws, pixels, status):
        dev.copy_(host, non_blocking=True)                  # (the entry rewrites the records and unstuffs the segment in place)
        lib.check(L.clipmi_jpeg_decode_cmyk8(base + offs[2], base, n, base + offs[1], len(tables), blocks, max_blocks, max_pixels,
                                             pixels.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes, lib.stream_ptr(gpu)),
                  "clipmi_jpeg_decode_cmyk8")

    def canon(d):                                           # the padding between the images' rows is not written
        keep = np.zeros(d["pixels"].size, bool)
        for r in recs:
            keep[int(r["out_off"]):int(r["out_off"]) + int(r["width"]) * int(r["height"]) * 4] = True
        d["pixels"][~keep] = 0
        return d
    got = W.run_independent(call, [("pixels", max(out_bytes, 16)), ("status", 4 * n)], ws_bytes, device=gpu, canon=canon)
    assert got["status"].view(np.int32).tolist() == [0] * n
    for r, (b, _) in zip(recs, files):
        h, w, o = int(r["height"]), int(r["width"]), int(r["out_off"])
        assert np.array_equal(got["pixels"][o:o + h * w * 4].reshape(h, w, 4), jc.pillow4(b))


def test_resize_crop_cmyk8(clipmi, gpu, tmp_path):
    """The scratch rows between the passes are the workspace. Down- and upscaling, and neither axis resampled (the crop-only path)"""
    lib, L = clipmi._lib, clipmi._lib.lib()
    rng = np.random.default_rng(572)
    blobs = [b for b, _ in _files()] + [jc.cmyk_file(jc.smooth4(rng, 64, 64), subsampling=2), jc.as_ycck(jc.cmyk_file(jc.smooth4(rng, 37, 70), subsampling=0))]
    imgs = [jc.pillow4(b) for b in blobs]
    jobs, coef, raw_bytes, scratch_bytes, max_rows = clipmi.resize.pack_jobs([a.shape[:2] for a in imgs], N_PX, px=4)
    assert {(int(j["need_h"]), int(j["need_v"])) for j in jobs} >= {(0, 0), (1, 1)}
    src = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in imgs])).to(gpu)
    small = torch.from_numpy(np.concatenate([jobs.view(np.uint8).reshape(-1), coef.view(np.uint8)])).to(gpu)
    n, block = len(imgs), 3 * N_PX * N_PX

    def call(ws, pixels):
        lib.check(L.clipmi_resize_crop_cmyk8(src.data_ptr(), small.data_ptr(), n, max_rows, small.data_ptr() + jobs.nbytes, N_PX,
                                             pixels.data_ptr(), ws.data_ptr(), lib.stream_ptr(gpu)), "clipmi_resize_crop_cmyk8")
    got = W.run_independent(call, [("pixels", n * block)], scratch_bytes, device=gpu)
    for k, b in enumerate(blobs):
        path = tmp_path / f"{k}.jpg"
        path.write_bytes(b)
        assert np.array_equal(got["pixels"][k * block:(k + 1) * block].reshape(3, N_PX, N_PX), clipmi.decode_worker.load_uint8(str(path), N_PX)), k
