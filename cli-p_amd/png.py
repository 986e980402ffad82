"""`Image.open(f).convert("RGB")` for PNG files on the device (csrc/png.hip).

The host walks the chunks (png_parse.parse) and lets through 8-bit grey and RGB files that are not interlaced; the device
inflates the IDAT stream (one wave per image), undoes the scanline filters and checks the Adler-32, and leaves Pillow's
bytes in HBM: rows of width*3 RGB bytes per image, the layout `clipmi_resize_crop_rgb8` takes. PNG is lossless, so there is
no tolerance: a file comes back with exactly Pillow's pixels (status 0) or goes back to Pillow - every file the parser
refuses (`Unsupported`) and every file the device reports (1 invalid DEFLATE data, 2 the stream ended early, produced too
little or wants to produce more, 3 a filter byte above 4, 4 the Adler-32 differs), so that Pillow's error handling stays the
reference's.
"""
import numpy as np
import torch

from . import _lib
from .png_parse import Parsed, Unsupported, parse  # noqa: F401

IMAGE = np.dtype([("stream_off", "<i8"), ("raw_off", "<i8"), ("out_off", "<i8"), ("stream_bytes", "<i4"), ("width", "<i4"),
                  ("height", "<i4"), ("channels", "<i4"), ("reserved", "<i4", 2)], align=True)
assert IMAGE.itemsize == 48


def pack(items):
    """Parsed records -> (IMAGE array, streams uint8, out_bytes, total_raw_bytes, max_raw_bytes)"""
    recs = np.zeros(len(items), dtype=IMAGE)
    soff = roff = ooff = 0
    max_raw = 1
    pieces = []
    for k, it in enumerate(items):
        r = recs[k]
        r["stream_off"], r["raw_off"], r["out_off"], r["stream_bytes"] = soff, roff, ooff, len(it.stream)
        r["width"], r["height"], r["channels"] = it.width, it.height, it.channels
        pad = (-len(it.stream)) % 16 + 16
        pieces.append(it.stream)
        pieces.append(b"\0" * pad)
        soff += len(it.stream) + pad
        raw = it.raw_bytes()
        roff += (raw + 15) // 16 * 16
        ooff += (it.width * it.height * 3 + 15) // 16 * 16
        max_raw = max(max_raw, raw)
    return recs, np.frombuffer(b"".join(pieces), np.uint8), ooff, roff, max_raw


def decode_device(items, device, stream=None):
    """Parsed records -> (out uint8 device tensor, records, status int32 device tensor): the RGB rows of image k start at
    records[k]["out_off"]. Asynchronous on torch's current stream of `device`; status is valid once that stream is."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.ClipmiError("png.decode_device needs the HIP path (no CPU fallback)")
    L = _lib.lib()
    recs, streams, out_bytes, total_raw, max_raw = pack(items)
    n = len(items)
    out = torch.empty(max(out_bytes, 16), dtype=torch.uint8, device=device)
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=device)
    if n == 0:
        return out, recs, status
    o_str = (recs.nbytes + 15) // 16 * 16
    host = torch.empty(o_str + streams.nbytes, dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    hv[:recs.nbytes] = recs.view(np.uint8).reshape(-1)
    hv[o_str:] = streams
    dev = host.to(device, non_blocking=True)
    ws_bytes = int(L.clipmi_png_workspace_bytes(n, total_raw))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    base = dev.data_ptr()
    rc = L.clipmi_png_decode_rgb8(base + o_str, base, n, total_raw, max_raw, out.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                  ws_bytes, _lib.stream_ptr(device))
    _lib.check(rc, "clipmi_png_decode_rgb8")
    cur = torch.cuda.current_stream(device)
    dev.record_stream(cur)
    ws.record_stream(cur)
    return out, recs, status


def decode_files(blobs, device):
    """PNG file contents -> list of uint8 [H,W,3] numpy arrays (None where the file is not for the device decoder or the
    device reported it). Synchronises; a convenience for tests and tools - the pipeline keeps the pixels in HBM."""
    items, where = [], []
    for k, b in enumerate(blobs):
        try:
            items.append(parse(b))
            where.append(k)
        except Unsupported:
            pass
    res = [None] * len(blobs)
    if not items:
        return res
    out, recs, status = decode_device(items, device)
    st = status.cpu().numpy()
    host = out.cpu().numpy()
    for t, k in enumerate(where):
        if st[t] == 0:
            r = recs[t]
            h, w, o = int(r["height"]), int(r["width"]), int(r["out_off"])
            res[k] = host[o:o + h * w * 3].reshape(h, w, 3)
    return res
