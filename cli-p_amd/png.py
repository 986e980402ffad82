"""`Image.open(f).convert("RGB")` for PNG files on the device (csrc/png.hip).

The host walks the chunks (png_parse.parse) and lets through 8-bit grey and RGB files that are not interlaced; the device
inflates the IDAT stream (one wave per image), undoes the scanline filters and checks the Adler-32, and leaves Pillow's
bytes in HBM: rows of width*3 RGB bytes per image, the layout `clipmi_resize_crop_rgb8` takes. With `modes=True` alpha,
palette and low-depth files decode too, to the pixels of their own mode (clipmi_png_decode_px8; status 5: a palette index beyond
the palette), and `transform_files` runs the transform of each kind on the device. With `interlaced=True` Adam7
files of the same colour types and depths decode as well, to the layout of the same picture stored without interlace (the record
carries INTERLACE_BIT; the unfilter kernel reconstructs the seven passes one after the other). With `deep=True` RGB files of
depth 16 decode too, and with `modes=True` beside it RGBA and grey + alpha files of depth 16: clipmi_png_decode_px8 reconstructs
the 16-bit scanlines and keeps every sample's high byte, which is what Pillow opens such a file as; the transform is that of
the 8-bit file (16-bit RGB is of kind "rgb": Parsed.px8 says which entry decodes a file). `chunks=True` is the host's business
alone (png_parse.parse(chunks=True)): files with metadata chunks, the same stream. PNG is lossless, so there is
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


PX_BYTES = {"rgb": 3, "alpha": 4, "index": 1}          # bytes per decoded pixel, by Parsed.kind
INTERLACE_BIT = 1 << 16                                # in reserved[0] of a record: the file is Adam7-interlaced (include/clipmi.h)


def reserved_words(px8, ctype, depth, entries, interlace):
    """The two `reserved` words of a record (include/clipmi.h; csrc/png.hip png_format reads them): a file of clipmi_png_decode_px8
    (Parsed.px8) carries colour type << 8 | depth and its palette entries, a file of clipmi_png_decode_rgb8 zeros, and an Adam7
    file of either INTERLACE_BIT in the first word. Scalars, or numpy arrays of one value per file -> int32 [..., 2]."""
    first = np.where(px8, np.asarray(ctype) << 8 | depth, 0) | np.where(np.asarray(interlace) != 0, INTERLACE_BIT, 0)
    return np.stack([first, np.where(px8, entries, 0)], axis=-1).astype(np.int32)


def pack(items):
    """Parsed records -> (IMAGE array, streams uint8, out_bytes, total_raw_bytes, max_raw_bytes). `reserved` says what the file is
    (reserved_words); the scanline sizes of an Adam7 file are those of its passes (Parsed.raw_bytes)."""
    recs = np.zeros(len(items), dtype=IMAGE)
    soff = roff = ooff = 0
    max_raw = 1
    pieces = []
    for k, it in enumerate(items):
        r = recs[k]
        r["stream_off"], r["raw_off"], r["out_off"], r["stream_bytes"] = soff, roff, ooff, len(it.stream)
        r["width"], r["height"], r["channels"] = it.width, it.height, it.channels
        r["reserved"] = reserved_words(it.px8, it.ctype, it.depth, it.n_entries, it.interlace)
        pad = (-len(it.stream)) % 16 + 16
        pieces.append(it.stream)
        pieces.append(b"\0" * pad)
        soff += len(it.stream) + pad
        raw = it.raw_bytes()
        roff += (raw + 15) // 16 * 16
        ooff += (it.width * it.height * PX_BYTES[it.kind] + 15) // 16 * 16
        max_raw = max(max_raw, raw)
    return recs, np.frombuffer(b"".join(pieces), np.uint8), ooff, roff, max_raw


def decode_device(items, device, stream=None):
    """Parsed records, all for one decode entry (Parsed.px8: 8-bit grey / RGB files, or the others) -> (out uint8 device tensor, records, status int32 device tensor): the
    decoded rows of image k (PX_BYTES of its kind per pixel) start at records[k]["out_off"]. Asynchronous on torch's current
    stream of `device`; status is valid once that stream is."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.ClipmiError("png.decode_device needs the HIP path (no CPU fallback)")
    L = _lib.lib()
    px8 = bool(items) and items[0].px8
    if any(it.px8 != px8 for it in items):
        raise ValueError("png.decode_device: 8-bit \"rgb\" files and the other files go to different entries")
    size_of, decode, name = ((L.clipmi_png_px8_workspace_bytes, L.clipmi_png_decode_px8, "clipmi_png_decode_px8") if px8 else
                             (L.clipmi_png_workspace_bytes, L.clipmi_png_decode_rgb8, "clipmi_png_decode_rgb8"))
    recs, streams, out_bytes, total_raw, max_raw = pack(items)
    n = len(items)
    out = torch.empty(max(out_bytes, 16), dtype=torch.uint8, device=device)
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=device)
    if n == 0:
        return out, recs, status
    dev, (_, o_str), _ = _lib.to_device16([recs, streams], device)
    ws_bytes = int(size_of(n, total_raw))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    base = dev.data_ptr()
    rc = decode(base + o_str, base, n, total_raw, max_raw, out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes,
                _lib.stream_ptr(device))
    _lib.check(rc, name)
    cur = torch.cuda.current_stream(device)
    dev.record_stream(cur)
    ws.record_stream(cur)
    return out, recs, status


def _parsed(blobs, modes, interlaced=False, chunks=False, deep=False):
    """-> [(position, Parsed)] of the files the parser lets through, split into the files of clipmi_png_decode_rgb8 and the others"""
    rgb, px8 = [], []
    for k, b in enumerate(blobs):
        try:
            it = parse(b, modes=modes, interlaced=interlaced, chunks=chunks, deep=deep)
        except Unsupported:
            continue
        (px8 if it.px8 else rgb).append((k, it))
    return rgb, px8


def decode_files(blobs, device, modes=False, interlaced=False, chunks=False, deep=False):
    """PNG file contents -> list of uint8 [H,W,3] numpy arrays (None where the file is not for the device decoder or the
    device reported it). modes=True: alpha, palette and low-depth files decode too (png_parse.parse(modes=True)) - files of kind
    "alpha" come back as uint8 [H,W,4], files of kind "index" as (uint8 [H,W], palette uint8 [256,3]). interlaced=True: Adam7
    files of the kinds let through decode too, to the same arrays as the picture stored without interlace. chunks=True: files with
    metadata chunks too (png_parse.parse(chunks=True)). deep=True: 16-bit RGB files too, and with modes RGBA and grey + alpha ones, as
    uint8 [H,W,3] and [H,W,4] of the samples' high bytes.
    Synchronises; a convenience for tests and tools - the pipeline keeps the pixels in HBM."""
    res = [None] * len(blobs)
    for group in _parsed(blobs, modes, interlaced, chunks, deep):
        if not group:
            continue
        out, recs, status = decode_device([it for _, it in group], device)
        st = status.cpu().numpy()
        host = out.cpu().numpy()
        for t, (k, it) in enumerate(group):
            if st[t] == 0:
                h, w, o = it.height, it.width, int(recs[t]["out_off"])
                if it.kind == "index":
                    res[k] = (host[o:o + h * w].reshape(h, w), it.palette)
                else:
                    res[k] = host[o:o + h * w * PX_BYTES[it.kind]].reshape(h, w, PX_BYTES[it.kind])
    return res


def transform_device(items, out_rows, n_px, out, decoded, recs, device):
    """The transform of decoded files on the device: the rows of `decoded` (decode_device's buffer, records `recs`) of the Parsed
    `items`, all of one kind -> out[out_rows[k]] uint8 [3,n_px,n_px], through the entry of that kind: clipmi_resize_crop_rgb8,
    clipmi_resize_crop_rgba8 or clipmi_nearest_crop_p8."""
    from .decode_worker import nearest_plan
    from .resize import NEAREST_JOB, pack_jobs
    L = _lib.lib()
    kind = items[0].kind
    px = PX_BYTES[kind]
    n = len(items)
    if kind == "index":
        jobs = np.zeros(n, dtype=NEAREST_JOB)
        tabs = np.zeros(n * (768 + 8 * n_px), np.uint8)            # per file: palette | column table | row table
        for k, it in enumerate(items):
            plan = nearest_plan(it.width, it.height, n_px)
            o = k * (768 + 8 * n_px)
            tabs[o:o + 768] = it.palette.reshape(-1)
            tabs[o + 768:o + 768 + 8 * n_px].view(np.int32)[:] = np.concatenate([plan["hcoef"], plan["vcoef"]])
            j = jobs[k]
            j["src_off"], j["w"], j["h"], j["out_index"] = int(recs[k]["out_off"]), it.width, it.height, out_rows[k]
            j["pal_off"], j["col_off"], j["row_off"] = o, (o + 768) // 4, (o + 768) // 4 + n_px
        small = np.concatenate([jobs.view(np.uint8).reshape(-1), tabs])
        dsmall = torch.from_numpy(small).to(device)
        rc = L.clipmi_nearest_crop_p8(decoded.data_ptr(), dsmall.data_ptr(), n, dsmall.data_ptr() + jobs.nbytes, n_px, out.data_ptr(),
                                      _lib.stream_ptr(device))
        _lib.check(rc, "clipmi_nearest_crop_p8")
        return
    jobs, coef, _, scratch_bytes, max_rows = pack_jobs([(it.height, it.width) for it in items], n_px, px=px)
    jobs["src_off"], jobs["out_index"] = recs["out_off"][:n], out_rows      # (the decoder's rows; the caller's rows of `out`)
    small = np.concatenate([jobs.view(np.uint8).reshape(-1), coef.view(np.uint8)])
    dsmall = torch.from_numpy(small).to(device)
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=device)
    name = "clipmi_resize_crop_rgba8" if kind == "alpha" else "clipmi_resize_crop_rgb8"
    rc = getattr(L, name)(decoded.data_ptr(), dsmall.data_ptr(), n, max_rows, dsmall.data_ptr() + jobs.nbytes, n_px, out.data_ptr(),
                          scratch.data_ptr(), _lib.stream_ptr(device))
    _lib.check(rc, name)


def transform_files(blobs, n_px, device, interlaced=False, chunks=False, deep=False):
    """PNG file contents -> per file the transform's pixels, uint8 [3,n_px,n_px] as decode_worker.load_uint8 gives them (None
    where the file is not for the device or the device reported it): decode on the device + the transform entry of the file's
    kind, "rgb" included; interlaced=True: Adam7 files too; chunks=True: files with metadata chunks too; deep=True: files of depth 16
    too. Synchronises; a convenience for tests and tools like decode_files."""
    device = torch.device(device)
    res = [None] * len(blobs)
    rgb, px8 = _parsed(blobs, True, interlaced, chunks, deep)
    groups = [rgb] + [[e for e in px8 if e[1].kind == kind] for kind in ("rgb", "alpha", "index")]       # (px8's "rgb": 16-bit RGB)
    out = torch.zeros((max(len(blobs), 1), 3, n_px, n_px), dtype=torch.uint8, device=device)
    keep = []
    for group in groups:
        if not group:
            continue
        items = [it for _, it in group]
        decoded, recs, status = decode_device(items, device)
        transform_device(items, [k for k, _ in group], n_px, out, decoded, recs, device)
        keep.append((group, status))
    host = out.cpu().numpy()
    for group, status in keep:
        st = status.cpu().numpy()
        for t, (k, _) in enumerate(group):
            if st[t] == 0:
                res[k] = host[k]
    return res
