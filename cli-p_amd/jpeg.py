"""`Image.open(tfn)` for baseline JPEG files on the device (reference build-index.py:47).

The host walks the markers (and removes the 0xFF00 byte stuffing, unless it leaves that to the device too); csrc/jpeg.hip does the
rest (Huffman decode in self-synchronising subsequences, DC prediction, jpeg_idct_islow, fancy upsampling, YCbCr -> RGB) and leaves Pillow's
bytes in HBM: rows of width*3 RGB bytes per image, the layout `clipmi_resize_crop_rgb8` takes (resize.py). Files this
parser does not let through (progressive, CMYK / RGB-coded, 12-bit, odd sampling, anything that is not a
JPEG; with `layouts=True` luma 1x2 / 4x1 / 1x4 and RGB-coded files pass) raise `Unsupported` and stay with Pillow in the
decode workers - that is a choice of decoder per file format, made on the host from the file's own header; a file the
device then reports (status != 0: 1 an invalid Huffman code, 2 the data ended early or ran over, 3 a marker inside a segment handed over with its stuffing, 4 a block whose IDCT leaves the range where
libjpeg-turbo's provably equals the device's) goes the same way, so that Pillow's error handling stays the reference's.
`cmyk=True` down the stack (opt-in, encode_files(device_jpeg_cmyk=True)) adds the four-component files jpeg_parse.parse(cmyk=True)
lets through, CMYK as stored and YCCK: their records are IMAGE4 (clipmi_jpeg_image4), clipmi_jpeg_decode_cmyk8 leaves Pillow's
mode-CMYK bytes, rows of width*4, and clipmi_resize_crop_cmyk8 is their transform (Pillow resamples in mode CMYK and converts after).
`transform_files` goes one step further: decode and the CLIP transform's resize + crop in one library call, without the full-size
RGB rows in between (clipmi_jpeg_decode_transform_rgb8, opt-in in the pipeline: encode_files(jpeg_fused=True)).
"""
from functools import partial

import numpy as np
import torch

from . import _lib
from .jpeg_parse import TABLE_BYTES, Parsed, Progressive, Unsupported, is_layout, parse, parse_progressive  # noqa: F401

def _image_dtype(nc):
    """clipmi_jpeg_image (nc = 3) / clipmi_jpeg_image4 (nc = 4): nc table indices of each class, nc rows of quantisation steps"""
    return np.dtype([("stream_off", "<i8"), ("coef_off", "<i8"), ("out_off", "<i8"), ("intervals_off", "<i8"), ("stream_bytes", "<i4"),
                     ("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("hs", "<i4"), ("vs", "<i4"), ("dc_tbl", "<i4", nc),
                     ("ac_tbl", "<i4", nc), ("restart_interval", "<i4"), ("n_intervals", "<i4"), ("stuffed", "<i4"), ("reserved", "<i4"),
                     ("quant", "u1", (nc, 64))], align=True)


IMAGE, IMAGE4 = _image_dtype(3), _image_dtype(4)      # IMAGE4: the record of a four-component file (parse(cmyk=True))
assert IMAGE.itemsize == 288 and IMAGE4.itemsize == 360


def _opted_in(items, layouts, cmyk=False):
    """The records of the layouts that are opt-in (jpeg_parse.parse(layouts=True), parse(cmyk=True)) pass only where the caller
    opted in too; three- and four-component records have different C records and entries, so one call takes one of the two"""
    if not layouts and any(is_layout(it) for it in items):
        raise Unsupported("a record of parse(layouts=True) packed without layouts=True")
    four = [it.ncomp == 4 for it in items]
    if any(four) and not cmyk:
        raise Unsupported("a record of parse(cmyk=True) packed without cmyk=True")
    if any(four) and not all(four):
        raise Unsupported("four-component records and others in one batch")


def pack(items, layouts=False, cmyk=False):
    """Parsed records -> (IMAGE array, tables uint8 [nt][288], streams uint8, out_bytes, total_blocks, max_blocks, max_pixels)
    layouts: the records may be those parse(layouts=True) adds - their sampling factors and colour transform travel in the record
    cmyk: the records may be those parse(cmyk=True) adds, all of them or none: an IMAGE4 array then, the outputs w*h*4 bytes"""
    _opted_in(items, layouts, cmyk)
    px = 4 if items and items[0].ncomp == 4 else 3
    recs = np.zeros(len(items), dtype=IMAGE4 if px == 4 else IMAGE)
    pool = {}
    soff = coff = ooff = 0
    max_blocks = max_pixels = 1
    pieces = []
    for k, it in enumerate(items):
        r = recs[k]
        r["stream_off"], r["coef_off"], r["out_off"], r["stream_bytes"] = soff, coff, ooff, len(it.stream)
        r["width"], r["height"], r["ncomp"], r["hs"], r["vs"] = it.width, it.height, it.ncomp, it.hs, it.vs
        idx = [pool.setdefault(t, len(pool)) for t in it.tables]
        r["dc_tbl"], r["ac_tbl"] = idx[0::2], idx[1::2]
        r["quant"] = it.quant
        r["stuffed"], r["reserved"] = it.stuffed, it.transform      # (reserved: the colour transform, clipmi_jpeg_image)
        pad = (-len(it.stream)) % 16 + 16
        pieces.append(it.stream)
        pieces.append(b"\0" * pad)
        soff += len(it.stream) + pad
        if it.ri:                                            # restart intervals: their byte offsets travel behind the segment
            r["restart_interval"], r["n_intervals"], r["intervals_off"] = it.ri, len(it.starts), soff
            raw = it.starts.astype("<u4").tobytes()
            raw += b"\0" * ((-len(raw)) % 16)
            pieces.append(raw)
            soff += len(raw)
        nb = it.blocks()
        coff += nb
        ooff += (it.width * it.height * px + 15) // 16 * 16
        max_blocks, max_pixels = max(max_blocks, nb), max(max_pixels, it.width * it.height)
    tables = np.frombuffer(b"".join(pool), np.uint8).reshape(-1, TABLE_BYTES) if pool else np.zeros((0, TABLE_BYTES), np.uint8)
    return recs, tables, np.frombuffer(b"".join(pieces), np.uint8), ooff, coff, max_blocks, max_pixels


def _decode_device(items, device, packer, workspace, entry):
    """decode_device's and decode_progressive_device's body. packer: pack or pack_progressive (the arrays in front of the
    streams are the entry's records and tables, in its order); workspace(L, n, total_blocks, ntables) -> bytes; entry: the library call"""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.ClipmiError(f"jpeg: {entry} needs the HIP path (no CPU fallback)")
    L = _lib.lib()
    *arrays, streams, out_bytes, total_blocks, max_blocks, max_pixels = packer(items)
    recs, tables = arrays[0], arrays[-1]
    n = len(items)
    out = torch.empty(max(out_bytes, 16), dtype=torch.uint8, device=device)
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=device)
    if n == 0:
        return out, recs, status
    dev, offs, _ = _lib.to_device16(arrays + [streams], device)
    ws_bytes = int(workspace(L, n, total_blocks, len(tables)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    base = dev.data_ptr()
    head = [base + offs[-1], base + offs[0], n]                    # streams, records, then (scans, their count,) tables, their count
    for a, o in zip(arrays[1:], offs[1:-1]):
        head += [base + o, len(a)]
    rc = getattr(L, entry)(*head, total_blocks, max_blocks, max_pixels, out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes,
                           _lib.stream_ptr(device))
    _lib.check(rc, entry)
    cur = torch.cuda.current_stream(device)
    dev.record_stream(cur)
    ws.record_stream(cur)
    return out, recs, status


def decode_device(items, device, stream=None, layouts=False, cmyk=False):
    """Parsed records -> (out uint8 device tensor, records, status int32 device tensor): the RGB rows of image k start at
    records[k]["out_off"]. Asynchronous on torch's current stream of `device`; status is valid once that stream is.
    cmyk: four-component records (all of them, or none: pack) go to clipmi_jpeg_decode_cmyk8 - rows of width*4 CMYK bytes."""
    four = cmyk and any(it.ncomp == 4 for it in items)
    return _decode_device(items, device, partial(pack, layouts=layouts, cmyk=cmyk), lambda L, n, blocks, nt: L.clipmi_jpeg_workspace_bytes(blocks, nt),
                          "clipmi_jpeg_decode_cmyk8" if four else "clipmi_jpeg_decode_rgb8")


def _decode_files(blobs, device, parser, decode):
    """decode_files' and decode_progressive_files' body: parser(file) -> a record or Unsupported; decode: the records' decode_*_device"""
    items, where = [], []
    for k, b in enumerate(blobs):
        try:
            items.append(parser(b))
            where.append(k)
        except Unsupported:
            pass
    res = [None] * len(blobs)
    if not items:
        return res
    # (four-component records decode in a call of their own: another record, another entry, 4 bytes a pixel)
    for px in (3, 4):
        sel = [t for t, it in enumerate(items) if (getattr(it, "ncomp", 3) == 4) == (px == 4)]
        if not sel:
            continue
        out, recs, status = decode([items[t] for t in sel], device)
        st = status.cpu().numpy()
        host = out.cpu().numpy()
        for u, t in enumerate(sel):
            if st[u] == 0:
                r = recs[u]
                h, w, o = int(r["height"]), int(r["width"]), int(r["out_off"])
                res[where[t]] = host[o:o + h * w * px].reshape(h, w, px)
    return res


def decode_files(blobs, device, keep_stuffing=False, layouts=False, cmyk=False):
    """JPEG file contents -> list of uint8 [H,W,3] numpy arrays (None where the file is not for the device decoder or the
    device reported it corrupt). Synchronises; a convenience for tests and tools - the pipeline keeps the pixels in HBM.
    keep_stuffing: hand the segments over as they are in the file and let the device remove the byte stuffing (the pipeline's form).
    layouts: also decode luma 1x2 / 4x1 / 1x4 and RGB-coded files (jpeg_parse.parse(layouts=True)).
    cmyk: also decode four-component files (jpeg_parse.parse(cmyk=True)): [H,W,4] arrays, np.asarray(Image.open(f)) of a CMYK file."""
    return _decode_files(blobs, device, lambda b: parse(b, keep_stuffing=keep_stuffing, layouts=layouts, cmyk=cmyk),
                         partial(decode_device, layouts=layouts, cmyk=cmyk))


# ---- progressive files (jpeg_parse.parse_progressive; csrc/jpeg.hip jpeg_progressive_kernel). Opt-in in the pipeline.
PIMAGE = np.dtype([("coef_off", "<i8"), ("out_off", "<i8"), ("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("hs", "<i4"),
                   ("vs", "<i4"), ("first_scan", "<i4"), ("n_scans", "<i4"), ("reserved", "<i4", 5), ("quant", "u1", (3, 64))], align=True)
SCAN = np.dtype([("stream_off", "<i8"), ("stream_bytes", "<i4"), ("ncomp", "<i4"), ("comp", "<i4", 3), ("tbl", "<i4", 3), ("ss", "<i4"),
                 ("se", "<i4"), ("ah", "<i4"), ("al", "<i4"), ("reserved", "<i4", 2)], align=True)
assert PIMAGE.itemsize == 256 and SCAN.itemsize == 64


def pack_progressive(items, layouts=False):
    """Progressive records -> (PIMAGE array, SCAN array, tables uint8 [nt][288], streams uint8, out_bytes, total_blocks,
    max_blocks, max_pixels); layouts: as pack's"""
    _opted_in(items, layouts)
    recs = np.zeros(len(items), dtype=PIMAGE)
    scans = np.zeros(sum(len(it.scans) for it in items), dtype=SCAN)
    pool = {}
    soff = coff = ooff = 0
    ns = 0
    max_blocks = max_pixels = 1
    pieces = []
    for k, it in enumerate(items):
        r = recs[k]
        r["coef_off"], r["out_off"] = coff, ooff
        r["width"], r["height"], r["ncomp"], r["hs"], r["vs"] = it.width, it.height, it.ncomp, it.hs, it.vs
        r["first_scan"], r["n_scans"] = ns, len(it.scans)
        r["reserved"][0] = it.transform                     # (the colour transform, clipmi_jpeg_progressive_image)
        r["quant"] = it.quant
        for sc in it.scans:
            s = scans[ns]
            s["stream_off"], s["stream_bytes"], s["ncomp"] = soff, len(sc.stream), len(sc.comps)
            s["comp"] = list(sc.comps) + [0] * (3 - len(sc.comps))
            tabs = sc.dc if sc.ss == 0 else sc.ac
            s["tbl"] = [pool.setdefault(t, len(pool)) if t is not None else -1 for t in tabs] + [-1] * (3 - len(tabs))
            s["ss"], s["se"], s["ah"], s["al"] = sc.ss, sc.se, sc.ah, sc.al
            pad = (-len(sc.stream)) % 16 + 16
            pieces.append(sc.stream)
            pieces.append(b"\0" * pad)
            soff += len(sc.stream) + pad
            ns += 1
        nb = it.blocks()
        coff += nb
        ooff += (it.width * it.height * 3 + 15) // 16 * 16
        max_blocks, max_pixels = max(max_blocks, nb), max(max_pixels, it.width * it.height)
    tables = np.frombuffer(b"".join(pool), np.uint8).reshape(-1, TABLE_BYTES) if pool else np.zeros((0, TABLE_BYTES), np.uint8)
    return recs, scans, tables, np.frombuffer(b"".join(pieces), np.uint8), ooff, coff, max_blocks, max_pixels


def decode_progressive_device(items, device, stream=None, layouts=False):
    """Progressive records -> (out uint8 device tensor, records, status int32 device tensor), as decode_device: the RGB rows of
    image k start at records[k]["out_off"]. Asynchronous on torch's current stream of `device`."""
    return _decode_device(items, device, partial(pack_progressive, layouts=layouts), lambda L, n, blocks, nt: L.clipmi_jpeg_progressive_workspace_bytes(n, blocks, nt),
                          "clipmi_jpeg_decode_progressive_rgb8")


def decode_progressive_files(blobs, device, layouts=False):
    """Progressive JPEG file contents -> list of uint8 [H,W,3] numpy arrays (None where the file is not for the device decoder
    or the device reported it). Synchronises; a convenience for tests and tools. layouts: as decode_files'."""
    return _decode_files(blobs, device, partial(parse_progressive, layouts=layouts), partial(decode_progressive_device, layouts=layouts))


# ---- decode + the transform in one call (csrc/jpeg.hip jpeg_color_resize_h_kernel): baseline and progressive files straight to
# the uint8 [3, n_px, n_px] pixels `transform` computes before its float tail, the same bytes as decode + resize_crop_rgb8.
class Staged:
    """A batch of files parsed, planned and on the device (stage_transform), for run_transform"""
    __slots__ = ("n", "n_px", "device", "groups", "keep")


def stage_transform(blobs, n_px, device, keep_stuffing=False, layouts=False, cmyk=False):
    """JPEG file contents (or records parse / parse_progressive returned) -> Staged: the records of both kinds packed, the
    transform planned with decode_worker's planner (resize.pack_jobs: job k writes block k of the output, whichever kind file k
    is), everything copied to the device, workspaces allocated. Raises Unsupported for a file neither parser takes.
    layouts: the parsers run with layouts=True, and records of those layouts are taken.
    cmyk: `parse` runs with cmyk=True, and the four-component files are a third group, which run_transform decodes to CMYK rows
    and hands to clipmi_resize_crop_cmyk8 whatever `fused` says (the fused entries do not take four components)."""
    from . import resize
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.ClipmiError("jpeg.stage_transform needs the HIP path (no CPU fallback)")
    L = _lib.lib()
    kinds = ([], [], [])                                  # (position, record) of the baseline, the progressive and the four-component files
    for k, b in enumerate(blobs):
        if not isinstance(b, (Parsed, Progressive)):
            try:
                b = parse(b, keep_stuffing=keep_stuffing, layouts=layouts, cmyk=cmyk)
            except Unsupported:
                b = parse_progressive(b, layouts=layouts)
        kinds[2 if b.ncomp == 4 else isinstance(b, Progressive)].append((k, b))
    st = Staged()
    st.n, st.n_px, st.device, st.groups, st.keep = len(blobs), n_px, device, [], []
    for which, members in enumerate(kinds):
        if not members:
            continue
        items = [it for _, it in members]
        progressive, px = which == 1, 4 if which == 2 else 3
        if progressive:
            recs, scans, tables, streams, out_bytes, total_blocks, max_blocks, max_pixels = pack_progressive(items, layouts)
            arrays = [recs, scans, tables]
            ws_bytes = int(L.clipmi_jpeg_progressive_workspace_bytes(len(items), total_blocks, len(tables)))
        else:
            recs, tables, streams, out_bytes, total_blocks, max_blocks, max_pixels = pack(items, layouts, cmyk)
            arrays = [recs, tables]
            ws_bytes = int(L.clipmi_jpeg_workspace_bytes(total_blocks, len(tables)))
        jobs, coef, _, scratch_bytes, max_rows = resize.pack_jobs([(it.height, it.width) for it in items], n_px, px=px)
        jobs["out_index"] = [k for k, _ in members]
        jobs["src_off"] = recs["out_off"]                 # (the decoder's rows: what the unfused form's resize reads)
        arrays += [jobs, coef, streams]
        dev, offs, host = _lib.to_device16(arrays, device)
        st.keep.append(host)
        st.groups.append(dict(progressive=progressive, px=px, n=len(items), dev=dev, offs=offs, nscans=len(scans) if progressive else 0,
                              ntables=len(tables), total_blocks=total_blocks, max_blocks=max_blocks, max_pixels=max_pixels,
                              out_bytes=out_bytes, max_rows=max_rows, ws_bytes=ws_bytes,
                              ws=torch.empty(ws_bytes, dtype=torch.uint8, device=device),
                              scratch=torch.empty(scratch_bytes, dtype=torch.uint8, device=device),
                              where=torch.tensor([k for k, _ in members], dtype=torch.long, device=device)))
    return st


def run_transform(st, fused=True):
    """Staged -> (uint8 [n][3][n_px][n_px] device tensor, int32 [n] status device tensor; a file with a non-zero status has
    unspecified pixels). fused: clipmi_jpeg_decode_transform_rgb8 / clipmi_jpeg_decode_progressive_transform_rgb8; not fused: the decode
    entries into full-size RGB rows, then clipmi_resize_crop_rgb8 over them; a group of four-component files (stage_transform(cmyk=True))
    always takes the second form, through clipmi_jpeg_decode_cmyk8 and clipmi_resize_crop_cmyk8. Asynchronous on torch's current stream."""
    L = _lib.lib()
    out = torch.empty((st.n, 3, st.n_px, st.n_px), dtype=torch.uint8, device=st.device)
    status = torch.zeros(max(st.n, 1), dtype=torch.int32, device=st.device)
    stream = _lib.stream_ptr(st.device)
    for g in st.groups:
        base, o = g["dev"].data_ptr(), g["offs"]
        gst = torch.zeros(g["n"], dtype=torch.int32, device=st.device)
        head = (base + o[-1], base, g["n"]) + ((base + o[1], g["nscans"], base + o[2]) if g["progressive"] else (base + o[1],))
        head += (g["ntables"], g["total_blocks"], g["max_blocks"])
        jobs, coef = base + o[-3], base + o[-2]
        tail = (gst.data_ptr(), g["ws"].data_ptr(), g["ws_bytes"], stream)
        if fused and g["px"] == 3:
            name = "clipmi_jpeg_decode_progressive_transform_rgb8" if g["progressive"] else "clipmi_jpeg_decode_transform_rgb8"
            rc = getattr(L, name)(*head, jobs, g["max_rows"], coef, st.n_px, out.data_ptr(), g["scratch"].data_ptr(), *tail)
            _lib.check(rc, name)
        else:
            name = "clipmi_jpeg_decode_cmyk8" if g["px"] == 4 else "clipmi_jpeg_decode_progressive_rgb8" if g["progressive"] else "clipmi_jpeg_decode_rgb8"
            resize = "clipmi_resize_crop_cmyk8" if g["px"] == 4 else "clipmi_resize_crop_rgb8"
            rgb = torch.empty(max(g["out_bytes"], 16), dtype=torch.uint8, device=st.device)
            _lib.check(getattr(L, name)(*head, g["max_pixels"], rgb.data_ptr(), *tail), name)
            rc = getattr(L, resize)(rgb.data_ptr(), jobs, g["n"], g["max_rows"], coef, st.n_px, out.data_ptr(), g["scratch"].data_ptr(), stream)
            _lib.check(rc, resize)
            rgb.record_stream(torch.cuda.current_stream(st.device))
        status.index_copy_(0, g["where"], gst)
    return out, status[:st.n]


def transform_files(blobs, n_px, device, fused=True, layouts=False, cmyk=False):
    """JPEG file contents, baseline and progressive alike -> (uint8 [n][3][n_px][n_px] device tensor: Pillow's decode + bicubic resize
    of the shorter side to n_px + centre crop, as decode_worker.load_uint8; int32 [n] status device tensor, as the decode entries').
    fused=False computes the same through the decode entries and clipmi_resize_crop_rgb8, with the full-size RGB rows between.
    layouts, cmyk: as stage_transform's."""
    return run_transform(stage_transform(blobs, n_px, device, layouts=layouts, cmyk=cmyk), fused)
