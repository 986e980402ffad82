"""The Pillow part of the CLIP transform, and a worker PROCESS that runs it (host image pipeline).

`load_uint8` is what `transform(image)` does before its float tail (build-index.py:47-48): open, resize the shorter side
to n_px (bicubic), centre crop, RGB. It needs numpy and Pillow only, so this file can also run as a plain script

    python decode_worker.py

that serves decode requests over its stdin / stdout (see DecodePool in pipeline.py). Why processes: Pillow releases the
GIL inside the JPEG decoder, but for small images the Python around it dominates — eight decode THREADS gave 902 images/s
on 224 x 224 JPEGs where one gave 895; eight worker processes scale with the cores. The script is started by path, never
imported through the package, so a worker never imports torch or touches the GPU.

Protocol: see serve(). A file that does not decode is answered b"0" and reported per file like build-index.py:55-58.
"""
import sys
from collections import namedtuple

import numpy as np

try:
    from . import jpeg_parse, png_parse
except ImportError:                                        # started by path (a worker): the parsers lie beside this file
    import jpeg_parse
    import png_parse


def load_uint8(path, n_px, out=None):
    """Pillow part of the upstream transform: resize shorter side to n_px (bicubic), centre crop,
    RGB; returns uint8 [3, n_px, n_px] (written into `out` when given: the worker's slot of the shared segment, one
    strided copy instead of two). Identical pixels to `make_transform` before its float tail."""
    from PIL import Image
    img = Image.open(path)
    w, h = img.size
    if not (w <= h and w == n_px) and not (h <= w and h == n_px):
        if w <= h:
            nw, nh = n_px, int(n_px * h / w)
        else:
            nh, nw = n_px, int(n_px * w / h)
        img = img.resize((nw, nh), Image.BICUBIC)
        w, h = nw, nh
    left = int(round((w - n_px) / 2.0))
    top = int(round((h - n_px) / 2.0))
    img = img.crop((left, top, left + n_px, top + n_px)).convert("RGB")
    chw = np.asarray(img, dtype=np.uint8).transpose(2, 0, 1)
    if out is None:
        return np.ascontiguousarray(chw)
    np.copyto(out, chw)
    return out


# ---- the resize on the device: integer coefficient tables of Pillow's bicubic resampling -------------------------------
RESIZE_PREC = 22          # Pillow: PRECISION_BITS = 32 - 8 - 2


def _bicubic(x):
    a = -0.5              # Pillow's bicubic_filter
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def coeffs_window(in_size, out_size, o0, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (the published algorithm, same float64 operations in the same
    order) for outputs o0 .. o0 + n_out - 1 of an axis resampled from in_size to out_size.
    -> (first tap int32 [n_out], tap count int32 [n_out], coefficients int32 [n_out][ksize])"""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(o0, o0 + n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    cnt = xmax - xmin
    k = np.arange(ksize, dtype=np.float64)[None, :]
    w = np.where(k < cnt[:, None], _bicubic((k + xmin[:, None] - center[:, None] + 0.5) * ss), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1]                          # a sequential sum, as the C loop's
    w = np.where(ww[:, None] != 0.0, w / ww[:, None], w)
    kk = np.trunc(np.where(w < 0, -0.5 + w * (1 << RESIZE_PREC), 0.5 + w * (1 << RESIZE_PREC))).astype(np.int64)
    kk = np.where(k < cnt[:, None], kk, 0)
    return xmin.astype(np.int32), cnt.astype(np.int32), kk.astype(np.int32)


def resize_plan(w, h, n_px):
    """What clipmi_resize_crop_rgb8 needs to turn a w x h RGB image into the transform's n_px x n_px pixels: the sizes
    torchvision's Resize(n_px) + CenterCrop(n_px) arrive at (as load_uint8), the source rows the crop window needs, and the
    coefficient blocks ([n_px] first tap | [n_px] count | [n_px][k] coefficients) of the resampled axes."""
    if (w <= h and w == n_px) or (h <= w and h == n_px):
        nw, nh = w, h
    elif w <= h:
        nw, nh = n_px, int(n_px * h / w)
    else:
        nh, nw = n_px, int(n_px * w / h)
    left = int(round((nw - n_px) / 2.0))
    top = int(round((nh - n_px) / 2.0))
    plan = {"nw": nw, "nh": nh, "left": left, "top": top, "need_h": int(nw != w), "need_v": int(nh != h), "hk": 0, "vk": 0,
            "hcoef": np.zeros(0, np.int32), "vcoef": np.zeros(0, np.int32), "r0": top, "nrows": n_px}
    if plan["need_v"]:
        ymin, ycnt, kv = coeffs_window(h, nh, top, n_px)
        plan["r0"] = int(ymin.min())
        plan["nrows"] = int((ymin + ycnt).max()) - plan["r0"]
        plan["vk"] = kv.shape[1]
        plan["vcoef"] = np.concatenate([ymin, ycnt, kv.reshape(-1)])
    if plan["need_h"]:
        xmin, xcnt, kh = coeffs_window(w, nw, left, n_px)
        plan["hk"] = kh.shape[1]
        plan["hcoef"] = np.concatenate([xmin, xcnt, kh.reshape(-1)])
    return plan


def nearest_window(in_size, out_size, o0, n_out):
    """Pillow's NEAREST resize (ImagingScaleAffine, what Image.resize does to palette and 1-bit images whatever filter is asked
    for): the source index of outputs o0 .. o0 + n_out - 1 of an axis scaled from in_size to out_size. The source coordinate starts
    at half a step and grows by SEQUENTIAL float64 additions of in_size / out_size, not by multiplication. -> int32 [n_out]"""
    step = in_size / out_size
    at = np.cumsum(np.concatenate([[0.5 * step], np.full(out_size - 1, step)]))       # (cumsum adds in order)
    return np.minimum(at[o0:o0 + n_out].astype(np.int64), in_size - 1).astype(np.int32)


def nearest_plan(w, h, n_px):
    """resize_plan for images Pillow resizes with NEAREST (modes P and 1): the same sizes and crop window; in place of the
    coefficient blocks the source column of each of the n_px output columns ("hcoef") and the source row of each output row
    ("vcoef"), what clipmi_nearest_crop_p8 takes; r0 / nrows span the rows the window reads."""
    plan = dict(resize_plan(w, h, n_px))
    plan["hcoef"] = nearest_window(w, plan["nw"], plan["left"], n_px)
    plan["vcoef"] = nearest_window(h, plan["nh"], plan["top"], n_px)
    plan["hk"] = plan["vk"] = 0
    plan["r0"] = int(plan["vcoef"].min())
    plan["nrows"] = int(plan["vcoef"].max()) - plan["r0"] + 1
    return plan


PLAN_INTS = 16            # header of a full-size image's region: w h r0 nrows need_h need_v left top hk vk n_hcoef n_vcoef


def decode_full(path, n_px, region):
    """For the resize on the device: decode an RGB image at full size into `region` (a uint8 view of the parent's big
    segment) as [pixels HWC | pad to 16 | PLAN_INTS int32 | horizontal coefficient block | vertical block] and return
    (w, h, bytes used); None when the image should take the host path instead (not 8-bit RGB - the transform resamples in
    the image's own mode and converts afterwards -, nothing to resample, or it does not fit the region)."""
    from PIL import Image
    img = Image.open(path)
    w, h = img.size
    if img.mode != "RGB" or (w <= h and w == n_px) or (h <= w and h == n_px):
        return None
    npix = w * h * 3
    if npix + 4096 > region.size:
        return None
    plan = resize_plan(w, h, n_px)
    o_hdr = (npix + 15) // 16 * 16
    total = o_hdr + 4 * (PLAN_INTS + plan["hcoef"].size + plan["vcoef"].size)
    if total > region.size:
        return None
    region[:npix] = np.asarray(img, dtype=np.uint8).reshape(-1)
    ints = np.frombuffer(region, dtype=np.int32, count=(total - o_hdr) // 4, offset=o_hdr)
    ints[:PLAN_INTS] = [w, h, plan["r0"], plan["nrows"], plan["need_h"], plan["need_v"], plan["left"], plan["top"],
                        plan["hk"], plan["vk"], plan["hcoef"].size, plan["vcoef"].size, 0, 0, 0, 0]
    ints[PLAN_INTS:PLAN_INTS + plan["hcoef"].size] = plan["hcoef"]
    ints[PLAN_INTS + plan["hcoef"].size:] = plan["vcoef"]
    return w, h, total


JPEG_HDR_INTS = 32        # header of a region that holds a parsed file (stage_jpeg, stage_jpeg_progressive, stage_png): int32, see HDR
JPEG_QUANT_OFF = 128      # 3 x 64 quantisation steps, natural order
JPEG_TABLES_OFF = 320     # six raw Huffman tables (jpeg_parse.TABLE_BYTES each): DC, AC per component
JPEG_COEF_OFF = 2048      # the resize plan's coefficient blocks (int32), then what the format stores (16-byte aligned)
# A four-component file's region (stage_jpeg_cmyk, KIND_JPEG_CMYK) has the same parts at offsets of its own - four rows of steps and
# eight tables do not fit the gaps above; the other kinds' regions keep theirs:
CMYK_QUANT_OFF = 128      # 4 x 64 quantisation steps, natural order
CMYK_TABLES_OFF = 384     # eight raw Huffman tables: DC, AC per component
CMYK_COEF_OFF = 2688      # the resize plan's coefficient blocks (HDR.COEF_OFF says so), then the segment and the intervals' offsets


class HDR:
    """Where each of the JPEG_HDR_INTS ints of a parsed file's region header lies (_write_head writes them, device_stage.py reads them
    through these names); [28..31] are zero. Offsets count bytes from the region's start."""
    KIND, W, H = 0, 1, 2      # KIND: KIND_BASELINE, KIND_PROGRESSIVE, KIND_PNG, KIND_PNG_ALPHA, KIND_PNG_INDEX or KIND_JPEG_CMYK
    NCOMP, HS, VS = 3, 4, 5   # components (PNG: samples per pixel), luma sampling factors (PNG: 0 0)
    COUNT = 6                 # baseline, PNG: bytes of the stream at DATA_OFF; progressive: scan records at DATA_OFF
    BLOCKS = 7                # 8 x 8 blocks of the image (PNG: 0)
    PLAN = slice(8, 16)       # resize_plan's r0 nrows need_h need_v left top hk vk: the order of resize.JOB and of decode_full's header
    NROWS = 9
    N_HCOEF, N_VCOEF = 16, 17                                       # ints in the horizontal and the vertical coefficient block
    DATA_OFF, COEF_OFF = 18, 19                                     # the format's data behind the coefficient blocks; the blocks
    #                                                                 (JPEG_COEF_OFF; CMYK_COEF_OFF in a KIND_JPEG_CMYK region)
    RESTART_INTERVAL, N_INTERVALS, INTERVALS_OFF, STUFFED = 20, 21, 22, 23     # baseline, KIND_JPEG_CMYK: DRI, number of intervals, offset of their
    #                                                                 uint32 byte offsets into the segment, 1: the segment keeps its stuffing
    TABLES_OFF, N_TABLES = 20, 21                                   # progressive: the scans' Huffman tables
    DEPTH, CTYPE, ENTRIES = 20, 21, 22                              # KIND_PNG_ALPHA, KIND_PNG_INDEX: bit depth, colour type, palette
    #                                                                 entries; an index file's palette (768 bytes) lies at JPEG_TABLES_OFF.
    #                                                                 KIND_PNG: 0 0 0 for the 8-bit grey and RGB files, 16 2 0 for a 16-bit
    #                                                                 RGB file - in every PNG kind depth 16 marks a file only PNG_DEEP_BIT
    #                                                                 lets through, and clipmi_png_decode_px8 decodes it
    TRANSFORM, LAYOUT = 24, 25                                      # baseline, progressive: the colour transform (0 YCbCr -> RGB, 1 none:
    #                                                                 R, G, B components; KIND_JPEG_CMYK: 2 CMYK as stored, 3 YCCK);
    #                                                                 1: a file only LAYOUTS_BIT lets through
    INTERLACE = 26                                                  # the PNG kinds: 1 an Adam7 file, which only PNG_INTERLACED_BIT lets
    #                                                                 through (its scanlines are those of its passes); 0 in a JPEG region
    CHUNKS = 27                                                     # the PNG kinds: 1 a file with a chunk only PNG_CHUNKS_BIT lets through
    #                                                                 (png_parse.Parsed.chunks); 0 in a JPEG region


KIND_BASELINE, KIND_PROGRESSIVE, KIND_PNG = 3, 4, 6       # (2: decode_full's full-size pixels; 5: WANTED_TAG)
KIND_PNG_ALPHA, KIND_PNG_INDEX = 7, 8                     # png_parse's kinds "alpha" and "index" (clipmi_png_decode_px8)
KIND_JPEG_CMYK = 9                                        # four-component baseline files, CMYK as stored and YCCK (clipmi_jpeg_decode_cmyk8)
_plans = {}


def _contents(path, data):
    if data is None:
        with open(path, "rb") as f:
            data = f.read()
    return data


def _plan(w, h, n_px, nearest=False):
    key = (w, h, n_px, nearest)
    plan = _plans.get(key)
    if plan is None:
        if len(_plans) > 256:
            _plans.clear()
        plan = _plans[key] = (nearest_plan if nearest else resize_plan)(w, h, n_px)
    return plan


def _data_off(plan, coef_off=JPEG_COEF_OFF):
    """The first free 16-aligned offset behind the header, the tables and the plan's coefficient blocks"""
    return (coef_off + 4 * (plan["hcoef"].size + plan["vcoef"].size) + 15) // 16 * 16


def _no_room(p, total):
    return p.width, p.height, -total                      # the file does not fit its region: what it would need


def _write_head(region, kind, p, sampling, count, blocks, plan, specific=(0, 0, 0, 0), layout=(0, 0), interlace=0, coef_off=JPEG_COEF_OFF, chunks=0):
    """The header (HDR: sampling = NCOMP HS VS, specific = the four ints at [20..23], layout = TRANSFORM LAYOUT) and the plan's
    coefficient blocks (at coef_off)"""
    nh, nv = plan["hcoef"].size, plan["vcoef"].size
    ints = np.frombuffer(region, dtype=np.int32, count=JPEG_HDR_INTS)
    ints[:] = [kind, p.width, p.height, *sampling, count, blocks, plan["r0"], plan["nrows"], plan["need_h"], plan["need_v"],
               plan["left"], plan["top"], plan["hk"], plan["vk"], nh, nv, _data_off(plan, coef_off), coef_off, *specific, *layout,
               interlace, chunks] + [0] * 4
    if nh + nv:
        co = np.frombuffer(region, dtype=np.int32, count=nh + nv, offset=coef_off)
        co[:nh] = plan["hcoef"]
        co[nh:] = plan["vcoef"]


def _stream_end(off, nbytes):
    return (off + nbytes + 16 + 15) // 16 * 16


def _write_stream(region, off, stream):
    """The stream at `off` and zeros behind it: at least 16, up to the next 16-byte boundary (_stream_end)"""
    region[off:off + len(stream)] = np.frombuffer(stream, np.uint8)
    region[off + len(stream):_stream_end(off, len(stream))] = 0


def _layout(p):
    """HDR.TRANSFORM and HDR.LAYOUT of a record of jpeg_parse's"""
    return p.transform, int(jpeg_parse.is_layout(p))


def stage_jpeg(path, n_px, region, data=None, layouts=False):
    """For the decode on the device (csrc/jpeg.hip): read the file, walk its markers (jpeg_parse.parse) and lay out in `region`
    [header | quantisation steps | Huffman tables | resize plan coefficients | entropy-coded segment, followed by >= 16 zero
    bytes | the restart intervals' offsets]. -> (w, h, bytes used), (w, h, -bytes needed) when the file does not fit the region;
    raises jpeg_parse.Unsupported for files Pillow has to decode. layouts: the request allows luma 1x2 / 4x1 / 1x4 and RGB-coded
    files (jpeg_parse.parse(layouts=True)); without it such a file raises Unsupported, as ever."""
    p = jpeg_parse.parse(_contents(path, data), keep_stuffing=True, layouts=layouts)     # (a plain slice where the file allows: the device removes the byte stuffing)
    return _lay_out_baseline(region, KIND_BASELINE, p, n_px, JPEG_QUANT_OFF, JPEG_TABLES_OFF, JPEG_COEF_OFF)


def _lay_out_baseline(region, kind, p, n_px, quant_off, tables_off, coef_off):
    """stage_jpeg's and stage_jpeg_cmyk's body: the record `parse` returned into `region`, its parts at the kind's offsets"""
    plan = _plan(p.width, p.height, n_px)
    o_stream = _data_off(plan, coef_off)
    o_int = _stream_end(o_stream, len(p.stream))
    n_int = len(p.starts) if p.ri else 0
    total = (o_int + 4 * n_int + 15) // 16 * 16
    if total > region.size:
        return _no_room(p, total)
    _write_head(region, kind, p, (p.ncomp, p.hs, p.vs), len(p.stream), p.blocks(), plan, (p.ri, n_int, o_int, p.stuffed),
                _layout(p), coef_off=coef_off)
    region[quant_off:quant_off + p.quant.size] = p.quant.reshape(-1)
    region[tables_off:tables_off + len(p.tables) * jpeg_parse.TABLE_BYTES] = np.frombuffer(b"".join(p.tables), np.uint8)
    _write_stream(region, o_stream, p.stream)
    if n_int:
        np.frombuffer(region, dtype=np.uint32, count=n_int, offset=o_int)[:] = p.starts
        region[o_int + 4 * n_int:total] = 0
    return p.width, p.height, total


def stage_jpeg_cmyk(path, n_px, region, data=None, layouts=False):
    """stage_jpeg for the four-component files jpeg_parse.parse(cmyk=True) lets through (clipmi_jpeg_decode_cmyk8): the same parts
    - [header | quantisation steps | Huffman tables | resize plan coefficients | segment | the restart intervals' offsets] - at
    CMYK_QUANT_OFF, CMYK_TABLES_OFF and CMYK_COEF_OFF, four rows of steps and eight tables. A grey or three-component file raises
    Unsupported: those are stage_jpeg's (a launch group holds one kind of record). layouts: component 0 may be sampled 1x2 / 4x1 / 1x4."""
    p = jpeg_parse.parse(_contents(path, data), keep_stuffing=True, layouts=layouts, cmyk=True)
    if p.ncomp != 4:
        raise jpeg_parse.Unsupported("not a four-component file")
    return _lay_out_baseline(region, KIND_JPEG_CMYK, p, n_px, CMYK_QUANT_OFF, CMYK_TABLES_OFF, CMYK_COEF_OFF)


PROG_SCAN_BYTES = 64      # one scan record in a progressive region: jpeg.SCAN's layout (clipmi_jpeg_scan), offsets region-relative


def stage_jpeg_progressive(path, n_px, region, data=None, layouts=False):
    """For the progressive decode on the device (csrc/jpeg.hip jpeg_progressive_kernel): read the file, walk its markers
    (jpeg_parse.parse_progressive) and lay out in `region` [header | quantisation steps | resize plan coefficients | scan records |
    the scans' Huffman tables | the scans' entropy-coded segments without byte stuffing, each 16-byte aligned and followed by
    >= 16 zero bytes]. A scan record's stream_off counts from the region's start and its table indices from the region's first
    table. -> (w, h, bytes used), (w, h, -bytes needed) when the file does not fit; raises jpeg_parse.Unsupported for files
    Pillow has to decode. layouts: as stage_jpeg's."""
    p = jpeg_parse.parse_progressive(_contents(path, data), layouts=layouts)
    plan = _plan(p.width, p.height, n_px)
    tables = {}
    for sc in p.scans:
        for t in (sc.dc if sc.ss == 0 else sc.ac):
            if t is not None:
                tables.setdefault(t, len(tables))
    o_scans = _data_off(plan)
    o_tab = o_scans + PROG_SCAN_BYTES * len(p.scans)
    total = (o_tab + jpeg_parse.TABLE_BYTES * len(tables) + 15) // 16 * 16
    offs = []
    for sc in p.scans:
        offs.append(total)
        total = _stream_end(total, len(sc.stream))
    if total > region.size:
        return _no_room(p, total)
    _write_head(region, KIND_PROGRESSIVE, p, (p.ncomp, p.hs, p.vs), len(p.scans), p.blocks(), plan, (o_tab, len(tables), 0, 0),
                _layout(p))
    region[JPEG_QUANT_OFF:JPEG_QUANT_OFF + 192] = p.quant.reshape(-1)
    rec = np.frombuffer(region, dtype=np.int32, count=PROG_SCAN_BYTES // 4 * len(p.scans), offset=o_scans).reshape(len(p.scans), -1)
    rec[:] = 0
    for k, sc in enumerate(p.scans):
        tabs = sc.dc if sc.ss == 0 else sc.ac
        idx = [tables[t] if t is not None else -1 for t in tabs] + [-1] * (3 - len(tabs))
        comps = list(sc.comps) + [0] * (3 - len(sc.comps))
        # <i8 stream_off | i4 stream_bytes, ncomp | comp[3] | tbl[3] | ss se ah al | reserved[2]
        rec[k, 0], rec[k, 1] = offs[k], 0
        rec[k, 2:14] = [len(sc.stream), len(sc.comps)] + comps + idx + [sc.ss, sc.se, sc.ah, sc.al]
    for t, j in tables.items():
        region[o_tab + j * jpeg_parse.TABLE_BYTES:o_tab + (j + 1) * jpeg_parse.TABLE_BYTES] = np.frombuffer(t, np.uint8)
    for sc, off in zip(p.scans, offs):
        _write_stream(region, off, sc.stream)
    return p.width, p.height, total


PNG_MAX_RAW = 16 << 20      # filtered scanlines of a file the device takes: one wave inflates one image (~30 ms per MB of literals,
                            # DESIGN 4.9), so a larger file would hold up its batch on the side stream; Pillow decodes those


def stage_png(path, n_px, region, data=None, modes=False, interlaced=False, chunks=False, deep=False):
    """For the PNG decode on the device (csrc/png.hip): read the file, walk its chunks (png_parse.parse) and lay out in `region`
    [header | resize plan coefficients | DEFLATE stream without the zlib header, 16-byte aligned and followed by >= 16 zero
    bytes]. -> (w, h, bytes used), (w, h, -bytes needed) when the file does not fit; raises png_parse.Unsupported for files
    Pillow has to decode, among them files of more than PNG_MAX_RAW bytes of scanlines.
    modes: the request allows alpha, palette and low-depth files (png_parse.parse(modes=True)). Their regions have the same
    layout under the kinds KIND_PNG_ALPHA and KIND_PNG_INDEX (HDR.KIND), with depth, colour type and palette entries in the
    header (HDR.DEPTH ..); an index file's palette lies at JPEG_TABLES_OFF and its "coefficient blocks" are nearest_plan's two
    tables. Without it such a file raises Unsupported, as ever.
    interlaced: the request allows Adam7 files of the kinds let through (png_parse.parse(interlaced=True)); the region has the
    same layout and says so in HDR.INTERLACE. Without it such a file raises Unsupported, as ever.
    chunks: the request allows files with metadata chunks (png_parse.parse(chunks=True)); the same region, and HDR.CHUNKS says that
    the file needed it. deep: the request allows files of depth 16 (png_parse.parse(deep=True)): RGB ones as KIND_PNG with depth
    and colour type in the header (16, 2), RGBA and grey + alpha ones (with modes) as KIND_PNG_ALPHA with HDR.DEPTH 16. Without
    either such a file raises Unsupported, as ever.
    data: the file's contents, when the caller has read them."""
    p = png_parse.parse(_contents(path, data), modes=modes, interlaced=interlaced, chunks=chunks, deep=deep)
    if p.raw_bytes() > PNG_MAX_RAW:
        raise png_parse.Unsupported("more than PNG_MAX_RAW bytes of scanlines")
    plan = _plan(p.width, p.height, n_px, nearest=p.kind == "index")
    o_stream = _data_off(plan)
    total = _stream_end(o_stream, len(p.stream))
    if total > region.size:
        return _no_room(p, total)
    if p.kind == "rgb":
        _write_head(region, KIND_PNG, p, (p.channels, 0, 0), len(p.stream), 0, plan, (16, 2, 0, 0) if p.depth == 16 else (0, 0, 0, 0),
                    interlace=p.interlace, chunks=p.chunks)
    else:
        _write_head(region, KIND_PNG_INDEX if p.kind == "index" else KIND_PNG_ALPHA, p, (p.channels, 0, 0), len(p.stream), 0, plan,
                    (p.depth, p.ctype, p.n_entries, 0), interlace=p.interlace, chunks=p.chunks)
        if p.kind == "index":
            region[JPEG_TABLES_OFF:JPEG_TABLES_OFF + 768] = p.palette.reshape(-1)
    _write_stream(region, o_stream, p.stream)
    return p.width, p.height, total


def _stage_png_kind(kind):
    """stage_png(modes=True) for the files of one of the new kinds only: a launch group holds one kind (PARSED)"""
    def stage(path, n_px, region, data=None, interlaced=False, chunks=False, deep=False):
        data = _contents(path, data)
        ctype, depth = data[25], data[24]                         # IHDR, before any work: which kind the file would be
        index = ctype == 3 or (ctype == 0 and depth == 1)
        if (ctype, depth) in ((0, 8), (2, 8), (2, 16)) or index != (kind == KIND_PNG_INDEX):      # (16-bit RGB is KIND_PNG's)
            raise png_parse.Unsupported("a file of another kind")
        return stage_png(path, n_px, region, data, modes=True, interlaced=interlaced, chunks=chunks, deep=deep)
    return stage


# One way a file can sit in a region of the big segment for the device. kind: the worker's reply tag (b"%d" % kind), HDR.KIND and
# the first entry of DecodePool's (kind, w, h, bytes); bit: the bit of the request's mode that allows it; magic: which files the
# stager is tried on (serve() looks at the first bytes); stat: encode_files' stats key - "staged" counts the files a worker laid
# out, "decoded" those of them the device did not report.
Kind = namedtuple("Kind", "kind bit magic stager stat counts")
FULL_SIZE = Kind(2, 1, None, decode_full, None, None)         # decoded pixels at full size, for the resize on the device
# the parsed files, in the order serve() tries them and the device's statuses are laid out (device_stage.DeviceStage.run)
PARSED = (Kind(KIND_BASELINE, 2, "jpeg", stage_jpeg, "jpeg_files", "staged"),
          Kind(KIND_PROGRESSIVE, 4, "jpeg", stage_jpeg_progressive, "jpeg_progressive_files", "staged"),
          Kind(KIND_PNG, 8, "png", stage_png, "png_files", "decoded"),
          # alpha, palette and low-depth PNG files: one bit of the mode for both kinds, one stats key
          Kind(KIND_PNG_ALPHA, 16, "png", _stage_png_kind(KIND_PNG_ALPHA), "png_mode_files", "decoded"),
          Kind(KIND_PNG_INDEX, 16, "png", _stage_png_kind(KIND_PNG_INDEX), "png_mode_files", "decoded"))
# Kinds added behind the five above. They are kept apart because PARSED is also the list of kinds every pull of
# device_stage.formats() covers; serve(), the reply tags, DeviceStage and the status layout run over ALL_PARSED.
PARSED_MORE = (Kind(KIND_JPEG_CMYK, 128, "jpeg", stage_jpeg_cmyk, "jpeg_cmyk_files", "staged"),)
ALL_PARSED = PARSED + PARSED_MORE
LAYOUTS_BIT = 32           # a bit of the mode that adds no kind: the two JPEG stagers run with layouts=True (jpeg_parse.parse(layouts=True));
#                            encode_files counts the files it lets through (HDR.LAYOUT) under LAYOUTS_STAT
LAYOUTS_STAT = "jpeg_layout_files"
PNG_INTERLACED_BIT = 64    # another such bit: the PNG stagers run with interlaced=True (png_parse.parse(interlaced=True)), so it takes
#                            effect only beside the bits of the PNG kinds; encode_files counts the files it lets through and the
#                            device did not report (HDR.INTERLACE) under PNG_INTERLACED_STAT, and not under the kind's own key
PNG_INTERLACED_STAT = "png_interlaced_files"
PNG_CHUNKS_BIT = 256       # two more such bits, for the PNG stagers as well: chunks=True (png_parse.parse(chunks=True): files with metadata
PNG_DEEP_BIT = 512         # chunks) and deep=True (files of depth 16; RGBA and grey + alpha ones need the bit of their kinds too).
#                            encode_files counts the files the device did not report under ONE key each: a 16-bit file (HDR.DEPTH)
#                            under PNG_DEEP_STAT, else an Adam7 file under PNG_INTERLACED_STAT, else a file with HDR.CHUNKS under
#                            PNG_CHUNKS_STAT, else under its kind's own key - so every key counts the files its switch added
PNG_CHUNKS_STAT, PNG_DEEP_STAT = "png_chunk_files", "png_deep_files"


def _stager_switches(mode, magic):
    """The keyword arguments the mode's kind-less bits give the stagers of the files with that magic"""
    if magic == "jpeg":
        return {"layouts": True} if mode & LAYOUTS_BIT else {}
    return {name: True for bit, name in ((PNG_INTERLACED_BIT, "interlaced"), (PNG_CHUNKS_BIT, "chunks"), (PNG_DEEP_BIT, "deep")) if mode & bit}
PARSED_KINDS = frozenset(k.kind for k in ALL_PARSED)
REGION_TAGS = frozenset(b"%d" % k.kind for k in (FULL_SIZE,) + ALL_PARSED)
WANTED_TAG = b"5"          # the transform's pixels are in the slot, and a larger region would have taken the parsed file


def serve(fin, fout):
    """Answer requests until stdin closes. Request line (tab separated):
         n_px | small segment or - | byte offset of the slot | big segment or - | byte offset of the region | its size |
         what the region may take (the bits of FULL_SIZE and ALL_PARSED, LAYOUTS_BIT, PNG_INTERLACED_BIT, PNG_CHUNKS_BIT, PNG_DEEP_BIT) |
         path as hex (file names may contain newlines and tabs)
       Reply, 17 bytes when a segment was named (status + <iiq, zero where unused): b"0" failed | b"1" the transform's n_px x n_px
              pixels are in the slot (no segment named: b"1" + the pixels) |
              a Kind's tag (FULL_SIZE, ALL_PARSED) + <iiq (w, h, bytes)>: the file sits in the region as that kind's stager left it,
              with its resize plan |
              WANTED_TAG + <iiq (w, h, bytes)>: as b"1", and the file would have been one of ALL_PARSED with a region of that many
              bytes."""
    import mmap
    import os
    import struct
    segments = {}                                              # name -> mmap of /dev/shm/<name> (the parent owns it)

    def mapped(name):
        seg = segments.get(name)
        if seg is None:
            if len(segments) > 8:                              # the parent rotates a few segments; drop stale mappings
                _close_all(segments)
            # plain mmap of the POSIX segment's file: multiprocessing.shared_memory would start a resource-tracker
            # process per worker and try to unlink the parent's segment at exit (Python < 3.13)
            fd = os.open("/dev/shm/" + name.lstrip("/"), os.O_RDWR)
            try:
                seg = segments[name] = mmap.mmap(fd, 0)
            finally:
                os.close(fd)
        return seg

    while True:
        line = fin.readline()
        if not line:
            break
        try:
            n_px_s, shm_name, off_s, big_name, big_off_s, big_cap_s, mode_s, path = line.rstrip(b"\n").split(b"\t", 7)
            n_px, off, mode = int(n_px_s), int(off_s), int(mode_s)
            fname = bytes.fromhex(path.decode("ascii")).decode("utf-8", "surrogateescape")      # hex: see DecodePool._run
            reply = wanted = None
            if big_name != b"-":
                region = np.frombuffer(mapped(big_name.decode()), dtype=np.uint8, count=int(big_cap_s), offset=int(big_off_s))
                full = None
                # the file is read once and its first bytes choose the parser (a PNG file used to be read by each of them in turn)
                data = magic = None
                if any(mode & k.bit for k in ALL_PARSED):
                    try:
                        data = _contents(fname, None)
                    except OSError:                            # unreadable: Pillow reports it
                        data = None
                    if data is not None:
                        magic = "png" if data[:8] == b"\x89PNG\r\n\x1a\n" else "jpeg" if data[:2] == b"\xff\xd8" else None
                for k in ALL_PARSED:
                    if full is not None or wanted is not None or not mode & k.bit or magic != k.magic:
                        continue
                    try:
                        full = k.stager(fname, n_px, region, data, **_stager_switches(mode, k.magic))
                    except Exception:                          # not a file for this device decoder: the next one, or Pillow
                        full = None
                    if full is not None and full[2] < 0:
                        full, wanted = None, (full[0], full[1], -full[2])
                    if full is not None:
                        reply = b"%d" % k.kind + struct.pack("<iiq", *full)
                data = None
                if full is None and mode & FULL_SIZE.bit:
                    full = decode_full(fname, n_px, region)
                    if full is not None:
                        reply = b"%d" % FULL_SIZE.kind + struct.pack("<iiq", *full)
                region = None
            if reply is None:
                if shm_name == b"-":
                    reply = b"1" + load_uint8(fname, n_px).tobytes()
                else:
                    slot = np.frombuffer(mapped(shm_name.decode()), dtype=np.uint8, count=3 * n_px * n_px, offset=off)
                    load_uint8(fname, n_px, out=slot.reshape(3, n_px, n_px))
                    slot = None                                # no view may outlive the request (close() refuses then)
                    reply = b"1" if wanted is None else WANTED_TAG + struct.pack("<iiq", *wanted)
        except KeyboardInterrupt:
            break
        except Exception:
            reply = b"0"
        if len(reply) == 1:
            reply += b"\0" * 16
        fout.write(reply)
        fout.flush()
    _close_all(segments)


def _close_all(segments):
    for s in segments.values():
        try:
            s.close()
        except BufferError:
            pass
    segments.clear()


if __name__ == "__main__":
    import signal
    signal.signal(signal.SIGINT, signal.SIG_IGN)      # Ctrl-C is the parent's business; a worker leaves at EOF on stdin
    try:
        serve(sys.stdin.buffer, sys.stdout.buffer)
    except (BrokenPipeError, KeyboardInterrupt):
        pass
