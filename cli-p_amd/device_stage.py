"""Regions of the big segment -> rows of the batch tensor: the device half of pipeline.encode_files' copy stage.

A decode worker leaves a file in its region of the big shared-memory segment decoded at full size (decode_worker.FULL_SIZE) or parsed
for a device decoder (decode_worker.PARSED). Here the regions' headers become the records the C entries take (`*_records`), a batch's
files are grouped under a budget of HBM (`file_need`, `_groups`), and `DeviceStage.run` copies the segment to the device once and queues
each kind's decode and transform behind the copy. What differs between the kinds is a row of `_FORMATS` (a `Format`) each."""
from collections import namedtuple
from functools import partial
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .decode_worker import (ALL_PARSED, FULL_SIZE, HDR, KIND_BASELINE, KIND_JPEG_CMYK, KIND_PNG, KIND_PNG_ALPHA, KIND_PNG_INDEX,
                            KIND_PROGRESSIVE, PARSED, PLAN_INTS)  # noqa: F401 (PARSED: the kinds formats() covers)


def _headers(bigview, n, cap, slots):
    """The region headers (decode_worker.HDR) of `slots` as int64 [len(slots)][JPEG_HDR_INTS]: one strided gather out of the
    segment (uint8, n regions of cap bytes)"""
    from .decode_worker import JPEG_HDR_INTS
    hd = np.lib.stride_tricks.as_strided(bigview[:4 * JPEG_HDR_INTS].view(np.int32), shape=(n, JPEG_HDR_INTS), strides=(cap, 4))
    return hd[slots].astype(np.int64)


def _resize_jobs(src_off, w, h, plan, n_hcoef, hcoef_off, out_index, n_px, px=3):
    """clipmi_resize_job records. plan: [n][8] r0 nrows need_h need_v left top hk vk (HDR.PLAN); hcoef_off: where each image's
    horizontal coefficient block starts, in ints from the segment's start - the vertical block follows it; the rows the
    vertical pass leaves for the horizontal one lie back to back in the scratch buffer (tmp_off), px bytes a pixel."""
    from .resize import JOB
    jobs = np.zeros(len(w), dtype=JOB)
    jobs["src_off"], jobs["w"], jobs["h"], jobs["out_index"] = src_off, w, h, out_index
    for k, f in enumerate(("r0", "nrows", "need_h", "need_v", "left", "top", "hk", "vk")):
        jobs[f] = plan[:, k]
    jobs["hcoef_off"] = hcoef_off
    jobs["vcoef_off"] = jobs["hcoef_off"] + n_hcoef
    tmp = plan[:, 1] * n_px * px
    jobs["tmp_off"] = np.cumsum(tmp) - tmp
    return jobs


def _decoded_jobs(hd, cap, slots, comp, n_px, px=3):
    """-> (the transform's jobs for parsed files whose decoded rows, px bytes a pixel, lie back to back, 16-byte aligned, in the
    decoder's output: the order of `slots`; their offsets there; their sizes). px 3 and 4: clipmi_resize_job records; px 1 (index
    rows): clipmi_nearest_job records that point at the palette and the two tables in the file's region."""
    w, h = hd[:, HDR.W], hd[:, HDR.H]
    out_sz = (w * h * px + 15) // 16 * 16
    out_off = np.cumsum(out_sz) - out_sz
    if px == 1:
        from .decode_worker import JPEG_TABLES_OFF
        from .resize import NEAREST_JOB
        jobs = np.zeros(len(w), dtype=NEAREST_JOB)
        jobs["src_off"], jobs["w"], jobs["h"], jobs["out_index"] = out_off, w, h, np.asarray(comp)[slots]
        jobs["pal_off"] = slots * cap + JPEG_TABLES_OFF
        jobs["col_off"] = (slots * cap + hd[:, HDR.COEF_OFF]) // 4
        jobs["row_off"] = jobs["col_off"] + hd[:, HDR.N_HCOEF]
        return jobs, out_off, out_sz
    jobs = _resize_jobs(out_off, w, h, hd[:, HDR.PLAN], hd[:, HDR.N_HCOEF], (slots * cap + hd[:, HDR.COEF_OFF]) // 4,
                        np.asarray(comp)[slots], n_px, px)
    return jobs, out_off, out_sz


def jpeg_records(bigview, n, cap, slots, comp, n_px, nc=3):
    """The device decoder's records out of a batch's regions of the big segment (decode_worker.stage_jpeg wrote them): every field
    comes out of the regions' headers as one strided numpy gather - no Python per image except the table-set look-up.
    bigview: the segment (uint8, n regions of cap bytes); slots: the regions that hold a parsed JPEG file; comp: slot -> row of the
    batch's tensor. -> (clipmi_jpeg_image records with offsets into the segment, distinct raw Huffman tables uint8, clipmi_resize_job
    records whose sources are the decoder's outputs laid out back to back, output bytes per image, blocks per image, number of tables)
    nc = 4: the regions decode_worker.stage_jpeg_cmyk wrote - clipmi_jpeg_image4 records, four rows of steps and eight tables at that
    kind's offsets, decoded rows of 4 bytes a pixel."""
    from . import jpeg as J
    from . import decode_worker as W
    quant_off, tables_off = (W.CMYK_QUANT_OFF, W.CMYK_TABLES_OFF) if nc == 4 else (W.JPEG_QUANT_OFF, W.JPEG_TABLES_OFF)
    nt = 2 * nc
    slots = np.asarray(slots, dtype=np.int64)
    n3 = len(slots)
    st = np.lib.stride_tricks.as_strided
    hd = _headers(bigview, n, cap, slots)
    jobs, out_off, out_sz = _decoded_jobs(hd, cap, slots, comp, n_px, 4 if nc == 4 else 3)
    blocks = hd[:, HDR.BLOCKS]
    recs = np.zeros(n3, dtype=J.IMAGE4 if nc == 4 else J.IMAGE)
    recs["stream_off"], recs["coef_off"], recs["out_off"] = slots * cap + hd[:, HDR.DATA_OFF], np.cumsum(blocks) - blocks, out_off
    recs["stream_bytes"], recs["width"], recs["height"] = hd[:, HDR.COUNT], hd[:, HDR.W], hd[:, HDR.H]
    recs["ncomp"], recs["hs"], recs["vs"] = hd[:, HDR.NCOMP], hd[:, HDR.HS], hd[:, HDR.VS]
    recs["restart_interval"], recs["n_intervals"] = hd[:, HDR.RESTART_INTERVAL], hd[:, HDR.N_INTERVALS]
    recs["intervals_off"], recs["stuffed"] = slots * cap + hd[:, HDR.INTERVALS_OFF], hd[:, HDR.STUFFED]
    recs["reserved"] = hd[:, HDR.TRANSFORM]                  # (the colour transform, clipmi_jpeg_image)
    recs["quant"] = st(bigview[quant_off:], shape=(n, nc * 64), strides=(cap, 1))[slots].reshape(n3, nc, 64)
    # the Huffman tables: distinct six-table (eight-table) sets first (files of one encoder share theirs), then distinct tables
    tabs = st(bigview[tables_off:], shape=(n, nt * J.TABLE_BYTES), strides=(cap, 1))[slots]
    sets, pool_t, set_idx = {}, {}, np.zeros((n3, nt), np.int32)
    for k in range(n3):
        key = tabs[k].tobytes()
        idx = sets.get(key)
        if idx is None:
            idx = sets[key] = [pool_t.setdefault(key[t * J.TABLE_BYTES:(t + 1) * J.TABLE_BYTES], len(pool_t)) for t in range(nt)]
        set_idx[k] = idx
    recs["dc_tbl"], recs["ac_tbl"] = set_idx[:, 0::2], set_idx[:, 1::2]
    tables = np.frombuffer(b"".join(pool_t), np.uint8)
    return recs, tables, jobs, out_sz, blocks, len(pool_t)


def progressive_records(bigview, n, cap, slots, comp, n_px):
    """jpeg_records for progressive files (decode_worker.stage_jpeg_progressive wrote the regions). -> (clipmi_jpeg_progressive_image
    records, clipmi_jpeg_scan records with offsets into the segment, distinct raw Huffman tables uint8, clipmi_resize_job records
    whose sources are the decoder's outputs laid out back to back, output bytes per image, blocks per image, number of tables)"""
    from . import jpeg as J
    from .decode_worker import JPEG_QUANT_OFF, PROG_SCAN_BYTES
    slots = np.asarray(slots, dtype=np.int64)
    n4 = len(slots)
    hd = _headers(bigview, n, cap, slots)
    jobs, out_off, out_sz = _decoded_jobs(hd, cap, slots, comp, n_px)
    nscans, blocks = hd[:, HDR.COUNT], hd[:, HDR.BLOCKS]
    recs = np.zeros(n4, dtype=J.PIMAGE)
    recs["coef_off"], recs["out_off"], recs["width"], recs["height"] = np.cumsum(blocks) - blocks, out_off, hd[:, HDR.W], hd[:, HDR.H]
    recs["ncomp"], recs["hs"], recs["vs"] = hd[:, HDR.NCOMP], hd[:, HDR.HS], hd[:, HDR.VS]
    recs["first_scan"], recs["n_scans"] = np.cumsum(nscans) - nscans, nscans
    recs["reserved"][:, 0] = hd[:, HDR.TRANSFORM]            # (the colour transform, clipmi_jpeg_progressive_image)
    recs["quant"] = np.lib.stride_tricks.as_strided(bigview[JPEG_QUANT_OFF:], shape=(n, 192), strides=(cap, 1))[slots].reshape(n4, 3, 64)
    scans = np.zeros(int(nscans.sum()), dtype=J.SCAN)
    pool_t = {}
    for k in range(n4):
        base = int(slots[k]) * cap
        o_scans, o_tab, nt = int(hd[k, HDR.DATA_OFF]), int(hd[k, HDR.TABLES_OFF]), int(hd[k, HDR.N_TABLES])
        local = bigview[base + o_scans:base + o_scans + PROG_SCAN_BYTES * int(nscans[k])].copy().view(J.SCAN)
        remap = np.array([pool_t.setdefault(bigview[base + o_tab + t * J.TABLE_BYTES:base + o_tab + (t + 1) * J.TABLE_BYTES].tobytes(),
                                            len(pool_t)) for t in range(nt)] + [-1], dtype=np.int32)
        local["stream_off"] += base
        local["tbl"] = remap[np.where(local["tbl"] >= 0, local["tbl"], nt)]
        f = int(recs["first_scan"][k])
        scans[f:f + len(local)] = local
    tables = np.frombuffer(b"".join(pool_t), np.uint8)
    return recs, scans, tables, jobs, out_sz, blocks, len(pool_t)


def _png_scanlines(hd, px=3):
    """Bytes of filtered scanlines per file. A KIND_PNG region's header does not carry the depth (stage_png leaves [20..23] zero for
    grey / RGB files, which are 8 bits deep); the regions of the other kinds do (HDR.DEPTH). An Adam7 file (HDR.INTERLACE) holds
    the scanlines of its passes (png_parse.adam7_raw_bytes). A 16-bit RGB file is a KIND_PNG region that does carry its depth
    (_png_deep); the 16-bit files of KIND_PNG_ALPHA carry it like every file of that kind."""
    from .png_parse import adam7_raw_bytes
    depth = np.where(_png_deep(hd), 16, 8) if px == 3 else hd[:, HDR.DEPTH]
    bits = hd[:, HDR.NCOMP] * depth
    plain = hd[:, HDR.H] * (1 + (hd[:, HDR.W] * bits + 7) // 8)
    lace = hd[:, HDR.INTERLACE] != 0
    return np.where(lace, adam7_raw_bytes(hd[:, HDR.W], hd[:, HDR.H], bits), plain) if lace.any() else plain


def _png_deep(hd):
    """Which of the headers are those of PNG regions with a 16-bit file (HDR.DEPTH; a JPEG region keeps other things there)"""
    png = (hd[:, HDR.KIND] == KIND_PNG) | (hd[:, HDR.KIND] == KIND_PNG_ALPHA) | (hd[:, HDR.KIND] == KIND_PNG_INDEX)
    return png & (hd[:, HDR.DEPTH] == 16)


def png_records(bigview, n, cap, slots, comp, n_px, px=3):
    """jpeg_records for PNG files (decode_worker.stage_png wrote the regions). -> (clipmi_png_image records with stream offsets into
    the segment and the scanline and output buffers laid out back to back, the transform's job records whose sources are the
    decoder's outputs, output bytes per image, scanline bytes per image, each rounded up to 16).
    px: bytes per decoded pixel - 3 for grey / RGB files (KIND_PNG), 4 "alpha" and 1 "index" for the files of png_parse's other kinds
    (stage_png(modes=True)), whose records carry colour type, depth and palette entries for clipmi_png_decode_px8. So do the
    records of 16-bit RGB files among the KIND_PNG regions (px 3), which that entry decodes too: _png_group sends a group of them
    there, and DeviceStage keeps them in groups of their own."""
    from . import png as P
    slots = np.asarray(slots, dtype=np.int64)
    hd = _headers(bigview, n, cap, slots)
    jobs, out_off, out_sz = _decoded_jobs(hd, cap, slots, comp, n_px, px)
    recs = np.zeros(len(slots), dtype=P.IMAGE)
    raw_sz = (_png_scanlines(hd, px) + 15) // 16 * 16
    recs["stream_off"], recs["raw_off"], recs["out_off"] = slots * cap + hd[:, HDR.DATA_OFF], np.cumsum(raw_sz) - raw_sz, out_off
    recs["stream_bytes"], recs["width"], recs["height"], recs["channels"] = hd[:, HDR.COUNT], hd[:, HDR.W], hd[:, HDR.H], hd[:, HDR.NCOMP]
    px8 = _png_deep(hd) if px == 3 else np.ones(len(slots), bool)       # (Parsed.px8: every file but 8-bit grey and RGB)
    recs["reserved"] = P.reserved_words(px8, hd[:, HDR.CTYPE], hd[:, HDR.DEPTH], hd[:, HDR.ENTRIES], hd[:, HDR.INTERLACE])
    return recs, jobs, out_sz, raw_sz


def _groups(need, budget):
    """[lo, hi) ranges of consecutive files whose `need` sums stay within the budget: a group closes when the next file would
    exceed it, and a file above the budget is a group of its own. No files, no group."""
    groups, lo, acc = [], 0, 0
    for k in range(len(need)):
        if k > lo and acc + need[k] > budget:
            groups.append((lo, k))
            lo, acc = k, 0
        acc += int(need[k])
    return groups + [(lo, len(need))] if len(need) else groups


def _split(groups, flag):
    """The [lo, hi) ranges cut where `flag` (bool per file) changes, so that each holds files of one value: the 16-bit RGB files
    among a batch's KIND_PNG regions go to another decode entry than the 8-bit ones (_png_group)"""
    out = []
    for lo, hi in groups:
        cuts = [lo] + [k for k in range(lo + 1, hi) if flag[k] != flag[k - 1]] + [hi]
        out += list(zip(cuts[:-1], cuts[1:]))
    return out


def _pack16(arrays):
    """Arrays -> (one uint8 buffer that holds their bytes at 16-byte-aligned offsets, the offsets)"""
    buf, offs = _lib.pack16(arrays)
    return buf.numpy(), offs


# A group builder: (library, what the records function returned) -> (the arrays that travel to the device, 16-byte aligned in this
# order, the transform's jobs last; output bytes per image; workspace bytes; the decode entry's name; its call). Every call has one
# shape: decode(base, sb, offs, rgb, status, ws, stream, tr) - the segment and the group's packed arrays on the device, the arrays'
# offsets, the full-size decoded rows, the group's statuses, the workspace, the stream and a Transform, which the entries that
# only decode ignore as those that transform too ignore rgb. Transform: the group's largest nrows, n_px, the batch's tensor and the
# rows between the resize's two passes (device pointers).
Transform = namedtuple("Transform", "max_rows n_px out scratch")


def _jpeg_group(L, r, progressive=False, fused=False, cmyk=False):
    recs, *scans, tables, jobs, out_sz, blocks, nt = r            # scans: [the scan records] of progressive files, else []
    total, most, pixels = int(blocks.sum()), int(blocks.max()), int((recs["width"].astype(np.int64) * recs["height"]).max())
    name = "clipmi_jpeg_decode_" + ("progressive_" if progressive else "") + ("transform_" if fused else "") + ("cmyk8" if cmyk else "rgb8")
    ws_bytes = int(L.clipmi_jpeg_progressive_workspace_bytes(len(recs), total, nt) if progressive else L.clipmi_jpeg_workspace_bytes(total, nt))

    def decode(base, sb, offs, rgb, status, ws, stream, tr):
        head = (sb + offs[1], len(scans[0]), sb + offs[2]) if progressive else (sb + offs[1],)
        # the fused entries take the transform's arguments (the jobs' coefficient offsets count from the segment's start, as for the
        # resize entry) where the others take max_pixels and the RGB rows
        mid = (sb + offs[-1], tr.max_rows, base, tr.n_px, tr.out, tr.scratch) if fused else (pixels, rgb)
        return getattr(L, name)(base, sb, len(recs), *head, nt, total, most, *mid, status, ws, ws_bytes, stream)

    return [recs, *scans, tables, jobs], out_sz, ws_bytes, name, decode


def _png_group(L, r, entry="clipmi_png_decode_rgb8", workspace="clipmi_png_workspace_bytes"):
    recs, jobs, out_sz, raw_sz = r
    total, most = int(raw_sz.sum()), int(raw_sz.max())
    if entry == "clipmi_png_decode_rgb8" and (recs["reserved"][:, 0] & 0xffff).any():      # 16-bit RGB files (png_records): the other entry
        if not (recs["reserved"][:, 0] & 0xffff).all():
            raise ValueError("a group of KIND_PNG files mixes 8-bit and 16-bit files")
        entry, workspace = "clipmi_png_decode_px8", "clipmi_png_px8_workspace_bytes"
    ws_bytes = int(getattr(L, workspace)(len(recs), total))

    def decode(base, sb, offs, rgb, status, ws, stream, tr):
        return getattr(L, entry)(base, sb, len(recs), total, most, rgb, status, ws, ws_bytes, stream)

    return [recs, jobs], out_sz, ws_bytes, entry, decode


class Format(NamedTuple):
    """What differs between the parsed kinds in DeviceStage, by decode_worker.Kind.kind"""
    records: Callable        # (bigview, n, cap, slots, comp, n_px) -> the kind's records out of the regions
    decoder_bytes: Callable  # headers -> bytes of HBM a file's decoder needs beside its decoded and the resize's rows (coefficients; scanlines)
    group: Callable          # a group builder, see above
    px: int                  # the bytes per decoded pixel
    entry: Optional[str]     # the transform entry that takes them; None: the decode entry transforms too (no full-size rows)

    @property
    def tmp_px(self):
        """Scratch bytes per pixel of the rows between the resize's passes (clipmi_nearest_crop_p8 needs no scratch rows)"""
        return 0 if self.entry == "clipmi_nearest_crop_p8" else self.px


_png_px8_group = partial(_png_group, entry="clipmi_png_decode_px8", workspace="clipmi_png_px8_workspace_bytes")
_FORMATS = {KIND_BASELINE: Format(jpeg_records, lambda hd: hd[:, HDR.BLOCKS] * 192, _jpeg_group, 3, "clipmi_resize_crop_rgb8"),
            KIND_PROGRESSIVE: Format(progressive_records, lambda hd: hd[:, HDR.BLOCKS] * 192, partial(_jpeg_group, progressive=True), 3,
                                     "clipmi_resize_crop_rgb8"),
            KIND_PNG: Format(png_records, _png_scanlines, _png_group, 3, "clipmi_resize_crop_rgb8"),
            KIND_PNG_ALPHA: Format(partial(png_records, px=4), partial(_png_scanlines, px=4), _png_px8_group, 4, "clipmi_resize_crop_rgba8"),
            KIND_PNG_INDEX: Format(partial(png_records, px=1), partial(_png_scanlines, px=1), _png_px8_group, 1, "clipmi_nearest_crop_p8")}


# With jpeg_fused the two JPEG kinds go through the entries that decode and transform in one call (transform entry None: the
# decode entry's call did it): no full-size RGB rows exist for them.
_FUSED_FORMATS = {KIND_BASELINE: _FORMATS[KIND_BASELINE]._replace(group=partial(_jpeg_group, fused=True), entry=None),
                  KIND_PROGRESSIVE: _FORMATS[KIND_PROGRESSIVE]._replace(group=partial(_jpeg_group, progressive=True, fused=True), entry=None)}


def formats(jpeg_fused=False):
    """_FORMATS, with the fused rows in place of the two JPEG kinds' when jpeg_fused"""
    return {**_FORMATS, **_FUSED_FORMATS} if jpeg_fused else _FORMATS


# The kinds of decode_worker.PARSED_MORE: four-component JPEG files decode to CMYK rows (jpeg_records(nc=4), clipmi_jpeg_decode_cmyk8)
# and clipmi_resize_crop_cmyk8 transforms them - with jpeg_fused too: the fused entries do not take four components.
cmyk_records = partial(jpeg_records, nc=4)
_cmyk_group = partial(_jpeg_group, cmyk=True)
_MORE_FORMATS = {KIND_JPEG_CMYK: Format(cmyk_records, lambda hd: hd[:, HDR.BLOCKS] * 192, _cmyk_group, 4, "clipmi_resize_crop_cmyk8")}


def all_formats(jpeg_fused=False):
    """formats(jpeg_fused) and the rows of the kinds added behind them: one row per kind of decode_worker.ALL_PARSED"""
    return {**formats(jpeg_fused), **_MORE_FORMATS}


def jpeg_fused_default():
    """$CLIPMI_DEVICE_JPEG_FUSED ("1" = on), off when unset"""
    import os
    return os.environ.get("CLIPMI_DEVICE_JPEG_FUSED", "0") not in ("", "0")


def jpeg_cmyk_default():
    """$CLIPMI_DEVICE_JPEG_CMYK ("1" = on), off when unset"""
    import os
    return os.environ.get("CLIPMI_DEVICE_JPEG_CMYK", "0") not in ("", "0")


def jpeg_layouts_default():
    """$CLIPMI_DEVICE_JPEG_LAYOUTS ("1" = on), off when unset"""
    import os
    return os.environ.get("CLIPMI_DEVICE_JPEG_LAYOUTS", "0") not in ("", "0")


def file_need(hd, fmt, n_px):
    """Bytes of HBM each file of one kind needs while its group is decoded, out of the region headers hd ([n][JPEG_HDR_INTS]) and the
    kind's row fmt of formats(): what its decoder needs, its full-size decoded rows (none where the decode entry transforms too)
    and the rows between the resize's two passes. DeviceStage sizes its groups by it."""
    rows = 0 if fmt.entry is None else (hd[:, HDR.W] * hd[:, HDR.H] * fmt.px + 15) // 16 * 16
    return fmt.decoder_bytes(hd) + rows + hd[:, HDR.NROWS] * n_px * fmt.tmp_px


class PinnedRing:
    """Three pinned staging buffers used in turn: batch i may still be in its H2D copy while batch i+1 is filled; a buffer is
    reused only after the copy that read it has finished (whoever starts the copy leaves its event in the slot's ev).
    alloc(n): a pinned tensor with room for n items along its first axis - a slot's buf, and np the same bytes as a numpy array."""

    def __init__(self, alloc):
        self.alloc, self.slots = alloc, []

    def take(self, n):
        slot = self.slots.pop(0) if len(self.slots) >= 3 else SimpleNamespace(buf=None, np=None, ev=None)
        if slot.ev is not None:
            slot.ev.synchronize()
        if slot.buf is None or slot.buf.shape[0] < n:
            slot.buf = self.alloc(n)
            slot.np = slot.buf.numpy()
        self.slots.append(slot)
        return slot


class Pending:
    """What the consumer checks behind a batch's encode step, and what has to live until then"""
    __slots__ = ("keep", "status", "slots", "count_ok", "chunk", "good", "layout_files", "interlaced", "chunked", "deep")

    def __init__(self):
        self.keep = []           # device tensors the queued kernels read and write
        self.status = None       # int32 device tensor: the decoders' per-file status, the kinds in ALL_PARSED's order (None: no parsed file)
        self.slots = None        # the slot of each status
        self.count_ok = []       # (stats key, lo, hi): ranges of `status` whose zeros count as files the device decoded
        self.chunk = self.good = None      # the batch's paths and its mask of good slots, for the files that go back to Pillow
        self.layout_files = 0    # staged JPEG files that only the layouts switch lets through (HDR.LAYOUT; decode_worker.LAYOUTS_STAT)
        self.interlaced = None   # bool per status: an Adam7 PNG file (HDR.INTERLACE; decode_worker.PNG_INTERLACED_STAT)
        self.chunked = None      # bool per status: a PNG file with metadata chunks (HDR.CHUNKS; decode_worker.PNG_CHUNKS_STAT)
        self.deep = None         # bool per status: a 16-bit PNG file (HDR.DEPTH; decode_worker.PNG_DEEP_STAT)


# One group of a kind's files: its packed arrays on the device and their offsets, its files, its largest nrows, its decode entry's name
# and call (see _jpeg_group), where its statuses start in the batch's tensor (bytes)
GroupCall = namedtuple("GroupCall", "dsmall offs n_files max_rows name decode status_off")
# The decodes and transforms of a batch's files of one kind, ready for the side stream: the groups run one after the other through one
# workspace, one buffer of decoded rows (None: the decode entry transforms too) and one of scratch rows; layout_files: how many of the
# files only the layouts switch lets through (HDR.LAYOUT, 0 in a PNG region); interlaced: which of the files are Adam7 PNG files
# (HDR.INTERLACE, 0 in a JPEG region), bool per file; chunked, deep: likewise HDR.CHUNKS and the 16-bit PNG files (_png_deep)
KindLaunch = namedtuple("KindLaunch", "fmt calls ws rgb scratch layout_files interlaced chunked deep", defaults=(0, None, None, None))


class DeviceStage:
    """The batch's regions of the big segment -> their rows of the batch's tensor (run). pool: the DecodePool that owns the
    segments; group_bytes: the HBM a group of parsed files may need (file_need); formats: all_formats()'s table."""

    def __init__(self, pool, dev, copy_stream, n_px, group_bytes, formats):
        self.pool, self.dev, self.copy_stream, self.n_px, self.group_bytes, self.formats = pool, dev, copy_stream, n_px, group_bytes, formats
        self.L = _lib.lib()
        self.ring = PinnedRing(lambda nbytes: torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8).pin_memory())

    def _resize(self, base, devt, src_ptr, jobs_ptr, n_jobs, max_rows, scratch, entry="clipmi_resize_crop_rgb8"):
        if entry == "clipmi_nearest_crop_p8":
            rc = self.L.clipmi_nearest_crop_p8(src_ptr, jobs_ptr, n_jobs, base, self.n_px, devt.data_ptr(), _lib.stream_ptr(self.dev))
        else:
            rc = getattr(self.L, entry)(src_ptr, jobs_ptr, n_jobs, max_rows, base, self.n_px, devt.data_ptr(), scratch.data_ptr(),
                                        _lib.stream_ptr(self.dev))
        _lib.check(rc, entry)

    def _stage_full(self, bigview, full, e2, cap, comp):
        """decode_full's regions [pixels | pad to 16 | PLAN_INTS header: w h, the plan, n_hcoef n_vcoef | coefficient blocks] -> (their
        resize jobs on the device, the scratch rows, the largest nrows)"""
        n_px = self.n_px
        wh = np.array([full[s_][1:3] for s_ in e2], dtype=np.int64)
        o_hdr = e2 * cap + (wh[:, 0] * wh[:, 1] * 3 + 15) // 16 * 16
        hd = np.stack([np.frombuffer(bigview, dtype=np.int32, count=PLAN_INTS, offset=int(o)) for o in o_hdr]).astype(np.int64)
        jobs = _resize_jobs(e2 * cap, wh[:, 0], wh[:, 1], hd[:, 2:10], hd[:, 10], o_hdr // 4 + PLAN_INTS, comp[e2], n_px)
        djobs = torch.from_numpy(jobs.view(np.uint8).reshape(-1).copy()).to(self.dev)
        scratch = torch.empty(max(int((hd[:, 3] * n_px * 3).sum()), 1), dtype=torch.uint8, device=self.dev)
        return djobs, scratch, max(1, int(hd[:, 3].max()))

    def _stage_kind(self, fmt, bigview, n, cap, slots, comp, status_at):
        """Groups of files whose decoded form (for JPEG coefficients, sample planes, RGB rows: ~22 bytes per pixel; for PNG
        scanlines and RGB rows) fits a budget: a batch of thumbnails is one group, a batch of 12-megapixel photos many -
        they run one after the other through ONE workspace per kind (the side stream is in order), so that HBM holds a
        group, not a batch, of decoded photos. status_at: where this kind's statuses start in the batch's tensor."""
        n_px, dev = self.n_px, self.dev
        hd = _headers(bigview, n, cap, slots)
        calls, ws_max, rgb_max, tmp_max = [], 0, 0, 0
        for lo, hi in _split(_groups(file_need(hd, fmt, n_px), self.group_bytes), _png_deep(hd)):
            arrays, out_sz, ws_bytes, name, decode = fmt.group(self.L, fmt.records(bigview, n, cap, slots[lo:hi], comp, n_px))
            small, offs = _pack16(arrays)
            dsmall = torch.from_numpy(small).to(dev)
            nrows = hd[lo:hi, HDR.NROWS]
            ws_max, rgb_max = max(ws_max, ws_bytes), max(rgb_max, int(out_sz.sum()) if fmt.entry is not None else 0)
            tmp_max = max(tmp_max, int((nrows * n_px * fmt.tmp_px).sum()))
            calls.append(GroupCall(dsmall, offs, hi - lo, int(nrows.max()), name, decode, 4 * (status_at + lo)))
        ws = torch.empty(ws_max, dtype=torch.uint8, device=dev)
        rgb = torch.empty(max(rgb_max, 16), dtype=torch.uint8, device=dev) if fmt.entry is not None else None
        scratch = torch.empty(max(tmp_max, 1), dtype=torch.uint8, device=dev)
        return KindLaunch(fmt, calls, ws, rgb, scratch, int(hd[:, HDR.LAYOUT].sum()), hd[:, HDR.INTERLACE] != 0,
                          hd[:, HDR.CHUNKS] != 0, _png_deep(hd))

    def _launch_kind(self, k, base, devt, status):
        for c in k.calls:
            sb = c.dsmall.data_ptr()
            tr = Transform(c.max_rows, self.n_px, devt.data_ptr(), k.scratch.data_ptr())
            rgb = k.rgb.data_ptr() if k.rgb is not None else None
            _lib.check(c.decode(base, sb, c.offs, rgb, status.data_ptr() + c.status_off, k.ws.data_ptr(), _lib.stream_ptr(self.dev), tr),
                       c.name)
            if k.fmt.entry is not None:                      # (None: the decode entry transformed too)
                self._resize(base, devt, rgb, sb + c.offs[-1], c.n_files, c.max_rows, k.scratch, k.fmt.entry)

    def run(self, devt, bigview, full, good, seg_index):
        """The regions of the batch in segment 2 + seg_index (bigview; full: slot -> (kind, w, h, bytes); good: the batch's mask) ->
        their rows of devt, on the copy stream behind devt's own copy: ONE H2D copy of the segment where it lies (it is page-locked:
        no packing copy on the host - packing 1 GB per batch of photo-sized images with one thread was slower than Pillow's resize),
        then clipmi_resize_crop_rgb8 for the full-size images (decode_worker.FULL_SIZE) and, for each kind of parsed file in
        decode_worker.ALL_PARSED's order, its decode entry and its transform entry (the kind's Format).
        The copy stream carries the copies only; the kernels go to the process's ONE side stream (_lib.side_stream: this ROCm gives a
        process three hardware queues) behind an event, so that the next batch's copy runs beside this batch's kernels instead of
        behind them, and the consumer finds them queued in front of its encode step.
        -> (event behind the kernels, Pending: what the consumer checks afterwards, whether the segment was copied in place).
        Where the segment could not be page-locked (locked-memory limit?) the batch goes through a pinned copy of it, and the caller
        lets the following ones take the host path. Returns when the segment has been copied (it is decoded into again two batches
        later)."""
        dev = self.dev
        n = len(good)
        comp = np.cumsum(good) - 1                           # slot -> row of devt
        cap = bigview.size // n
        used = (max(full) + 1) * cap
        e2 = np.array(sorted(s_ for s_, v in full.items() if v[0] == FULL_SIZE.kind), dtype=np.int64)
        parsed = [np.array(sorted(s_ for s_, v in full.items() if v[0] == k.kind), dtype=np.int64) for k in ALL_PARSED]
        # a kind's 16-bit PNG files behind its others, so that _split cuts a kind's groups once (a no-op without such files)
        parsed = [slots[np.argsort(_png_deep(_headers(bigview, n, cap, slots)), kind="stable")] if len(slots) and k.magic == "png" else slots
                  for k, slots in zip(ALL_PARSED, parsed)]
        n_status = sum(len(slots) for slots in parsed)      # one status tensor: the kinds in ALL_PARSED's order
        in_place = self.pool.pin_segment(2 + seg_index)
        if in_place:
            slot = None
            src = torch.from_numpy(bigview[:used])
        else:
            slot = self.ring.take(used)
            np.copyto(slot.np[:used], bigview[:used])
            src = slot.buf[:used]
        pending = Pending()
        kind_launches = []
        with torch.cuda.stream(self.copy_stream):
            dbig = src.to(dev, non_blocking=True)
            base = dbig.data_ptr()
            if n_status:
                pending.status = torch.empty(n_status, dtype=torch.int32, device=dev)
                pending.slots = np.concatenate(parsed)
                pending.interlaced = np.zeros(n_status, dtype=bool)
                pending.chunked, pending.deep = np.zeros(n_status, dtype=bool), np.zeros(n_status, dtype=bool)
            if len(e2):
                djobs, scratch, max_rows = self._stage_full(bigview, full, e2, cap, comp)
                pending.keep += [djobs, scratch]
            status_at = 0
            for kind, slots in zip(ALL_PARSED, parsed):      # the kinds follow each other on the side stream in ALL_PARSED's order
                if not len(slots):
                    continue
                k = self._stage_kind(self.formats[kind.kind], bigview, n, cap, slots, comp, status_at)
                kind_launches.append(k)
                pending.layout_files += k.layout_files
                pending.interlaced[status_at:status_at + len(slots)] = k.interlaced
                pending.chunked[status_at:status_at + len(slots)] = k.chunked
                pending.deep[status_at:status_at + len(slots)] = k.deep
                pending.keep += [c.dsmall for c in k.calls] + [k.ws, k.rgb, k.scratch]
                if kind.counts == "decoded":
                    pending.count_ok.append((kind.stat, status_at, status_at + len(slots)))
                status_at += len(slots)
            ev_copy = torch.cuda.Event()
            ev_copy.record(self.copy_stream)
        side = _lib.side_stream(dev)[1]
        with torch.cuda.stream(side):
            side.wait_event(ev_copy)
            if len(e2):
                self._resize(base, devt, base, djobs.data_ptr(), len(e2), max_rows, scratch)
            for k in kind_launches:
                self._launch_kind(k, base, devt, pending.status)
            ev = torch.cuda.Event()
            ev.record(side)
        ev_copy.synchronize()                                 # the segment is decoded into again two batches later
        pending.keep.append(dbig)
        if slot is not None:
            slot.ev = ev_copy
        return ev, pending, in_place
