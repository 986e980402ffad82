"""Marker walk of a baseline JPEG file for the device decoder (csrc/jpeg.hip; SURVEY.md §8(f) next-1, reference
build-index.py:47). numpy only - the decode workers (decode_worker.py) import this file by path, without torch.

`parse` lets through what the device decodes - 8-bit baseline / extended-sequential Huffman, one interleaved scan, grey or
YCbCr with luma sampling 1x1 / 2x1 / 2x2 and 1x1 chroma, with or without restart intervals - and raises `Unsupported` for
everything else (progressive, CMYK / RGB-coded, 12-bit, arithmetic coding, odd sampling, not a JPEG) and every header libjpeg or
Pillow refuses (a marker either does not know, a second SOI, sampling factors outside 1..4, Huffman codes that overflow their
lengths, more than JPEG_MAX_DIMENSION or Pillow's decompression-bomb limit of pixels): those files stay with Pillow.
That is a choice of decoder per file format, made on the host from the file's own header.

`layouts=True` (both parsers; opt-in, encode_files(device_jpeg_layouts=True)) also lets through YCbCr files with luma sampling
1x2 (4:4:0), 4x1 (4:1:1) or 1x4 and 1x1 chroma, and the three-component files libjpeg takes for RGB-coded (no JFIF marker and an
Adobe marker with transform 0 or the component ids R, G, B) at any luma sampling the device takes: `transform` = 1 in the record,
the three upsampled planes are the pixels. Luma 4x2, 2x4, a factor of 3 and subsampled luma stay refused.

`cmyk=True` (`parse` only; opt-in, encode_files(device_jpeg_cmyk=True)) also lets through four-component files whose components
1-3 are sampled 1x1 and whose component 0 has a sampling the device takes (the LAYOUT_SAMPLINGS with layouts=True as well):
`ncomp` = 4, eight tables, `quant` [4][64], `transform` = 2 (CMYK as stored: no Adobe marker, or Adobe transform 0) or 3 (YCCK:
Adobe transform 2) - libjpeg's default_decompress_parms for four components, where a JFIF marker plays no part. Adobe transform
1, component 3 sampled like component 0 (IJG's own YCCK default) and progressive four-component files stay refused.
"""
import re

import numpy as np

TABLE_BYTES = 288          # a raw table: DHT's 16 counts + up to 256 symbols (zero padded to 272) + class (0 DC, 1 AC) + 15 zero bytes
MAX_STREAM = 1 << 28
MAX_INTERVALS = 1 << 16
_NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                     21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                     60, 61, 54, 47, 55, 62, 63])
_INV_NATURAL = np.argsort(_NATURAL)


_MARKER = re.compile(rb"\xff[^\x00]")
# Markers in front of the scan that the walk takes: SOF0/1, DHT, DQT, DRI, APP0-15, COM, SOS, and the other SOFn and DAC, which
# it refuses by name. Every one of them is in Pillow's JpegImagePlugin.MARKER and read by libjpeg's jdmarker.c read_markers; any
# other marker there - an unknown code, a second SOI, EOI, RSTn, DNL, JPG, JPGn - is an error for one of the two.
_KNOWN = frozenset([0xC0, 0xC1, 0xC4, 0xDA, 0xDB, 0xDD, 0xFE, *range(0xC2, 0xD0), *range(0xE0, 0xF0)]) - {0xC8}
MAX_DIMENSION = 65500          # jmorecfg.h JPEG_MAX_DIMENSION: libjpeg refuses a wider or taller frame (jdinput.c initial_setup)
MAX_PIXELS = 2 * 89478485      # 2 x PIL.Image.MAX_IMAGE_PIXELS: above it Image.open raises DecompressionBombError


class Unsupported(Exception):
    """Not a file for the device decoder; Pillow's path takes it."""


class Parsed:
    __slots__ = ("width", "height", "ncomp", "hs", "vs", "quant", "tables", "stream", "ri", "starts", "stuffed", "transform")
    # transform: the colour transform, 0 = YCbCr -> RGB (and grey), 1 = none: the components are R, G, B (parse(layouts=True) only);
    # 2 = CMYK as stored, 3 = YCCK (four components: parse(cmyk=True) only);
    # ri: restart interval in MCUs (0: none); starts: uint32 byte offsets into `stream` of the restart intervals (None without);
    # stuffed: 1 = `stream` is the file's segment as it is, 0xFF00 stuffing included (parse(keep_stuffing=True))

    def mcus(self):
        hs, vs = (self.hs, self.vs) if self.ncomp != 1 else (1, 1)
        return -(-self.width // (8 * hs)) * -(-self.height // (8 * vs))

    def blocks(self):
        return self.mcus() * (self.hs * self.vs + self.ncomp - 1 if self.ncomp != 1 else 1)


SAMPLINGS = ((1, 1), (2, 1), (2, 2))                 # luma sampling factors the device takes (chroma 1x1) ...
LAYOUT_SAMPLINGS = ((1, 2), (4, 1), (1, 4))          # ... and those `layouts=True` adds


def _sampling(comps, jfif, adobe, adobe_tf, width, layouts):
    """The two parsers' rule for a three-component frame, and `parse`'s for a four-component one -> (hs, vs, transform); raises
    Unsupported"""
    if len(comps) == 4:
        # jdapimin.c default_decompress_parms, four components: CMYK unless an Adobe marker says YCCK (a JFIF marker plays no part);
        # another transform value libjpeg warns about and takes for YCCK - Pillow's file
        tf = {0: 2, 2: 3}.get(adobe_tf if adobe else 0)
        if tf is None:
            raise Unsupported("Adobe transform of a four-component file")
    else:
        ids = (comps[0][0], comps[1][0], comps[2][0])
        # jdapimin.c default_decompress_parms: which three-component files are YCbCr
        ycc = True if jfif else (adobe_tf != 0) if adobe else ids != (0x52, 0x47, 0x42)
        if not ycc and not layouts:
            raise Unsupported("RGB-coded JPEG")
        tf = 0 if ycc else 1
    hs, vs = comps[0][1], comps[0][2]
    if any((h, v) != (1, 1) for _, h, v, _ in comps[1:]) or \
            (hs, vs) not in (SAMPLINGS + LAYOUT_SAMPLINGS if layouts else SAMPLINGS):
        raise Unsupported("sampling factors")
    if hs == 2 and (width + 1) // 2 <= 2:
        raise Unsupported("too narrow for fancy upsampling")
    return hs, vs, tf


def is_layout(p):
    """Whether `layouts=True` was needed for this record (Parsed or Progressive): the files the switch adds"""
    return (p.ncomp == 3 and p.transform != 0) or (p.ncomp != 1 and (p.hs, p.vs) in LAYOUT_SAMPLINGS)


def parse(data, keep_stuffing=False, layouts=False, cmyk=False):
    """JPEG file bytes -> Parsed (header fields, quantisation steps in natural order, the six Huffman tables a scan can
    name as raw 288-byte records, the entropy-coded segment without byte stuffing). Raises Unsupported.
    keep_stuffing: a file without restart intervals that ends with its EOI marker is only SLICED - the segment keeps its stuffing
    (Parsed.stuffed = 1) and the device removes it and looks for markers inside (csrc/jpeg.hip jpeg_unstuff_kernel): no pass over
    the data on the host at all.
    layouts: also take luma 1x2 / 4x1 / 1x4 and RGB-coded files (the module's docstring).
    cmyk: also take four-component files, CMYK as stored or YCCK (the module's docstring): eight tables, quant [4][64]."""
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise Unsupported("not a JPEG file")
    n = len(data)
    i = 2
    qt = {}
    huff = {}
    frame = None
    ri = 0
    jfif = adobe = False
    adobe_tf = 0
    while True:
        if i + 4 > n or data[i] != 0xFF:
            raise Unsupported("marker expected")
        m = data[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m not in _KNOWN:
            raise Unsupported("marker")
        L = (data[i + 2] << 8) | data[i + 3]
        if L < 2 or i + 2 + L > n:
            raise Unsupported("truncated segment")
        if m == 0xDB:
            k = i + 4
            while k < i + 2 + L:
                if data[k] >> 4 or (data[k] & 15) > 3 or k + 65 > i + 2 + L:
                    raise Unsupported("quantisation table")
                qt[data[k] & 15] = data[k + 1:k + 65]
                k += 65
        elif m == 0xC0 or m == 0xC1:
            if frame is not None or L < 11 or data[i + 4] != 8:
                raise Unsupported("frame header")
            nf = data[i + 9]
            if L != 8 + 3 * nf:
                raise Unsupported("frame header")
            frame = ((data[i + 5] << 8) | data[i + 6], (data[i + 7] << 8) | data[i + 8],
                     [(data[i + 10 + 3 * c], data[i + 11 + 3 * c] >> 4, data[i + 11 + 3 * c] & 15, data[i + 12 + 3 * c]) for c in range(nf)])
            # libjpeg: sampling factors 1..4 on every component, grey included (jdinput.c initial_setup), the size limit; Pillow:
            # the decompression-bomb limit - checked before anything is sized for the file
            if any(not (1 <= h <= 4 and 1 <= v <= 4) for _, h, v, _ in frame[2]) or len({c[0] for c in frame[2]}) != nf:
                raise Unsupported("frame header")
            if frame[0] > MAX_DIMENSION or frame[1] > MAX_DIMENSION or frame[0] * frame[1] > MAX_PIXELS:
                raise Unsupported("too many pixels")
        elif 0xC2 <= m <= 0xCF and m != 0xC4 and m != 0xC8 and m != 0xCC:
            raise Unsupported("not a baseline frame")
        elif m == 0xCC:
            raise Unsupported("arithmetic coding")
        elif m == 0xC4:
            k = i + 4
            while k < i + 2 + L:
                if k + 17 > i + 2 + L:
                    raise Unsupported("Huffman table")
                cnt = sum(data[k + 1:k + 17])
                if cnt > 256 or k + 17 + cnt > i + 2 + L or (data[k] >> 4) > 1 or (data[k] & 15) > 3:
                    raise Unsupported("Huffman table")
                if (data[k] >> 4) == 0 and cnt and max(data[k + 17:k + 17 + cnt]) > 15:
                    raise Unsupported("DC Huffman table")               # libjpeg refuses such a table (jdhuff.c)
                code = 0                                                # canonical codes: every length's last code fits its
                for l in range(1, 17):                                  # length and is not all ones (jdhuff.c
                    code += data[k + l]                                 # jpeg_make_d_derived_tbl)
                    if code >= 1 << l:
                        raise Unsupported("Huffman table")
                    code <<= 1
                huff[data[k]] = bytes(data[k + 1:k + 17 + cnt]).ljust(272, b"\0") + bytes([data[k] >> 4]) + b"\0" * 15
                k += 17 + cnt
        elif m == 0xDD:
            if L != 4:
                raise Unsupported("restart interval")
            ri = (data[i + 4] << 8) | data[i + 5]
        elif m == 0xE0 and L >= 16 and data[i + 4:i + 9] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and L >= 14 and data[i + 4:i + 9] == b"Adobe":
            adobe, adobe_tf = True, data[i + 15]
        elif m == 0xDA:
            break
        i += 2 + L
    if frame is None:
        raise Unsupported("no frame header")
    height, width, comps = frame
    nc = len(comps)
    if width == 0 or height == 0 or nc not in ((1, 3, 4) if cmyk else (1, 3)):
        raise Unsupported("frame")
    ns = data[i + 4]
    if ns != nc or L != 6 + 2 * ns or data[i + 5 + 2 * ns] != 0 or data[i + 6 + 2 * ns] != 63 or data[i + 7 + 2 * ns] != 0:
        raise Unsupported("scan header")
    out = Parsed()
    out.width, out.height, out.ncomp = width, height, nc
    tables = []
    quant = np.zeros((4 if nc == 4 else 3, 64), np.uint8)
    for c in range(nc):
        cid, td_ta = data[i + 5 + 2 * c], data[i + 6 + 2 * c]
        if cid != comps[c][0]:
            raise Unsupported("scan order")
        dc, ac = huff.get(td_ta >> 4), huff.get(0x10 | (td_ta & 15))
        q = qt.get(comps[c][3])
        if dc is None or ac is None or q is None:
            raise Unsupported("missing table")
        tables += [dc, ac]
        quant[c] = np.frombuffer(q, np.uint8)[_INV_NATURAL]
    while len(tables) < 6:
        tables += tables[:2]
    if nc != 1:
        out.hs, out.vs, out.transform = _sampling(comps, jfif, adobe, adobe_tf, width, layouts)
    else:
        out.hs, out.vs, out.transform = 1, 1, 0
    out.quant, out.tables = quant, tables
    # the entropy-coded segment ends at the first marker that is not a stuffed 0xFF00 (C-speed searches: a photo's segment
    # holds thousands of stuffed bytes)
    i += 2 + L
    out.ri, out.starts, out.stuffed = ri, None, 0
    if keep_stuffing and not ri and n - i >= 2 and data[n - 2] == 0xFF and data[n - 1] == 0xD9:
        j = n - 2
        while j > i and data[j - 1] == 0xFF:                 # fill bytes in front of EOI (a data 0xFF has its 0x00 behind it): not
            j -= 1                                           # the segment's - the device would take them for a marker inside it
        out.stream = data[i:j]
        out.stuffed = 1
    elif ri:
        # restart intervals: RSTn markers, numbered 0..7 in turn (jdmarker.c read_restart_marker), separate them; every
        # interval starts on a byte with fresh DC predictions - an independent chain for the device. The markers are dropped.
        want = -(-out.mcus() // ri)
        if want > MAX_INTERVALS:
            raise Unsupported("too many restart intervals")
        parts, count, seg = [], 0, i
        while True:
            m_ = _MARKER.search(data, seg)
            if m_ is None:
                raise Unsupported("no end of image")
            j = e = m_.start()
            while j + 1 < n and data[j + 1] == 0xFF:         # fill bytes in front of a marker: rare, walk them
                j += 1
            if j + 1 >= n:
                raise Unsupported("no end of image")
            nxt = data[j + 1]
            if nxt == 0:
                raise Unsupported("fill bytes inside the scan")
            if nxt == 0xD0 + (count & 7) and count + 1 < want:
                parts.append(data[seg:e].replace(b"\xff\x00", b"\xff"))
                count += 1
                seg = j + 2
                continue
            if nxt != 0xD9 or count + 1 != want:
                raise Unsupported("marker inside the scan")
            parts.append(data[seg:e].replace(b"\xff\x00", b"\xff"))
            break
        lens = np.fromiter((len(x) for x in parts), dtype=np.int64, count=len(parts))
        out.starts = (np.cumsum(lens) - lens).astype(np.uint32)
        out.stream = b"".join(parts)
    else:
        m_ = _MARKER.search(data, i)
        if m_ is None:
            raise Unsupported("no end of image")
        j = e = m_.start()
        nxt = data[j + 1]
        if nxt == 0xFF:                                      # fill bytes in front of a marker: rare, walk them
            while j + 1 < n and data[j + 1] == 0xFF:
                j += 1
            if j + 1 >= n:
                raise Unsupported("no end of image")
            nxt = data[j + 1]
            if nxt == 0:
                raise Unsupported("fill bytes inside the scan")
        if nxt != 0xD9:
            raise Unsupported("marker inside the scan")         # further scans
        out.stream = data[i:e].replace(b"\xff\x00", b"\xff")   # (the fill bytes are not the segment's)
    if len(out.stream) >= MAX_STREAM:
        raise Unsupported("too large")
    return out


MAX_SCANS = 100            # more scans than any encoder writes (libjpeg's richest script has 10; a file of 100+ is an attack)
MAX_WORK = 1 << 26         # coefficient steps of the device's serial walk: blocks x band width, summed over the scans. A 12-megapixel
                           # 4:2:0 photo in libjpeg's script takes ~48 M; above the bound the walk would keep a GPU busy for seconds
_BETWEEN = frozenset([0xC4, 0xDA, 0xFE, *range(0xE0, 0xF0)])          # markers a progressive file may hold between its scans


class Scan:
    __slots__ = ("comps", "ss", "se", "ah", "al", "dc", "ac", "stream")
    # comps: frame component indices, increasing; dc / ac: per scan component the 288-byte record of the table the scan decodes with
    # (DC first scans: dc; AC scans: ac; DC refinements read raw bits and name none - None); stream: the segment, stuffing removed


class Progressive:
    __slots__ = ("width", "height", "ncomp", "hs", "vs", "quant", "scans", "transform")      # transform: as Parsed's

    def mcus(self):
        hs, vs = (self.hs, self.vs) if self.ncomp == 3 else (1, 1)
        return -(-self.width // (8 * hs)) * -(-self.height // (8 * vs))

    def blocks(self):
        return self.mcus() * (self.hs * self.vs + 2 if self.ncomp == 3 else 1)


def _dht(data, k, end, huff):
    """DHT payload data[k:end] -> huff[class << 4 | id] = 288-byte record (the checks of parse)"""
    while k < end:
        if k + 17 > end:
            raise Unsupported("Huffman table")
        cnt = sum(data[k + 1:k + 17])
        if cnt > 256 or k + 17 + cnt > end or (data[k] >> 4) > 1 or (data[k] & 15) > 3:
            raise Unsupported("Huffman table")
        if (data[k] >> 4) == 0 and cnt and max(data[k + 17:k + 17 + cnt]) > 15:
            raise Unsupported("DC Huffman table")
        code = 0
        for l in range(1, 17):
            code += data[k + l]
            if code >= 1 << l:
                raise Unsupported("Huffman table")
            code <<= 1
        huff[data[k]] = bytes(data[k + 1:k + 17 + cnt]).ljust(272, b"\0") + bytes([data[k] >> 4]) + b"\0" * 15
        k += 17 + cnt


def parse_progressive(data, layouts=False):
    """Progressive JPEG file bytes -> Progressive (header fields, quantisation steps in natural order, the scans in file order
    with their own Huffman tables and segments). Raises Unsupported for every file the device decoder does not vouch for:
      * anything `parse` refuses in a frame header (marker whitelist, size and decompression-bomb limits, Huffman codes that
        overflow, the YCbCr / Adobe rule, grey or luma 1x1 / 2x1 / 2x2 with 1x1 chroma, too narrow for fancy upsampling;
        layouts=True widens the last two rules exactly as it does for `parse`);
      * a frame other than SOF2 (baseline files go to `parse`; SOF10 and the other arithmetic-coded frames stay with Pillow);
      * scan parameters libjpeg refuses (jdphuff.c start_pass_phuff_decoder: a DC scan with Se != 0, an AC scan of more than one
        component, Ss > Se, Se > 63, Al > 13, Ah neither 0 nor Al + 1) or only warns about (jdphuff.c: a "bogus progression" -
        an AC scan before the component's DC scan, a refinement whose Ah is not the bit its coefficient has reached, a first
        scan of a coefficient already coded);
      * an incomplete script - some coefficient of some component not at Al = 0 by EOI. libjpeg(-turbo) then applies block
        smoothing (jdcoefct.c smoothing_ok / decompress_smooth_data); a complete script decodes with plain jpeg_idct_islow;
      * restart intervals (DRI) anywhere in the file: not handled on the device for now;
      * DQT or DNL after the first SOS, a marker other than SOS, DHT, COM or APPn between scans, a missing EOI,
        more than MAX_SCANS scans, scan components out of frame order, a missing table;
      * more than MAX_WORK coefficient steps (blocks x band width, summed over the scans): the device walks each chain of
        scans serially, so the cost grows with pixels x bands x scans whatever the size of the data."""
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise Unsupported("not a JPEG file")
    n = len(data)
    i = 2
    qt, huff = {}, {}
    frame = None
    jfif = adobe = False
    adobe_tf = 0
    while True:                                              # the header, up to the first SOS
        if i + 4 > n or data[i] != 0xFF:
            raise Unsupported("marker expected")
        m = data[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m not in _KNOWN:
            raise Unsupported("marker")
        L = (data[i + 2] << 8) | data[i + 3]
        if L < 2 or i + 2 + L > n:
            raise Unsupported("truncated segment")
        if m == 0xDB:
            k = i + 4
            while k < i + 2 + L:
                if data[k] >> 4 or (data[k] & 15) > 3 or k + 65 > i + 2 + L:
                    raise Unsupported("quantisation table")
                qt[data[k] & 15] = data[k + 1:k + 65]
                k += 65
        elif m == 0xC2:
            if frame is not None or L < 11 or data[i + 4] != 8:
                raise Unsupported("frame header")
            nf = data[i + 9]
            if L != 8 + 3 * nf:
                raise Unsupported("frame header")
            frame = ((data[i + 5] << 8) | data[i + 6], (data[i + 7] << 8) | data[i + 8],
                     [(data[i + 10 + 3 * c], data[i + 11 + 3 * c] >> 4, data[i + 11 + 3 * c] & 15, data[i + 12 + 3 * c]) for c in range(nf)])
            if any(not (1 <= h <= 4 and 1 <= v <= 4) for _, h, v, _ in frame[2]) or len({c[0] for c in frame[2]}) != nf:
                raise Unsupported("frame header")
            if frame[0] > MAX_DIMENSION or frame[1] > MAX_DIMENSION or frame[0] * frame[1] > MAX_PIXELS:
                raise Unsupported("too many pixels")
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Unsupported("not a progressive Huffman frame")
        elif m == 0xCC:
            raise Unsupported("arithmetic coding")
        elif m == 0xC4:
            _dht(data, i + 4, i + 2 + L, huff)
        elif m == 0xDD:
            raise Unsupported("restart intervals in a progressive file")
        elif m == 0xE0 and L >= 16 and data[i + 4:i + 9] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and L >= 14 and data[i + 4:i + 9] == b"Adobe":
            adobe, adobe_tf = True, data[i + 15]
        elif m == 0xDA:
            break
        i += 2 + L
    if frame is None:
        raise Unsupported("no frame header")
    height, width, comps = frame
    nc = len(comps)
    if width == 0 or height == 0 or nc not in (1, 3):
        raise Unsupported("frame")
    out = Progressive()
    out.width, out.height, out.ncomp = width, height, nc
    if nc == 3:
        out.hs, out.vs, out.transform = _sampling(comps, jfif, adobe, adobe_tf, width, layouts)
    else:
        out.hs, out.vs, out.transform = 1, 1, 0
    quant = np.zeros((3, 64), np.uint8)
    for c in range(nc):
        q = qt.get(comps[c][3])
        if q is None:
            raise Unsupported("missing table")
        quant[c] = np.frombuffer(q, np.uint8)[_INV_NATURAL]
    out.quant = quant
    cid = {c[0]: k for k, c in enumerate(comps)}
    bits = [[-1] * 64 for _ in range(nc)]                  # jdphuff.c coef_bits: the bit each coefficient has reached (-1: none)
    scans = []
    while True:                                              # data[i] is an SOS marker here
        ns = data[i + 4] if i + 4 < n else 0
        if not 1 <= ns <= nc or L != 6 + 2 * ns:
            raise Unsupported("scan header")
        if len(scans) == MAX_SCANS:
            raise Unsupported("too many scans")
        s = Scan()
        idx = [cid.get(data[i + 5 + 2 * k], -1) for k in range(ns)]
        if min(idx) < 0 or any(a >= b for a, b in zip(idx, idx[1:])):
            raise Unsupported("scan components")
        s.comps = tuple(idx)
        s.ss, s.se = data[i + 5 + 2 * ns], data[i + 6 + 2 * ns]
        s.ah, s.al = data[i + 7 + 2 * ns] >> 4, data[i + 7 + 2 * ns] & 15
        if s.ss == 0:
            if s.se != 0:
                raise Unsupported("DC scan with Se != 0")
        elif s.se > 63 or s.ss > s.se or ns != 1:
            raise Unsupported("AC scan parameters")
        if s.al > 13 or (s.ah and s.al != s.ah - 1):
            raise Unsupported("successive approximation")
        for c in idx:
            b = bits[c]
            if s.ss and b[0] < 0:
                raise Unsupported("AC scan before the DC scan")
            for k in range(s.ss, s.se + 1):
                if (s.ah == 0 and b[k] >= 0) or (s.ah and b[k] != s.ah):
                    raise Unsupported("bogus progression")
                b[k] = s.al
        tabs = []
        for k in range(ns):
            td_ta = data[i + 6 + 2 * k]
            t = None if (s.ss == 0 and s.ah) else huff.get(td_ta >> 4) if s.ss == 0 else huff.get(0x10 | (td_ta & 15))
            if t is None and not (s.ss == 0 and s.ah):
                raise Unsupported("missing table")
            tabs.append(t)
        s.dc, s.ac = (tabs, None) if s.ss == 0 else (None, tabs)
        i += 2 + L
        m_ = _MARKER.search(data, i)
        if m_ is None:
            raise Unsupported("no end of image")
        j = m_.start()
        while data[j + 1] == 0xFF:                           # fill bytes in front of a marker
            j += 1
            if j + 1 >= n:
                raise Unsupported("no end of image")
        if data[j + 1] == 0:
            raise Unsupported("fill bytes inside the scan")
        s.stream = data[i:m_.start()].replace(b"\xff\x00", b"\xff")
        if len(s.stream) >= MAX_STREAM:
            raise Unsupported("too large")
        scans.append(s)
        i = j
        while True:                                          # the markers up to the next SOS or EOI
            if i + 2 > n or data[i] != 0xFF:
                raise Unsupported("marker expected")
            m = data[i + 1]
            if m == 0xFF:
                i += 1
                continue
            if m == 0xD9:
                break
            if m not in _BETWEEN:
                raise Unsupported("marker between scans")
            if i + 4 > n:
                raise Unsupported("truncated segment")
            L = (data[i + 2] << 8) | data[i + 3]
            if L < 2 or i + 2 + L > n:
                raise Unsupported("truncated segment")
            if m == 0xDA:
                break
            if m == 0xC4:
                _dht(data, i + 4, i + 2 + L, huff)
            i += 2 + L
        if m == 0xD9:
            break
    if any(b != 0 for row in bits for b in row):
        raise Unsupported("incomplete scan script (block smoothing)")
    blocks_of = [-(-width // 8) * -(-height // 8)] if nc == 1 else [
        -(-width // 8) * -(-height // 8), *[-(-(-(-width // out.hs)) // 8) * -(-(-(-height // out.vs)) // 8)] * 2]
    if sum(sum(blocks_of[c] for c in s.comps) * (s.se - s.ss + 1) for s in scans) > MAX_WORK:
        raise Unsupported("too much work for the serial walk")
    out.scans = scans
    return out
