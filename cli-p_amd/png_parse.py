"""Host side of the PNG decode on the device (csrc/png.hip): walk the chunks and hand over the DEFLATE stream.

`parse(data)` lets through 8-bit grey (colour type 0) and RGB (colour type 2) files that are not interlaced and carry no
`tRNS` and no APNG chunk (`parse(data, modes=True)` also RGBA, grey + alpha, palette files at depth 1/2/4/8, with or without
`tRNS`, and grey files at depth 1/2/4: kinds "alpha" and "index", see Parsed), and returns the IDAT payloads joined, without the 2-byte zlib header; the Adler-32 and anything
behind it stay in place (the device finds the trailer behind the final block itself). `parse(data, interlaced=True)` also lets
Adam7 files (interlace method 1) of the colour types and depths the other argument allows through: the same stream, whose
scanlines are those of the seven passes (adam7_passes), one pass after the other. Everything else raises `Unsupported`
and stays with Pillow: palette, alpha, 16-bit and 1/2/4-bit files (the transform resamples those modes differently), Adam7
files without that argument, and any file whose chunks this parser cannot vouch for - in front of the image data AND behind it: Pillow's load_end()
runs its chunk handlers on everything up to IEND, and a handler that raises there makes `convert("RGB")` fail although the
pixels are complete. Pure Python plus zlib.crc32, no Pillow: decode_worker.py imports it under both import forms, like jpeg_parse.
"""
import re
import struct
import zlib

SIGNATURE = b"\x89PNG\r\n\x1a\n"
# Pillow warns from this many pixels on (Image.MAX_IMAGE_PIXELS) and refuses at twice as many; such a file is Pillow's to judge.
# Below it the filtered data (height x (1 + width x channels) bytes) stays far under 2^31 - 1.
MAX_PIXELS = 89478485
MAX_TEXT_BYTES = 1 << 20
# The unfilter kernel keeps a band's last row in LDS (48 KiB): rows of up to this many pixels; wider files are Pillow's.
MAX_WIDTH = 16384
MAX_ROW_BYTES = 49152      # ... and, for the modes behind `modes=True`, of up to this many bytes: RGBA rows of at most 12288 pixels

# Chunks allowed in front of the first IDAT, with the length Pillow's handler needs (None: any), and why each can change
# neither mode nor size nor pixels of `Image.open(f).convert("RGB")` (PIL/PngImagePlugin.py, PngStream.chunk_*):
ALLOWED_BEFORE_IDAT = {
    b"gAMA": 4,      # stored as info["gamma"]; Pillow never applies a gamma (a shorter chunk would raise in i32)
    b"cHRM": 32,     # stored as info["chromaticity"] only
    b"sRGB": 1,      # stored as info["srgb"] only (an empty chunk raises "Truncated sRGB chunk")
    b"pHYs": 9,      # stored as info["dpi"] / info["aspect"]; no resampling follows from it
    b"tEXt": None,   # stored as info / text entries; Pillow refuses more than 64 MiB of text, so the total is capped here
    b"tIME": None,   # no handler: read, CRC checked and dropped
    b"sBIT": None,   # no handler: Pillow does not shift samples by the significant bits
    b"bKGD": None,   # no handler: there is no alpha to composite over a background in colour types 0 and 2
}
# Behind the IDAT run Pillow (load_end) checks no CRC, stops at IEND, at a chunk type that is not four word characters and
# where fewer than 8 bytes are left, skips chunks it has no handler for (if they fit the file) and calls its handler for the
# rest. Let through there: the chunks of the list above under the same length rule (their handlers raise on other lengths:
# "Truncated sRGB chunk", struct.error, ...; text counts towards the same cap) and chunks Pillow has no handler for. A chunk
# that runs past the end of the file ("Truncated File Read") and every other chunk with a handler are refused.
PILLOW_HANDLERS = (b"IHDR", b"IDAT", b"IEND", b"PLTE", b"tRNS", b"gAMA", b"cHRM", b"sRGB", b"pHYs", b"tEXt", b"zTXt", b"iTXt",
                   b"iCCP", b"eXIf", b"acTL", b"fcTL", b"fdAT")
_CID = re.compile(rb"\w\w\w\w")                                # Pillow's is_cid

# not in the list on purpose: PLTE / tRNS (change the mode or the pixels), iCCP / zTXt / iTXt (decompressed while opening, may
# raise), eXIf (kept as is, but an orientation tag is a caller's business), acTL / fcTL / fdAT (APNG), unknown chunks.


# Adam7: (x0, y0, dx, dy) of the seven passes in file order - pass p holds the pixels (x0 + i dx, y0 + j dy)
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def adam7_passes(width, height):
    """[(x0, y0, dx, dy, pw, ph)] of the seven passes of a width x height image: pass p is an image of pw x ph pixels of its own,
    pw = ceil((width - x0) / dx), ph likewise; a pass with pw == 0 or ph == 0 has no bytes in the file, not even filter bytes.
    width, height >= 1: ints, or integer numpy arrays (x0 < dx and y0 < dy, so the rounded-up quotients are never negative)."""
    return [(x0, y0, dx, dy, (width - x0 + dx - 1) // dx, (height - y0 + dy - 1) // dy) for x0, y0, dx, dy in ADAM7]


def adam7_raw_bytes(width, height, bits):
    """bytes of filtered scanlines of an Adam7 file whose pixels have `bits` bits: ph x (1 + ceil(pw x bits / 8)) over the
    non-empty passes. Ints, or integer numpy arrays (device_stage sizes a batch's files at once)."""
    return sum((pw > 0) * ph * (1 + (pw * bits + 7) // 8) for _, _, _, _, pw, ph in adam7_passes(width, height))


class Unsupported(Exception):
    """Not a file for the device decoder: Pillow decodes it (or reports it)."""


class Parsed:
    """kind: what the device decodes the file to - "rgb" (3 bytes per pixel, clipmi_png_decode_rgb8), "alpha" (4 bytes per pixel:
    RGBA, grey + alpha, grey at depth 2/4) or "index" (1 byte per pixel: palette files, 1-bit grey), both clipmi_png_decode_px8.
    channels: samples per pixel; palette: uint8 [256][3], zero beyond the n_entries entries (None for "rgb" and "alpha"; 1-bit grey
    is the two-entry palette black, white). interlace: 0, or 1 for an Adam7 file (parse(interlaced=True))."""
    __slots__ = ("width", "height", "channels", "stream", "kind", "depth", "ctype", "palette", "n_entries", "interlace")

    def __init__(self, width, height, channels, stream, kind="rgb", depth=8, ctype=None, palette=None, n_entries=0, interlace=0):
        self.width, self.height, self.channels, self.stream = width, height, channels, stream
        self.kind, self.depth, self.ctype = kind, depth, (2 if channels == 3 else 0) if ctype is None else ctype
        self.palette, self.n_entries, self.interlace = palette, n_entries, interlace

    def row_bytes(self):
        """bytes of a full row of the image without its filter byte (no pass row of an Adam7 file is longer)"""
        return (self.width * self.channels * self.depth + 7) // 8

    def raw_bytes(self):
        """size of the filtered scanlines the stream has to produce"""
        if self.interlace:
            return adam7_raw_bytes(self.width, self.height, self.channels * self.depth)
        return self.height * (1 + self.row_bytes())


# colour type -> (samples per pixel, the depths taken under modes=True); 16-bit files stay Pillow's
_MODES = {6: (4, (8,)), 4: (2, (8,)), 3: (1, (1, 2, 4, 8)), 0: (1, (1, 2, 4))}


def _palette(body, n_entries):
    import numpy as np
    pal = np.zeros((256, 3), np.uint8)
    pal[:n_entries] = np.frombuffer(body, np.uint8).reshape(n_entries, 3)
    return pal


def parse(data, modes=False, interlaced=False):
    """PNG file contents -> Parsed; raises Unsupported(reason). modes: also let the files of kinds "alpha" and "index" through.
    interlaced: also let Adam7 files (interlace method 1) of the colour types and depths let through anyway through."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise Unsupported("not a PNG file")
    pos, n = 8, len(data)
    first = True
    text = 0
    pieces = None
    plte = None                                                # the PLTE chunk's body (colour type 3 under modes=True)
    seen_trns = False
    while True:
        if pos + 8 > n:
            if pieces is not None:
                break                                          # Pillow reads no further than the image data: no IEND is fine
            raise Unsupported("file ends before the image data")
        length, cid = struct.unpack_from(">I4s", data, pos)
        body = pos + 8
        if pieces is not None:
            if cid != b"IDAT":
                break                                          # the IDAT run is over; Pillow stops reading here as well
            if body + length > n:
                raise Unsupported("IDAT chunk runs past the end of the file")
            pieces.append(data[body:body + length])            # (CRC not checked: Pillow does not, the Adler-32 guards the data)
            pos = body + length + 4
            continue
        if body + length + 4 > n:
            raise Unsupported("chunk runs past the end of the file")
        if cid == b"IDAT":
            if first:
                raise Unsupported("IDAT before IHDR")
            pieces = []
            continue
        if zlib.crc32(data[pos + 4:body + length]) != struct.unpack_from(">I", data, body + length)[0]:
            raise Unsupported("bad CRC in %r" % cid)
        if first:
            if cid != b"IHDR" or length != 13:
                raise Unsupported("IHDR is not the first chunk")
            width, height, depth, ctype, comp, filt, lace = struct.unpack_from(">IIBBBBB", data, body)
            rgb = depth == 8 and ctype in (0, 2)
            if not rgb and not (modes and ctype in _MODES and depth in _MODES[ctype][1]):
                raise Unsupported("bit depth %d, colour type %d" % (depth, ctype))
            if comp != 0 or filt != 0:
                raise Unsupported("unknown compression or filter method")
            if lace != 0 and not (interlaced and lace == 1):
                raise Unsupported("interlaced")
            if width < 1 or height < 1:
                raise Unsupported("empty image")
            if width * height > MAX_PIXELS:
                raise Unsupported("too many pixels")
            if width > MAX_WIDTH:
                raise Unsupported("rows too wide")
            channels = (3 if ctype == 2 else 1) if rgb else _MODES[ctype][0]
            if (width * channels * depth + 7) // 8 > MAX_ROW_BYTES:
                raise Unsupported("rows too wide")
            first = False
        elif not rgb and ctype == 3 and cid == b"PLTE":
            # exactly one, 1 .. 1 << depth whole entries (Pillow takes the palette as it comes; a longer one is its to judge)
            if plte is not None or seen_trns or length % 3 or not 3 <= length <= 768 or length > 3 << depth:
                raise Unsupported("PLTE chunk")
            plte = data[body:body + length]
        elif not rgb and ctype == 3 and cid == b"tRNS":
            # behind the palette, at most one alpha per entry: it sets info["transparency"] and changes no pixel of convert("RGB")
            if plte is None or seen_trns or length > len(plte) // 3:
                raise Unsupported("tRNS chunk")
            seen_trns = True
        else:
            want = ALLOWED_BEFORE_IDAT.get(cid, -1)
            if want == -1 or (want is not None and length != want):
                raise Unsupported("chunk %r in front of the image data" % cid)
            if cid == b"tEXt":
                text += length
                if text > MAX_TEXT_BYTES:
                    raise Unsupported("too much text")
        pos = body + length + 4
    # behind the IDAT run: what Pillow's load_end() walks (see PILLOW_HANDLERS above)
    while pos + 8 <= n:
        length, cid = struct.unpack_from(">I4s", data, pos)
        if not _CID.fullmatch(cid) or cid == b"IEND":
            break                                              # Pillow stops reading here
        if pos + 8 + length > n:
            raise Unsupported("chunk %r behind the image data runs past the end of the file" % cid)
        want = ALLOWED_BEFORE_IDAT.get(cid, -1)
        if want == -1:
            if cid in PILLOW_HANDLERS:
                raise Unsupported("chunk %r behind the image data" % cid)
        elif want is not None and length != want:
            raise Unsupported("chunk %r of %d bytes behind the image data" % (cid, length))
        if cid == b"tEXt":
            text += length
            if text > MAX_TEXT_BYTES:
                raise Unsupported("too much text")
        pos += 12 + length
    stream = b"".join(pieces)
    if len(stream) < 2:
        raise Unsupported("no zlib header")
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf * 256 + flg) % 31 or flg & 0x20:
        raise Unsupported("bad zlib header")
    if len(stream) - 2 >= 1 << 31:
        raise Unsupported("stream too large")
    if rgb:
        return Parsed(width, height, channels, stream[2:], interlace=lace)
    if ctype == 3:
        if plte is None:
            raise Unsupported("no PLTE chunk")
        return Parsed(width, height, 1, stream[2:], "index", depth, 3, _palette(plte, len(plte) // 3), len(plte) // 3, interlace=lace)
    if ctype == 0 and depth == 1:
        return Parsed(width, height, 1, stream[2:], "index", 1, 0, _palette(b"\0\0\0\xff\xff\xff", 2), 2, interlace=lace)
    return Parsed(width, height, channels, stream[2:], "alpha", depth, ctype, interlace=lace)
