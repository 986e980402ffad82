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

`parse(data, chunks=True)` also lets the metadata chunks through that change no pixel of the transform, each under the rule its
handler in Pillow sets (METADATA_CHUNKS, _metadata): iCCP, zTXt, iTXt, eXIf, tRNS on 8-bit grey and on RGB files, and every chunk
Pillow has no handler for. The compressed ones are inflated here, bounded like Pillow's (a few KB of zlib per file).
`parse(data, deep=True)` also lets files of depth 16 through: RGB (kind "rgb", depth 16), and with `modes=True` RGBA and grey +
alpha (kind "alpha", depth 16). Pillow opens them as RGB / RGBA / RGBA (L L L A) made of every sample's high byte, and so does
the device. Two things stay Pillow's whatever is switched on: 16-bit grey (colour type 0 at depth 16), which Pillow opens as
I;16, resamples in 16 bits and clips to 255 in convert("RGB") - another resampler, not the high bytes' -, and tRNS on the alpha
colour types and on grey below depth 8.
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
# What chunks=True adds (the chunks with a handler among them): see _metadata for each one's rule
METADATA_CHUNKS = (b"iCCP", b"zTXt", b"iTXt", b"eXIf", b"tRNS")
MAX_TEXT_CHUNK = 1 << 20   # PngImagePlugin.MAX_TEXT_CHUNK: _safe_zlib_decompress raises "Decompressed data too large" beyond it

# not in the list on purpose: PLTE / tRNS (change the mode or the pixels), iCCP / zTXt / iTXt (decompressed while opening, may
# raise), eXIf (kept as is, but an orientation tag is a caller's business), acTL / fcTL / fdAT (APNG), unknown chunks.
# parse(chunks=True) takes iCCP / zTXt / iTXt / eXIf, tRNS on 8-bit grey and RGB and the unknown ones under rules of their own.


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
    is the two-entry palette black, white). interlace: 0, or 1 for an Adam7 file (parse(interlaced=True)). depth: 16 for the files
    of parse(deep=True) - RGB stays kind "rgb", RGBA and grey + alpha kind "alpha": the device leaves the samples' high bytes."""
    __slots__ = ("width", "height", "channels", "stream", "kind", "depth", "ctype", "palette", "n_entries", "interlace", "chunks")

    def __init__(self, width, height, channels, stream, kind="rgb", depth=8, ctype=None, palette=None, n_entries=0, interlace=0,
                 chunks=0):
        self.width, self.height, self.channels, self.stream = width, height, channels, stream
        self.kind, self.depth, self.ctype = kind, depth, (2 if channels == 3 else 0) if ctype is None else ctype
        self.palette, self.n_entries, self.interlace = palette, n_entries, interlace
        self.chunks = chunks                                   # 1: the file holds a chunk that only parse(chunks=True) lets through

    @property
    def px8(self):
        """whether clipmi_png_decode_px8 decodes the file (clipmi_png_decode_rgb8 takes 8-bit grey and RGB only): the kinds "alpha"
        and "index", and 16-bit RGB, which is of kind "rgb" for what the device leaves (3 bytes per pixel)"""
        return self.kind != "rgb" or self.depth == 16

    def row_bytes(self):
        """bytes of a full row of the image without its filter byte (no pass row of an Adam7 file is longer)"""
        return (self.width * self.channels * self.depth + 7) // 8

    def raw_bytes(self):
        """size of the filtered scanlines the stream has to produce"""
        if self.interlace:
            return adam7_raw_bytes(self.width, self.height, self.channels * self.depth)
        return self.height * (1 + self.row_bytes())


# colour type -> (samples per pixel, the depths taken under modes=True); 16-bit files are deep=True's
_MODES = {6: (4, (8,)), 4: (2, (8,)), 3: (1, (1, 2, 4, 8)), 0: (1, (1, 2, 4))}
# colour type -> samples per pixel of the depth-16 files deep=True takes (4 and 6 under modes=True only); not colour type 0: Pillow
# opens 16-bit grey as I;16 and resamples it in 16 bits
_DEEP = {2: 3, 6: 4, 4: 2}


def _palette(body, n_entries):
    import numpy as np
    pal = np.zeros((256, 3), np.uint8)
    pal[:n_entries] = np.frombuffer(body, np.uint8).reshape(n_entries, 3)
    return pal


def _inflated(z):
    """Bytes that PngImagePlugin._safe_zlib_decompress makes of z: decompressobj().decompress(z, MAX_TEXT_CHUNK), "Decompressed data
    too large" where input is left over at the cap - refused here from an output of the cap's size on. A zlib error counts 0:
    chunk_iCCP, chunk_zTXt and chunk_iTXt catch it and drop the profile or the text."""
    try:
        n = len(zlib.decompressobj().decompress(z, MAX_TEXT_CHUNK))
    except zlib.error:
        return 0
    if n >= MAX_TEXT_CHUNK:
        raise Unsupported("compressed chunk inflates to MAX_TEXT_CHUNK or more")
    return n


def _metadata(cid, s, ctype, depth):
    """The rule of one of METADATA_CHUNKS with the body s, restated from its handler in PIL/PngImagePlugin.py (PngStream.chunk_*).
    -> the bytes it adds to Pillow's text memory (check_text_memory), None for any other chunk; raises Unsupported where the
    handler raises or where Pillow's result is not vouched for."""
    if cid == b"iCCP":
        # chunk_iCCP: comp_method = s[s.find(0) + 1] must be 0 (SyntaxError otherwise; no NUL reads s[0], an empty chunk raises
        # IndexError), then _safe_zlib_decompress(s[i + 2:]); stored as info["icc_profile"], which no step of the transform applies
        i = s.find(b"\0")
        if i < 0 or i + 1 >= len(s) or s[i + 1] != 0:
            raise Unsupported("iCCP chunk")
        _inflated(s[i + 2:])
        return 0
    if cid == b"zTXt":
        # chunk_zTXt: k, v = s.split(NUL, 1) (no NUL: v empty); v[0] must be 0 where there is a v; _safe_zlib_decompress(v[1:])
        _, _, v = s.partition(b"\0")
        if v and v[0] != 0:
            raise Unsupported("zTXt chunk")
        return _inflated(v[1:])
    if cid == b"iTXt":
        # chunk_iTXt returns without a word for every malformed shape: no NUL, fewer than 2 bytes behind it, fewer than three
        # NUL-separated fields, a compression method other than 0, a zlib error, text that is not UTF-8. Only flag != 0 with
        # method 0 inflates (_safe_zlib_decompress); plain text counts as it is
        _, nul, r = s.partition(b"\0")
        if not nul or len(r) < 2:
            return 0
        fields = r[2:].split(b"\0", 2)
        if len(fields) != 3:
            return 0
        if r[0] != 0:
            return _inflated(fields[2]) if r[1] == 0 else 0
        return len(fields[2])
    if cid == b"eXIf":
        return 0                                               # chunk_eXIf: kept as info["exif"]; nobody applies its orientation tag
    if cid == b"tRNS":
        # chunk_tRNS: i16(s) for mode L, three of them for RGB (struct.error on a shorter chunk) -> info["transparency"], which
        # changes no pixel of resize / crop / convert("RGB"). Palette files have their own rule in parse(); on the alpha colour
        # types and on grey below depth 8 the chunk stays refused
        if (ctype == 0 and depth == 8 and len(s) == 2) or (ctype == 2 and len(s) == 6):
            return 0
        raise Unsupported("tRNS chunk")
    return None


def parse(data, modes=False, interlaced=False, chunks=False, deep=False):
    """PNG file contents -> Parsed; raises Unsupported(reason). modes: also let the files of kinds "alpha" and "index" through.
    interlaced: also let Adam7 files (interlace method 1) of the colour types and depths let through anyway through.
    chunks: also let files through that carry METADATA_CHUNKS or chunks Pillow has no handler for (Parsed.chunks says that the file
    needed it). deep: also let RGB files of depth 16 through, and with modes RGBA and grey + alpha files of depth 16."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise Unsupported("not a PNG file")
    pos, n = 8, len(data)
    first = True
    text = 0
    pieces = None
    plte = None                                                # the PLTE chunk's body (colour type 3 under modes=True)
    seen_trns = False
    marked = 0                                                 # a chunk was let through that only chunks=True lets through
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
            deep16 = deep and depth == 16 and (ctype == 2 or (modes and ctype in _DEEP))
            if not rgb and not deep16 and not (modes and ctype in _MODES and depth in _MODES[ctype][1]):
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
            channels = (3 if ctype == 2 else 1) if rgb else _DEEP[ctype] if deep16 else _MODES[ctype][0]
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
            if want == -1 and chunks:
                added = _metadata(cid, data[body:body + length], ctype, depth)
                if added is None:
                    # no handler in Pillow (_open: AttributeError -> read, CRC checked - above - and dropped); ChunkStream.read
                    # raises for a type that is not four word characters
                    if cid in PILLOW_HANDLERS or not _CID.fullmatch(cid):
                        raise Unsupported("chunk %r in front of the image data" % cid)
                    added = 0
                text += added
                marked = 1
            elif want == -1 or (want is not None and length != want):
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
                # (load_end calls the same handlers; a palette file's tRNS belongs in front of the image data: _metadata refuses it)
                added = _metadata(cid, data[pos + 8:pos + 8 + length], ctype, depth) if chunks else None
                if added is None:
                    raise Unsupported("chunk %r behind the image data" % cid)
                text += added
                marked = 1
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
        return Parsed(width, height, channels, stream[2:], interlace=lace, chunks=marked)
    if deep16:
        return Parsed(width, height, channels, stream[2:], "rgb" if ctype == 2 else "alpha", 16, ctype, interlace=lace, chunks=marked)
    if ctype == 3:
        if plte is None:
            raise Unsupported("no PLTE chunk")
        return Parsed(width, height, 1, stream[2:], "index", depth, 3, _palette(plte, len(plte) // 3), len(plte) // 3, interlace=lace,
                      chunks=marked)
    if ctype == 0 and depth == 1:
        return Parsed(width, height, 1, stream[2:], "index", 1, 0, _palette(b"\0\0\0\xff\xff\xff", 2), 2, interlace=lace, chunks=marked)
    return Parsed(width, height, channels, stream[2:], "alpha", depth, ctype, interlace=lace, chunks=marked)
