"""PNG files for the tests of `png_parse.parse(chunks=True)` and `png_parse.parse(deep=True)` and of the device decode behind
them: files of depth 16 (colour types 2, 6, 4; plain and Adam7) and files that carry metadata chunks. No tests here.

Pillow's encoder writes 16-bit files of mode I;16 only, so the 16-bit files come from a writer of its own on top of png_cases:
samples are uint16, stored high byte first, filtered with the pixel's bytes (6, 8, 4) as the unit. The low bytes are noise that
does not depend on the high bytes: a store that keeps the wrong byte, or a filter that drops the low bytes before Sub, Average
and Paeth have used them, cannot pass. Pillow itself is the reference everywhere.
"""
import io
import struct
import zlib

import numpy as np
from PIL import Image

import png_cases
import png_interlace_cases as A
import png_mode_cases as M

SAMPLES = {2: 3, 6: 4, 4: 2}                                   # colour type -> samples per pixel of the depth-16 files deep=True takes
KIND = {2: "rgb", 6: "alpha", 4: "alpha"}                      # ... and the kind the parser gives them
MAX_WIDTH = {2: 8192, 6: 6144, 4: 12288}                       # rows of 49152 bytes
CTYPES = (2, 6, 4)


# ---- 16-bit files -------------------------------------------------------------------------------------------------------------
def samples16(rng, ctype, h, w, k=0):
    """uint16 [h][w][ch]: the high bytes noise, smooth or screenshot-like (k), the low bytes noise of their own"""
    ch = SAMPLES[ctype]
    high = (png_cases.noise, png_cases.smooth, png_cases.screenshot)[k % 3](rng, h, w, ch)
    low = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    return high.astype(np.uint16) << 8 | low


def pixel_bytes(s):
    """uint16 [h][w][ch] -> uint8 [h][w][2 ch], each sample's high byte first (PNG 1.2, 2.1)"""
    h, w, ch = s.shape
    return np.stack([(s >> 8).astype(np.uint8), (s & 255).astype(np.uint8)], axis=3).reshape(h, w, 2 * ch)


def scanlines16(s, mode="cycle"):
    return png_cases.filter_rows(pixel_bytes(s), png_cases.filters_for(mode, s.shape[0]))


def lace_scanlines16(s):
    """the scanlines of the seven passes, each filtered on its own (png_interlace_cases.pass_filters)"""
    b = pixel_bytes(s)
    out = []
    for p, (x0, y0, dx, dy) in enumerate(A.PASSES):
        sub = np.ascontiguousarray(b[y0::dy, x0::dx])
        if sub.size:
            out.append(png_cases.filter_rows(sub, A.pass_filters(p, sub.shape[0])))
    return b"".join(out)


def write16(s, ctype, mode="cycle", lace=0, idat=8192, before=b"", after=b"", raw=None, **kw):
    """uint16 [h][w][ch] -> a PNG file of depth 16 (lace=1: Adam7; raw: other scanlines under the same header)"""
    h, w, ch = s.shape
    assert ch == SAMPLES[ctype]
    if raw is None:
        raw = lace_scanlines16(s) if lace else scanlines16(s, mode)
    return png_cases.assemble(w, h, ch, png_cases.deflate(raw, **kw), idat=idat, before=before, after=after, depth=16, ctype=ctype, lace=lace)


def deep_file(rng, ctype, h, w, k=0, mode="cycle", **kw):
    return write16(samples16(rng, ctype, h, w, k), ctype, mode, **kw)


def high_bytes(s, ctype):
    """what Pillow opens the file as: RGB, RGBA, or RGBA as L L L A, of the samples' high bytes"""
    hi = (s >> 8).astype(np.uint8)
    return np.concatenate([np.repeat(hi[..., :1], 3, axis=2), hi[..., 1:]], axis=2) if ctype == 4 else hi


def pillow_pixels(blob):
    """Pillow's own-mode pixels of a file, uint8 [h][w][3 or 4]"""
    im = Image.open(io.BytesIO(blob))
    assert im.mode in ("RGB", "RGBA"), im.mode
    return np.asarray(im)


WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 300]             # either side of the 4-unit step
HEIGHTS = [1, 2, 63, 64, 65, 129]                              # either side of a 64-row band


def decode_cases(rng):
    """[(name, file)], all valid and all for the device with modes and deep on: every width x height with the colour types, the
    filter modes, the levels and the contents in turn; each of the five filters on every row and the cycling modes for each
    colour type (smooth high bytes, so that Paeth and Average select among their candidates); every level for each colour type"""
    cases = []
    k = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            ctype, mode, level = CTYPES[k % 3], png_cases.MODES[(k // 3) % len(png_cases.MODES)], png_cases.LEVELS[(k // 2) % 4]
            cases.append((f"c{ctype}_w{w}h{h}_f{mode}_l{level}", deep_file(rng, ctype, h, w, k // 3, mode, level=level)))
            k += 1
    for ctype in CTYPES:
        for mode in png_cases.MODES:
            cases.append((f"c{ctype}_filter{mode}_smooth", deep_file(rng, ctype, 70, 37, 1, mode, level=6)))
        for level in png_cases.LEVELS:
            cases.append((f"c{ctype}_level{level}", deep_file(rng, ctype, 65, 22, level, "cycle1", level=level)))
    return cases


def lace_cases(rng):
    """[(name, file)]: Adam7 files of depth 16, 1 x 1 up to 9 x 9 (every combination of empty passes) with the colour types in
    turn, and 65 x 63 for each colour type"""
    cases = []
    k = 0
    for w in A.SMALL:
        for h in A.SMALL:
            ctype = CTYPES[k % 3]
            cases.append((f"lace_c{ctype}_{h}x{w}", deep_file(rng, ctype, h, w, k // 3, lace=1, level=(1, 6, 9)[k % 3])))
            k += 1
    for ctype in CTYPES:
        cases.append((f"lace_c{ctype}_63x65", deep_file(rng, ctype, 63, 65, 1, lace=1)))
    return cases


def widest_cases(rng):
    """65 rows of the widest row each colour type may have: screenshot-like high bytes and low bytes that repeat along a row, so that
    the files stay small"""
    cases = []
    for ctype in CTYPES:
        w = MAX_WIDTH[ctype]
        s = samples16(rng, ctype, 65, 256, 2)
        cases.append((f"widest_c{ctype}_{w}", write16(np.tile(s, (1, w // 256, 1)), ctype, "cycle", level=1)))
    return cases


def corrupt_cases(rng, ctype, h=40, w=50):
    """[(name, file, the status the device gives the stream)]: a cut stream (2), a flipped Adler-32 (4), a filter byte 5 (3) and
    a stream that inflates to the scanlines of the 8-bit file (2: too little)"""
    s = samples16(rng, ctype, h, w, 1)
    raw = scanlines16(s)
    z = png_cases.deflate(raw)
    bad = bytearray(raw)
    bad[(h // 2) * (1 + w * 2 * SAMPLES[ctype])] = 5

    def f(zz):
        return png_cases.assemble(w, h, SAMPLES[ctype], zz, depth=16, ctype=ctype)
    short = png_cases.filter_rows((s >> 8).astype(np.uint8), [0] * h)
    return [("cut", f(z[:len(z) // 2]), 2), ("adler", f(z[:-4] + struct.pack(">I", zlib.adler32(raw) ^ 1)), 4),
            ("filter5", f(png_cases.deflate(bytes(bad))), 3), ("eight_bit_sized", f(png_cases.deflate(short)), 2)]


# ---- metadata chunks ----------------------------------------------------------------------------------------------------------
C = png_cases.chunk
CAP = 1 << 20                                                  # PngImagePlugin.MAX_TEXT_CHUNK


def z(n, fill=b"\x5a"):
    """a zlib stream that inflates to n bytes"""
    return zlib.compress(fill * n, 1)


XMP = b"XML:com.adobe.xmp\0\0\0\0\0" + b"<x:xmpmeta xmlns:x='adobe:ns:meta/'/>"
EXIF6 = b"MM\0*\0\0\0\x08\0\x01\x01\x12\0\x03\0\0\0\x01\0\x06\0\0\0\0\0\0"          # one tag: orientation 6


def valid_chunks():
    """[(name, chunk bytes)]: chunks that change no pixel; Pillow opens the file with each of them, in front of and behind the data"""
    return [("iCCP", C(b"iCCP", b"sRGB IEC61966-2.1\0\0" + z(3144))),
            ("iCCP_twice", C(b"iCCP", b"a\0\0" + z(100)) + C(b"iCCP", b"b\0\0" + z(200))),
            ("iTXt_plain", C(b"iTXt", XMP)),
            ("iTXt_compressed", C(b"iTXt", b"Comment\0\1\0en\0Kommentar\0" + z(500))),
            ("zTXt", C(b"zTXt", b"Comment\0\0" + z(700))),
            ("eXIf", C(b"eXIf", EXIF6)),
            ("iDOT", C(b"iDOT", struct.pack(">7I", 2, 0, 130, 40, 130, 130, 7000))),
            ("sPLT", C(b"sPLT", b"pal\0\x08" + bytes(range(12)))),
            ("hIST", C(b"hIST", b"\0\1\0\2")),
            ("oFFs", C(b"oFFs", struct.pack(">iiB", 10, -10, 1))),
            ("unknown_critical", C(b"ABCD", b"whatever")),
            ("screenshot", C(b"iCCP", b"Display P3\0\0" + z(536)) + C(b"eXIf", EXIF6) + C(b"iTXt", XMP) + C(b"pHYs", struct.pack(">IIB", 5669, 5669, 1)) +
             C(b"iDOT", struct.pack(">7I", 2, 0, 130, 40, 130, 130, 7000)))]


def broken_zlib_chunks():
    """[(name, chunk bytes)]: compressed chunks whose data is bad or cut - Pillow drops the profile or the text and goes on"""
    good = z(4000, b"abcdefg")
    return [("iCCP_bad_zlib", C(b"iCCP", b"p\0\0not zlib data")), ("iCCP_cut_zlib", C(b"iCCP", b"p\0\0" + good[:len(good) // 2])),
            ("iCCP_no_data", C(b"iCCP", b"p\0\0")),
            ("zTXt_bad_zlib", C(b"zTXt", b"k\0\0\xff\xfe\xfd")), ("zTXt_cut_zlib", C(b"zTXt", b"k\0\0" + good[:9])),
            ("iTXt_bad_zlib", C(b"iTXt", b"k\0\1\0\0\0not zlib")), ("iTXt_cut_zlib", C(b"iTXt", b"k\0\1\0\0\0" + good[:len(good) - 5]))]


def tolerated_shapes():
    """[(name, chunk bytes)]: malformed iTXt / zTXt shapes that Pillow's handlers return from without a word"""
    return [("iTXt_no_nul", C(b"iTXt", b"keyword only")), ("iTXt_short", C(b"iTXt", b"k\0\0")), ("iTXt_two_fields", C(b"iTXt", b"k\0\0\0lang\0no more")),
            ("iTXt_method_1", C(b"iTXt", b"k\0\1\1\0\0" + z(10))), ("iTXt_bad_utf8", C(b"iTXt", b"k\0\0\0\0\0\xff\xfe\xfd")),
            ("iTXt_empty", C(b"iTXt", b"")), ("zTXt_no_nul", C(b"zTXt", b"keyword only")), ("zTXt_empty_value", C(b"zTXt", b"k\0")),
            ("zTXt_empty", C(b"zTXt", b"")), ("eXIf_empty", C(b"eXIf", b"")), ("eXIf_garbage", C(b"eXIf", b"\xff" * 33))]


def failing_chunks():
    """[(name, chunk bytes, whether Pillow fails behind the image data too)]: chunks that make Pillow raise; None: a chunk the
    parser goes on refusing on either side whatever Pillow makes of it (APNG, a second IHDR, PLTE in an RGB file)"""
    return [("iCCP_method_1", C(b"iCCP", b"p\0\1" + z(100)), True), ("zTXt_method_1", C(b"zTXt", b"k\0\1" + z(100)), True),
            ("iCCP_no_nul", C(b"iCCP", b"profile"), True), ("iCCP_empty", C(b"iCCP", b""), True),
            ("iCCP_nul_last", C(b"iCCP", b"profile\0"), True),
            ("bad_type", C(b"ab-d", b"data"), False),             # behind the image data Pillow stops reading there
            ("iCCP_2MiB", C(b"iCCP", b"p\0\0" + z(2 << 20)), True), ("zTXt_2MiB", C(b"zTXt", b"k\0\0" + z(2 << 20)), True),
            ("iTXt_2MiB", C(b"iTXt", b"k\0\1\0\0\0" + z(2 << 20)), True),
            ("acTL", C(b"acTL", struct.pack(">II", 2, 0)), None), ("IHDR_again", C(b"IHDR", struct.pack(">IIBBBBB", 4, 4, 8, 2, 0, 0, 0)), None),
            ("PLTE", C(b"PLTE", bytes(range(12))), None), ("unknown_bad_crc", C(b"zzZz", b"private", crc=3), False)]


def bound_chunks():
    """[(name, chunk bytes)]: compressed chunks on either side of the cap"""
    out = []
    for what, head in (("iCCP", b"p\0\0"), ("zTXt", b"k\0\0"), ("iTXt", b"k\0\1\0\0\0")):
        out += [(f"{what}_cap_minus_1", C(what.encode(), head + z(CAP - 1))), (f"{what}_cap", C(what.encode(), head + z(CAP)))]
    return out


def trns_cases(rng):
    """[(name, file with tRNS, the same file without, the switches it needs)] for tRNS in front of and behind the image data: 2 bytes
    on 8-bit grey, 6 on RGB at depth 8 and 16 (the files the chunk is let through on), and the lengths and colour types it is not"""
    g8, rgb8, s16 = png_cases.smooth(rng, 20, 24, 1), png_cases.smooth(rng, 20, 24, 3), samples16(rng, 2, 20, 24, 1)
    zg, zr, z16 = (png_cases.deflate(png_cases.filter_rows(a, png_cases.filters_for("cycle", 20))) for a in (g8, rgb8, pixel_bytes(s16)))
    la, rgba = M.samples_for(rng, 4, 8, 20, 24, 1)[0], M.samples_for(rng, 6, 8, 20, 24, 1)[0]
    g4 = M.samples_for(rng, 0, 4, 20, 24, 1)[0]
    zla, zrgba, zg4 = (png_cases.deflate(M.scanlines(a, c, d)) for a, c, d in ((la, 4, 8), (rgba, 6, 8), (g4, 0, 4)))
    out = []
    for name, (w, h, ch, zz, kw), body in (("grey8_2", (24, 20, 1, zg, {}), b"\0\x80"), ("rgb8_6", (24, 20, 3, zr, {}), b"\0\1\0\2\0\3"),
                                           ("rgb16_6", (24, 20, 3, z16, dict(depth=16, ctype=2)), b"\1\2\3\4\5\6"),
                                           ("grey8_1", (24, 20, 1, zg, {}), b"\0"), ("grey8_0", (24, 20, 1, zg, {}), b""),
                                           ("grey8_3", (24, 20, 1, zg, {}), b"\0\1\2"), ("rgb8_5", (24, 20, 3, zr, {}), b"\0\1\0\2\0"),
                                           ("rgb8_8", (24, 20, 3, zr, {}), b"\0\1\0\2\0\3\0\4"), ("rgb16_2", (24, 20, 3, z16, dict(depth=16, ctype=2)), b"\1\2"),
                                           ("la8_2", (24, 20, 2, zla, dict(ctype=4)), b"\0\1"), ("rgba8_6", (24, 20, 4, zrgba, dict(ctype=6)), b"\0\1\0\2\0\3"),
                                           ("grey4_2", (24, 20, 1, zg4, dict(depth=4, ctype=0)), b"\0\3")):
        free = png_cases.assemble(w, h, ch, zz, **kw)
        for where in ("before", "after"):
            out.append((f"tRNS_{name}_{where}", png_cases.assemble(w, h, ch, zz, **{where: C(b"tRNS", body)}, **kw), free))
    return out


def base_image(rng, h=260, w=300):
    """the chunk-free file the chunk cases are built on, as (w, h, its zlib stream)"""
    img = png_cases.smooth(rng, h, w, 3)
    return w, h, png_cases.deflate(png_cases.filter_rows(img, png_cases.filters_for("cycle", h)), level=1)


def with_chunk(base, chunk, where):
    w, h, zz = base
    return png_cases.assemble(w, h, 3, zz, **{where: chunk})


def transform_ref(blob, n_px=224):
    """Pillow live through resize -> crop -> convert("RGB") (decode_worker.load_uint8); None where Pillow raises"""
    try:
        return M.load_uint8_blob(blob, n_px)
    except Exception:
        return None
