"""Adam7-interlaced PNG files for the tests of `png_parse.parse(interlaced=True)` and the device decoder behind it. No tests here.

Pillow's encoder writes no interlaced files, so this is a writer of its own on top of png_cases and png_mode_cases: the image
is split into its seven sub-images, each is packed and filtered on its own (a filter byte per pass row, every type in turn and a
filter other than None on each pass's first row) and the passes' scanlines are deflated as one stream. Beside it the numpy
restatement of what the device does with such a file: inflate to exactly the summed size, unfilter pass by pass, scatter.
"""
import io
import struct
import zlib

import numpy as np
from PIL import Image

import png_cases
import png_mode_cases as M

PASSES = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))     # x0 y0 dx dy (PNG 1.2, 8.2)
SAMPLES = {**M.SAMPLES, 2: 3}                                  # colour type -> samples per pixel
# every (colour type, depth) the two entries take, with the kind the parser gives it
MODES = {(0, 8): "rgb", (2, 8): "rgb", **M.MODES}


def unit_of(ctype, depth):
    """the filter's unit: the pixel's bytes, 1 below depth 8"""
    return SAMPLES[ctype] if depth == 8 else 1


def pass_filters(p, ph):
    """a filter type per row of pass p: never None on the first row, every type from five rows on"""
    return [(1 + p % 4 + k) % 5 for k in range(ph)]


def pass_pieces(samples, ctype, depth):
    """samples uint8 [h][w][ch] -> per non-empty pass (its number, its filtered scanlines as bytes, the bytes of one of its
    scanlines with the filter byte)"""
    pieces = []
    for p, (x0, y0, dx, dy) in enumerate(PASSES):
        sub = samples[y0::dy, x0::dx]
        if not sub.size:
            continue
        rows = M.pack_rows(np.ascontiguousarray(sub), depth)
        unit = unit_of(ctype, depth)
        raw = png_cases.filter_rows(rows.reshape(rows.shape[0], rows.shape[1] // unit, unit), pass_filters(p, rows.shape[0]))
        pieces.append((p, raw, 1 + rows.shape[1]))
    return pieces


def scanlines(samples, ctype, depth):
    return b"".join(raw for _, raw, _ in pass_pieces(samples, ctype, depth))


def before_chunks(ctype, palette=None, alphas=None):
    return M.plte(palette) + (M.trns(alphas) if alphas is not None else b"") if ctype == 3 else b""


def write(samples, ctype, depth, palette=None, alphas=None, idat=8192, lace=1, raw=None, **kw):
    """samples uint8 [h][w][samples per pixel] -> an interlaced PNG file of that colour type and depth (raw: other scanlines
    under the same header)"""
    h, w, ch = samples.shape
    assert ch == SAMPLES[ctype]
    z = png_cases.deflate(scanlines(samples, ctype, depth) if raw is None else raw, **kw)
    return png_cases.assemble(w, h, ch, z, idat=idat, before=before_chunks(ctype, palette, alphas), depth=depth, ctype=ctype, lace=lace)


def plain_scanlines(samples, ctype, depth, mode="cycle1"):
    """the scanlines of the same picture stored without interlace"""
    if depth == 8 and ctype in (0, 2):
        return png_cases.filter_rows(samples, png_cases.filters_for(mode, samples.shape[0]))
    return M.scanlines(samples, ctype, depth, mode)


def samples_for(rng, ctype, depth, h, w, k=0):
    if depth == 8 and ctype in (0, 2):
        return (png_cases.noise, png_cases.smooth, png_cases.screenshot)[k % 3](rng, h, w, SAMPLES[ctype]), None
    return M.samples_for(rng, ctype, depth, h, w, k)


def lace_file(rng, ctype, depth, h, w, k=0, with_trns=False, **kw):
    s, pal = samples_for(rng, ctype, depth, h, w, k)
    alphas = rng.integers(0, 256, int(rng.integers(1, len(pal) + 1))) if with_trns else None
    return write(s, ctype, depth, palette=pal, alphas=alphas, **kw)


# every kind of file, as (name, colour type, depth, tRNS)
KINDS = [("l8", 0, 8, False), ("rgb8", 2, 8, False)] + M.KINDS + [("p2t", 3, 2, True), ("p1t", 3, 1, True)]
SMALL = (1, 2, 3, 4, 5, 7, 8, 9)


def cases(rng):
    """[(name, file)], all valid, all for the device with modes and interlaced on: the list the GPU test decodes"""
    out = []
    k = 0
    for w in SMALL:                                            # every combination of empty passes, the kinds in turn
        for h in SMALL:
            name, ctype, depth, t = KINDS[k % len(KINDS)]
            out.append((f"small_{name}_{h}x{w}", lace_file(rng, ctype, depth, h, w, k, with_trns=t, level=(1, 6, 9)[k % 3])))
            k += 1
    for h in (127, 128, 129, 130, 511, 512, 513):              # band edges of pass 7 (h / 2 rows) and pass 1 (h / 8 rows)
        out.append((f"band_rgb8_{h}x9", lace_file(rng, 2, 8, h, 9, k, level=6)))
        k += 1
    for w in (21, 22, 42, 43, 44, 45):                         # pass rows of 63 .. 69 bytes (passes 7 and 6): either side of a wave
        out.append((f"wave_rgb8_17x{w}", lace_file(rng, 2, 8, 17, w, k, level=6)))
        k += 1
    out.append(("smooth_rgb8_224x224", lace_file(rng, 2, 8, 224, 224, 1, level=6)))
    out.append(("wrap_rgb8_300x500", lace_file(rng, 2, 8, 300, 500, 1, level=1)))      # 450 KB of scanlines: the DEFLATE ring wraps
    for name, ctype, depth, t in KINDS:                        # pass widths x depth that are no multiple of 8 in several passes
        for h, w in ((19, 9), (19, 13), (133, 33)):
            out.append((f"kind_{name}_{h}x{w}", lace_file(rng, ctype, depth, h, w, k, with_trns=t, level=(1, 6, 9)[k % 3])))
            k += 1
    return out


# ---- Pillow as the reference --------------------------------------------------------------------------------------------------
def pillow_pixels(blob):
    """what decode_files(modes=True, interlaced=True) has to return for a file, from Pillow: ("rgb", uint8 [h][w][3]) for an 8-bit
    grey or RGB file, else png_mode_cases.pillow_pixels"""
    im = Image.open(io.BytesIO(blob))
    depth, ctype = blob[24], blob[25]
    if depth == 8 and ctype in (0, 2):
        assert im.mode == ("L" if ctype == 0 else "RGB"), im.mode
        return "rgb", np.asarray(im.convert("RGB"))
    return M.pillow_pixels(blob)


def same(got, blob):
    """what decode_files returned for a file == Pillow's pixels in the file's own mode (and its palette)"""
    kind, ref = pillow_pixels(blob)
    if kind == "index":
        return isinstance(got, tuple) and np.array_equal(got[0], ref) and np.array_equal(got[1], M.pillow_palette(blob)[0])
    return got is not None and not isinstance(got, tuple) and got.shape == ref.shape and np.array_equal(got, ref)


# ---- the CPU restatement ------------------------------------------------------------------------------------------------------
def cpu_samples(p):
    """png_parse.Parsed of an interlaced file -> its samples uint8 [h][w][channels], None where the device would report the
    file: the stream does not inflate to exactly the passes' bytes with a matching Adler-32, or a filter byte is above 4"""
    raw = png_cases.inflate_exact(p.stream, p.raw_bytes())
    if raw is None:
        return None
    unit = p.channels if p.depth == 8 else 1
    out = np.zeros((p.height, p.width, p.channels), np.uint8)
    at = 0
    for x0, y0, dx, dy in PASSES:
        pw, ph = len(range(x0, p.width, dx)), len(range(y0, p.height, dy))
        if not pw or not ph:
            continue
        nb = (pw * p.channels * p.depth + 7) // 8
        rows = png_cases.unfilter(raw[at:at + ph * (1 + nb)], nb // unit, ph, unit)
        at += ph * (1 + nb)
        if rows is None:
            return None
        rows = (rows[..., 0] if unit == 1 else rows).reshape(ph, nb)
        if p.depth < 8:
            bits = np.unpackbits(rows, axis=1)[:, :pw * p.depth].reshape(ph, pw, p.depth)
            s = (bits.astype(np.int64) << np.arange(p.depth - 1, -1, -1)).sum(axis=2).astype(np.uint8).reshape(ph, pw, 1)
        else:
            s = rows.reshape(ph, pw, p.channels)
        out[y0::dy, x0::dx] = s
    assert at == len(raw)
    return out


def cpu_decode(p):
    """-> what decode_files gives for the file (without the palette): uint8 [h][w][3], [h][w][4] or [h][w]; None where the device
    would report it (cpu_samples, and an index beyond the palette)"""
    s = cpu_samples(p)
    if s is None:
        return None
    if p.kind == "rgb":
        return np.repeat(s, 3, axis=2) if p.channels == 1 else s
    if p.kind == "index":
        s = s.reshape(p.height, p.width)
        return None if int(s.max()) >= p.n_entries else s
    if p.ctype == 6:
        return s
    if p.ctype == 4:
        return np.concatenate([np.repeat(s[..., :1], 3, axis=2), s[..., 1:]], axis=2)
    v = (s.reshape(p.height, p.width).astype(np.int64) * (85 if p.depth == 2 else 17)).astype(np.uint8)
    return np.stack([v, v, v, np.full_like(v, 255)], axis=2)


# ---- malformed files ----------------------------------------------------------------------------------------------------------
def malformed_corpus(rng):
    """[(family, file)]: the damages of png_cases.malformed_corpus placed in four interlaced files (RGB, grey, RGBA, 4-bit
    palette), and one of this form's own: the scanlines of the picture stored without interlace under a header that says
    interlaced, and the reverse ("wrong_order")"""
    corpus = []
    pal = rng.integers(0, 256, (16, 3), dtype=np.uint8)
    base = [(2, 8, png_cases.smooth(rng, 30, 40, 3), 6, None), (0, 8, png_cases.noise(rng, 17, 23, 1), 9, None),
            (6, 8, M.samples_for(rng, 6, 8, 65, 22, 2)[0], 1, None), (3, 4, rng.integers(0, 16, (40, 41, 1), dtype=np.uint8), 0, pal)]
    for ctype, depth, s, level, palette in base:
        h, w, ch = s.shape
        pieces = pass_pieces(s, ctype, depth)
        raw = b"".join(r for _, r, _ in pieces)
        z = png_cases.deflate(raw, level=level)
        before = before_chunks(ctype, palette)

        def f(zz, lace=1, **kw):
            return png_cases.assemble(w, h, ch, zz, before=before, depth=depth, ctype=ctype, lace=lace, **kw)

        for _ in range(12):
            zz = bytearray(z)
            k = int(rng.integers(2, len(zz)))
            zz[k] ^= 1 << int(rng.integers(0, 8))
            corpus.append(("bitflip", f(bytes(zz))))
        for _ in range(6):
            corpus.append(("truncated", f(z[:int(rng.integers(2, len(z) - 4))])))
        corpus.append(("truncated", f(z[:-8])))
        starts = np.cumsum([0] + [len(r) for _, r, _ in pieces])
        for ft in (5, 6, 255):                                 # in a row of a pass other than the first
            j = int(rng.integers(1, len(pieces)))
            stride = pieces[j][2]
            bad = bytearray(raw)
            bad[int(starts[j]) + int(rng.integers(0, len(pieces[j][1]) // stride)) * stride] = ft
            corpus.append(("filter_byte", f(png_cases.deflate(bytes(bad), level=level))))
        corpus.append(("adler_wrong", f(z[:-4] + struct.pack(">I", (zlib.adler32(raw) + 1) & 0xffffffff))))
        corpus.append(("adler_wrong", f(z[:-1] + bytes([z[-1] ^ 0x80]))))
        corpus.append(("adler_missing", f(z[:-4])))
        last = pieces[-1]
        corpus.append(("extra_rows", f(png_cases.deflate(raw + last[1][:2 * last[2]], level=level))))      # two more rows of the last pass
        corpus.append(("short_data", f(png_cases.deflate(raw[:-5], level=level))))
        corpus.append(("harmless", f(z + b"garbage behind the stream")))
        corpus.append(("harmless", f(z, idat=1 << 30) + b"bytes after IEND"))
        corpus.append(("harmless", f(z, iend=False)))
        corpus.append(("harmless", f(z, after=png_cases.chunk(b"tEXt", b"k\0v", crc=12345))))
        good = f(z, idat=1 << 30)
        k = good.index(b"IDAT") + 4 + len(z)                   # (one IDAT chunk: its CRC follows the stream)
        corpus.append(("harmless", good[:k] + bytes([good[k] ^ 0xff]) + good[k + 1:]))
        plain = png_cases.deflate(plain_scanlines(s, ctype, depth), level=level)
        corpus.append(("wrong_order", f(plain)))               # plain scanlines, the header says interlaced
        corpus.append(("wrong_order", f(z, lace=0)))           # the passes' scanlines, the header says not interlaced
    return corpus
