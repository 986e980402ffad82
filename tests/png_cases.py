"""PNG files for the tests of the device PNG decoder (cli-p_amd/png_parse.py, csrc/png.hip). No tests here.

A PNG writer of its own (a chosen filter per row in numpy, zlib.compressobj with chosen level, wbits, strategy and flush
points, IDAT pieces of a chosen size), a small bit-level DEFLATE writer for streams zlib never emits, a seeded corpus of
malformed files tagged by family, and the CPU restatement of the decoder: zlib.decompressobj(-15) plus a numpy unfilter.
"""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"


# ---- images ---------------------------------------------------------------------------------------------------------------
def smooth(rng, h, w, ch=3):
    """photo-like: a few low-frequency waves plus a little noise"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((h, w, ch), np.uint8)
    for c in range(ch):
        f = rng.uniform(0.01, 0.15, 4)
        p = rng.uniform(0, 6.28, 4)
        v = 128 + 50 * np.sin(f[0] * x + p[0]) + 40 * np.cos(f[1] * y + p[1]) + 25 * np.sin(f[2] * (x + y) + p[2])
        out[..., c] = np.clip(v + rng.normal(0, 2, (h, w)), 0, 255).astype(np.uint8)
    return out


def noise(rng, h, w, ch=3):
    return rng.integers(0, 256, (h, w, ch), dtype=np.uint8)


def screenshot(rng, h, w, ch=3):
    """screenshot-like: flat areas, text-like edges, long matches"""
    a = np.full((h, w, ch), 245, np.uint8)
    for _ in range(max(1, h * w // 4000)):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        a[y0:y0 + int(rng.integers(1, 40)), x0:x0 + int(rng.integers(1, 120))] = rng.integers(0, 256, ch, dtype=np.uint8)
    for y0 in range(4, h - 8, 14):                              # "lines of text": short dark runs on the background
        xs = rng.integers(0, 2, w // 3 + 1).repeat(3)[:w].astype(bool)
        a[y0:y0 + 7:2, xs] = 30
    return a


# ---- the writer -----------------------------------------------------------------------------------------------------------
def chunk(cid, body, crc=None):
    c = zlib.crc32(cid + body) if crc is None else crc
    return struct.pack(">I", len(body)) + cid + body + struct.pack(">I", c & 0xffffffff)


def filter_rows(img, filters):
    """img uint8 [h][w][ch], filters: one filter type per row -> the filtered scanlines (PNG 1.2 section 6), bytes"""
    h, w, ch = img.shape
    cur = img.reshape(h, w * ch).astype(np.int32)
    up = np.vstack([np.zeros((1, w * ch), np.int32), cur[:-1]])
    left = np.hstack([np.zeros((h, ch), np.int32), cur[:, :-ch]])
    ul = np.hstack([np.zeros((h, ch), np.int32), up[:, :-ch]])
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    pred = np.stack([np.zeros_like(cur), left, up, (left + up) >> 1, paeth])
    f = np.asarray(filters, np.int64)
    body = ((cur - pred[np.minimum(f, 4), np.arange(h)]) & 255).astype(np.uint8)
    return np.hstack([f.astype(np.uint8)[:, None], body]).tobytes()


def deflate(raw, level=6, wbits=15, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, flush_mode=zlib.Z_SYNC_FLUSH):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    if not flush_every:
        return co.compress(raw) + co.flush()
    out = []
    for k in range(0, len(raw), flush_every):
        out.append(co.compress(raw[k:k + flush_every]))
        out.append(co.flush(flush_mode))
    out.append(co.flush())
    return b"".join(out)


def assemble(w, h, ch, zstream, idat=8192, before=b"", after=b"", iend=True, depth=8, ctype=None, lace=0):
    ctype = (2 if ch == 3 else 0) if ctype is None else ctype
    out = [SIG, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, lace)), before]
    for k in range(0, max(len(zstream), 1), idat):
        out.append(chunk(b"IDAT", zstream[k:k + idat]))
    out.append(after)
    if iend:
        out.append(chunk(b"IEND", b""))
    return b"".join(out)


def filters_for(mode, h):
    if mode == "cycle":
        return [k % 5 for k in range(h)]
    if mode == "cycle1":                                       # a filter other than None on row 0
        return [(k + 1) % 5 for k in range(h)]
    if mode == "cycle4":
        return [(k + 4) % 5 for k in range(h)]
    return [int(mode)] * h


def write(img, mode="cycle", idat=8192, before=b"", **kw):
    h, w, ch = img.shape
    return assemble(w, h, ch, deflate(filter_rows(img, filters_for(mode, h)), **kw), idat=idat, before=before)


WIDTHS = [1, 2, 3, 21, 22, 64, 300]                            # RGB rows of 21 and 22 pixels are 64 and 67 bytes: either side of a wave
HEIGHTS = [1, 2, 63, 64, 65, 129]
MODES = [0, 1, 2, 3, 4, "cycle", "cycle1", "cycle4"]
LEVELS = [0, 1, 6, 9]


def writer_cases(rng):
    """[(name, file bytes)]: every file valid, every one of them for the device decoder"""
    cases = []
    k = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for ch in (1, 3):
                img = (smooth, noise, screenshot)[k % 3](rng, h, w, ch)
                mode, level = MODES[k % len(MODES)], LEVELS[(k // 3) % 4]
                cases.append((f"w{w}h{h}c{ch}_f{mode}_l{level}", write(img, mode, level=level)))
                k += 1
    for mode in MODES:                                         # each filter on every row, at a size with more than one band
        for ch in (1, 3):
            cases.append((f"filter{mode}_c{ch}", write(smooth(rng, 70, 37, ch), mode, level=6)))
    for mode in MODES:                                         # every filter mode at every level, rows of 67 bytes, two bands
        for level in LEVELS:
            cases.append((f"mode{mode}_l{level}", write((noise, smooth, screenshot)[level % 3](rng, 65, 22, 3), mode, level=level)))
    for name, strat in (("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huff", zlib.Z_HUFFMAN_ONLY)):
        for wbits in (9, 15):
            for ch in (1, 3):
                cases.append((f"{name}_wb{wbits}_c{ch}", write(smooth(rng, 65, 64, ch), "cycle", strategy=strat, wbits=wbits)))
    for wbits in (9, 15):
        cases.append((f"default_wb{wbits}", write(screenshot(rng, 129, 300, 3), "cycle1", wbits=wbits, level=9)))
    for every in (1, 2, 3, 5, 7, 11, 13, 112):                 # empty stored blocks, block starts at every bit offset
        for name, fm in (("sync", zlib.Z_SYNC_FLUSH), ("full", zlib.Z_FULL_FLUSH)):
            cases.append((f"{name}{every}", write(smooth(rng, 20, 21, 3), "cycle", flush_every=every, flush_mode=fm,
                                                  strategy=zlib.Z_FIXED if every % 2 else zlib.Z_DEFAULT_STRATEGY)))
    for idat in (1, 7, 8192):
        cases.append((f"idat{idat}", write(smooth(rng, 40, 50, 3), "cycle", idat=idat)))
    cases.append(("stored_blocks", write(noise(rng, 129, 300, 3), 0, level=0)))          # 116 KB at level 0: several stored blocks
    tile = noise(rng, 128, 85, 3)                              # rows of 256 bytes: the data repeats with period exactly 32768
    cases.append(("period32768", write(np.vstack([tile] * 3), 0, level=9)))
    for name, gen in (("noise", noise), ("smooth", smooth), ("screen", screenshot)):     # over 128 KiB: the window ring wraps
        for level in LEVELS:
            cases.append((f"wrap_{name}_l{level}", write(gen(rng, 224, 224, 3), "cycle" if level != 1 else 4, level=level)))
    cases.append(("wrap_grey_l6", write(smooth(rng, 300, 500, 1), "cycle1", level=6)))
    cases.append(("chunks_before", write(smooth(rng, 9, 9, 3), "cycle", before=chunk(b"gAMA", struct.pack(">I", 45455)) +
                                         chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1)) + chunk(b"tEXt", b"Comment\0hello") +
                                         chunk(b"sRGB", b"\0") + chunk(b"tIME", b"\x07\xe8\x01\x01\0\0\0") + chunk(b"bKGD", b"\0\0\0\0\0\0") +
                                         chunk(b"sBIT", b"\x08\x08\x08") + chunk(b"cHRM", struct.pack(">8I", *range(1, 9))))))
    return cases + bit_writer_cases(rng)


# ---- bit-level DEFLATE ------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):                               # LSB first (header fields, extra bits)
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):                               # Huffman codes go most significant bit first
        for k in range(nbits - 1, -1, -1):
            self.put(code >> k & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """code lengths -> {symbol: (code, length)} (RFC 1951 3.2.2; not validated: malformed sets are wanted too)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    res = {}
    for s, l in enumerate(lens):
        if l:
            res[s] = (nxt[l], l)
            nxt[l] += 1
    return res


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 13 + [5] * 6                                   # a complete code over all 19 code-length symbols


def put_tokens(bw, tokens, lit, dist):
    """tokens: int literal | ("m", length, distance) | ("sym", literal/length symbol) | ("mraw", length, distance symbol)"""
    for t in tokens:
        if isinstance(t, (int, np.integer)):
            bw.code(*lit[int(t)])
            continue
        if t[0] == "sym":
            bw.code(*lit[t[1]])
            continue
        length = t[1]
        ls = max(k for k in range(29) if LEN_BASE[k] <= length) if length < 258 else 28
        bw.code(*lit[257 + ls])
        bw.put(length - LEN_BASE[ls], LEN_EXTRA[ls])
        if t[0] == "mraw":
            bw.code(*dist[t[2]])
            continue
        ds = max(k for k in range(30) if DIST_BASE[k] <= t[2])
        bw.code(*dist[ds])
        bw.put(t[2] - DIST_BASE[ds], DIST_EXTRA[ds])


def expand(tokens):
    """what the literals and matches of a token list produce"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, (int, np.integer)):
            out.append(int(t))
        else:
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out)


def stored_block(bw, data, final, nlen=None):
    bw.put(final, 1)
    bw.put(0, 2)
    bw.align()
    bw.put(len(data), 16)
    bw.put(len(data) ^ 0xffff if nlen is None else nlen, 16)
    for b in data:
        bw.put(b, 8)


def fixed_block(bw, tokens, final, eob=True):
    bw.put(final, 1)
    bw.put(1, 2)
    put_tokens(bw, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))
    if eob:
        bw.code(*canonical(FIXED_LIT)[256])


def dynamic_header(bw, litlens, distlens, final, hlit=None, hdist=None, cl_syms=None):
    """the block header of a dynamic block; the code lengths are run-length coded over the JOINED sequence, so a run may go
    from the literal lengths into the distance lengths. cl_syms: [(code-length symbol, extra value)] instead of that coding."""
    bw.put(final, 1)
    bw.put(2, 2)
    bw.put((len(litlens) if hlit is None else hlit) - 257, 5)
    bw.put((len(distlens) if hdist is None else hdist) - 1, 5)
    bw.put(19 - 4, 4)
    for s in CL_ORDER:
        bw.put(CL_LENS[s], 3)
    cl = canonical(CL_LENS)
    if cl_syms is None:
        seq, cl_syms, k = list(litlens) + list(distlens), [], 0
        while k < len(seq):
            run = 1
            while k + run < len(seq) and seq[k + run] == seq[k]:
                run += 1
            if seq[k] == 0 and run >= 3:
                r = min(run, 138)
                cl_syms.append((18, r - 11) if r >= 11 else (17, r - 3))
                k += r
            elif run >= 4:
                r = min(run - 1, 6)
                cl_syms += [(seq[k], 0), (16, r - 3)]
                k += 1 + r
            else:
                cl_syms.append((seq[k], 0))
                k += 1
    for s, extra in cl_syms:
        bw.code(*cl[s])
        if s >= 16:
            bw.put(extra, (2, 3, 7)[s - 16])


def dynamic_block(bw, tokens, litlens, distlens, final, **kw):
    dynamic_header(bw, litlens, distlens, final, **kw)
    lit, dist = canonical(litlens), canonical(distlens)
    put_tokens(bw, tokens, lit, dist)
    bw.code(*lit[256])


def zwrap(deflated, raw, adler=None):
    a = zlib.adler32(raw) if adler is None else adler
    return b"\x78\x01" + deflated + struct.pack(">I", a & 0xffffffff)


def small_image(rng, h=6, w=5, values=None):
    """an RGB image whose filtered scanlines (filter None) hold only byte values from `values`"""
    values = list(range(15)) if values is None else values
    img = np.asarray(values, np.uint8)[rng.integers(0, len(values), (h, w, 3))]
    return img, filter_rows(img, [0] * h)


def lit15_lens():
    """a complete literal/length code with two 15-bit codes: byte values 0..14 get 1..15 bits, end-of-block the other 15-bit code"""
    lens = [0] * 257
    for v in range(15):
        lens[v] = v + 1
    lens[256] = 15
    return lens


def bit_writer_cases(rng):
    cases = []
    # a literal code with 15-bit codes (value 14 and end-of-block), a complete two-code distance code that is not used
    img, raw = small_image(rng)
    bw = BitWriter()
    dynamic_block(bw, list(raw), lit15_lens(), [1, 1], 1)
    cases.append(("bits_lit15", assemble(5, 6, 3, zwrap(bw.bytes(), raw))))
    # a code-length repeat that runs from the literal lengths into the distance lengths (zeros 263 .. 285, then four distance
    # zeros), and a single one-bit distance code (symbol 4: distances 5 and 6), used by matches. The bytes are 0 .. 4 only, so
    # that whatever lands on a row's first byte is a valid filter type.
    lens = lit15_lens()[:256] + [0] * 30
    lens[14], lens[256], lens[257 + 5] = 0, 15, 15               # length symbol 262: a match of 8
    tokens = [int(v) for v in rng.integers(0, 5, 7)] + [("m", 8, 6), ("m", 8, 5), ("m", 8, 6)]
    tokens += [int(v) for v in rng.integers(0, 5, 4 * 25 - 31)]
    bw = BitWriter()
    dynamic_block(bw, tokens, lens, [0, 0, 0, 0, 1], 1)
    cases.append(("bits_repeat_across_onebit_dist", assemble(8, 4, 3, zwrap(bw.bytes(), expand(tokens)))))
    # an empty dynamic block in front of the data, and a final empty stored block behind it
    img, raw = small_image(rng, 7, 9, list(range(256)))
    bw = BitWriter()
    dynamic_block(bw, [], lit15_lens(), [1, 1], 0)
    fixed_block(bw, list(raw[:50]), 0)
    stored_block(bw, raw[50:], 0)
    stored_block(bw, b"", 1)
    cases.append(("bits_empty_dynamic_first_empty_stored_last", assemble(9, 7, 3, zwrap(bw.bytes(), raw))))
    # an overlapping match (distance 1, length 258) and length symbol 284 with all extra bits set (also 258), fixed code
    tokens = [0, ("m", 258, 1), 3, 1, 2, ("m", 100, 3), ("m", 258, 2)] + [0] * (30 * 31 - 620)
    assert len(expand(tokens)) == 30 * 31
    bw = BitWriter()
    fixed_block(bw, tokens, 1)
    cases.append(("bits_overlap_fixed", assemble(30, 30, 1, zwrap(bw.bytes(), expand(tokens)))))
    return cases


# ---- the CPU restatement ----------------------------------------------------------------------------------------------------
def inflate_exact(stream, nbytes):
    """the rule of the device decoder on the CPU: valid raw DEFLATE data that ends after exactly nbytes bytes, followed by a
    matching Adler-32 -> the bytes, else None"""
    d = zlib.decompressobj(-15)
    try:
        raw = d.decompress(stream)
    except zlib.error:
        return None
    if not d.eof or len(raw) != nbytes or len(d.unused_data) < 4:
        return None
    if struct.unpack(">I", d.unused_data[:4])[0] != zlib.adler32(raw):
        return None
    return raw


def unfilter(raw, w, h, ch):
    """filtered scanlines -> uint8 [h][w][3] (grey replicated), None for a filter byte above 4"""
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * ch)
    out = np.zeros((h, w * ch), np.int32)
    prev = np.zeros(w * ch, np.int32)
    for y in range(h):
        ft, f = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        if ft > 4:
            return None
        cur = out[y]
        if ft == 0:
            cur[:] = f
        elif ft == 2:
            cur[:] = (f + prev) & 255
        elif ft == 1:
            cur[:] = (np.cumsum(f.reshape(w, ch), axis=0) & 255).reshape(-1)
        else:
            a = np.zeros(ch, np.int32)
            c = np.zeros(ch, np.int32)
            for x in range(w):
                b = prev[x * ch:(x + 1) * ch]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
                    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
                a = (f[x * ch:(x + 1) * ch] + pred) & 255
                cur[x * ch:(x + 1) * ch] = a
                c = b
        prev = cur
    px = out.astype(np.uint8).reshape(h, w, ch)
    return np.repeat(px, 3, axis=2) if ch == 1 else px


def cpu_decode(parsed):
    raw = inflate_exact(parsed.stream, parsed.raw_bytes())
    return None if raw is None else unfilter(raw, parsed.width, parsed.height, parsed.channels)


# ---- malformed files ---------------------------------------------------------------------------------------------------------
def _bits_file(build, raw, w=5, h=6, **kw):
    bw = BitWriter()
    build(bw)
    return assemble(w, h, 3, zwrap(bw.bytes(), raw, **kw))


def behind_idat_cases(rng):
    """([(name, file)] Pillow refuses, [(name, file)] Pillow accepts): valid 16 x 16 RGB images with something behind the IDAT
    run. Pillow's load_end() calls its chunk handlers there, without CRC checks, up to IEND: a handler that raises makes
    `convert("RGB")` fail although the pixels are complete."""
    img = smooth(rng, 16, 16)
    z = deflate(filter_rows(img, filters_for("cycle", 16)))

    def f(after, iend=True):
        return assemble(16, 16, 3, z, after=after, iend=iend)

    refused = [("sRGB_empty", f(chunk(b"sRGB", b""))), ("gAMA_2", f(chunk(b"gAMA", b"\0\1"))), ("pHYs_1", f(chunk(b"pHYs", b"\1"))),
               ("cHRM_2", f(chunk(b"cHRM", b"\0\1"))), ("iCCP_xxxx", f(chunk(b"iCCP", b"xxxx"))), ("IHDR_1", f(chunk(b"IHDR", b"\1"))),
               ("sRGB_bad_crc_empty", f(chunk(b"sRGB", b"", crc=7))),
               ("sRGB_past_end", f(struct.pack(">I", 1000) + b"sRGB" + b"\0" * 10, iend=False)),
               ("tIME_past_end", f(struct.pack(">I", 1000) + b"tIME" + b"\0" * 10, iend=False)),
               ("zzZz_past_end", f(chunk(b"tEXt", b"k\0v") + struct.pack(">I", 50) + b"zzZz" + b"\0" * 49, iend=False))]
    accepted = [("unknown_fits", f(chunk(b"zzZz", b"private data"))), ("unknown_bad_crc", f(chunk(b"zzZz", b"private", crc=3))),
                ("short_garbage", f(b"\1\2\3\4\5", iend=False)), ("not_a_chunk_type", f(struct.pack(">I", 1 << 30) + b"\xff\0!?" + b"rest", iend=False)),
                ("good_lengths", f(chunk(b"sRGB", b"\0") + chunk(b"gAMA", struct.pack(">I", 45455)) + chunk(b"pHYs", struct.pack(">IIB", 1, 1, 0)) +
                                   chunk(b"cHRM", struct.pack(">8I", *range(8))) + chunk(b"tEXt", b"Comment\0x") + chunk(b"tIME", b"1234567"))),
                ("after_iend_anything", f(b"") + chunk(b"sRGB", b"") + struct.pack(">I", 1000) + b"iCCP")]
    return refused, accepted


def malformed_corpus(rng):
    """[(family, file bytes)]. The "harmless" family holds files Pillow accepts with correct pixels and the device must
    decode as well; everything else is damaged in the stream itself."""
    corpus = []
    base = [(smooth(rng, 30, 40, 3), "cycle", 6), (noise(rng, 17, 23, 1), "cycle1", 9), (screenshot(rng, 64, 90, 3), 4, 1),
            (noise(rng, 40, 40, 3), 0, 0)]
    for img, mode, level in base:
        h, w, ch = img.shape
        raw = filter_rows(img, filters_for(mode, h))
        z = deflate(raw, level=level)
        for _ in range(12):                                    # bit flips in the stream (behind the zlib header)
            zz = bytearray(z)
            k = int(rng.integers(2, len(zz)))
            zz[k] ^= 1 << int(rng.integers(0, 8))
            corpus.append(("bitflip", assemble(w, h, ch, bytes(zz))))
        for _ in range(6):
            corpus.append(("truncated", assemble(w, h, ch, z[:int(rng.integers(2, len(z) - 4))])))
        corpus.append(("truncated", assemble(w, h, ch, z[:-8])))
        for ft in (5, 6, 17, 255):
            bad = bytearray(raw)
            bad[int(rng.integers(0, h)) * (1 + w * ch)] = ft
            corpus.append(("filter_byte", assemble(w, h, ch, deflate(bytes(bad), level=level))))
        corpus.append(("adler_wrong", assemble(w, h, ch, z[:-4] + struct.pack(">I", (zlib.adler32(raw) + 1) & 0xffffffff))))
        corpus.append(("adler_wrong", assemble(w, h, ch, z[:-1] + bytes([z[-1] ^ 0x80]))))
        corpus.append(("adler_missing", assemble(w, h, ch, z[:-4])))
        corpus.append(("extra_rows", assemble(w, h, ch, deflate(raw + raw[:2 * (1 + w * ch)], level=level))))
        corpus.append(("short_data", assemble(w, h, ch, deflate(raw[:-5], level=level))))
        good = assemble(w, h, ch, z, idat=1 << 30)
        corpus.append(("harmless", assemble(w, h, ch, z + b"garbage behind the stream")))
        corpus.append(("harmless", good + b"bytes after IEND"))
        corpus.append(("harmless", assemble(w, h, ch, z, iend=False)))
        corpus.append(("harmless", assemble(w, h, ch, z, after=chunk(b"tEXt", b"k\0v", crc=12345))))
        k = good.index(b"IDAT") + 4 + len(z)                    # (one IDAT chunk: its CRC follows the stream)
        corpus.append(("harmless", good[:k] + bytes([good[k] ^ 0xff]) + good[k + 1:]))
    refused, accepted = behind_idat_cases(rng)
    corpus += [("behind_idat", b) for _, b in refused] + [("harmless", b) for _, b in accepted]
    # streams from the bit writer: what a DEFLATE decoder has to refuse
    img, raw = small_image(rng)
    lit, one = lit15_lens(), [1, 1]
    corpus.append(("block_type_3", _bits_file(lambda bw: (bw.put(1, 1), bw.put(3, 2), bw.put(0, 29)), raw)))
    corpus.append(("len_nlen", _bits_file(lambda bw: stored_block(bw, raw, 1, nlen=len(raw)), raw)))
    over = list(lit)
    over[20] = over[21] = 1                                    # three one-bit codes
    corpus.append(("oversubscribed", _bits_file(lambda bw: dynamic_block(bw, list(raw), over, one, 1), raw)))
    inc = list(lit)
    inc[0] = 0                                                 # the one-bit code is missing
    corpus.append(("incomplete", _bits_file(lambda bw: dynamic_block(bw, [b or 1 for b in raw], inc, one, 1), raw)))
    inc2 = [0] * 257
    inc2[0], inc2[256] = 2, 2                                  # two two-bit codes
    corpus.append(("incomplete", _bits_file(lambda bw: dynamic_block(bw, [0] * len(raw), inc2, one, 1), bytes(len(raw)))))
    corpus.append(("incomplete", _bits_file(lambda bw: dynamic_block(bw, list(raw), lit, [2, 2], 1), raw)))     # distance code
    no256 = list(lit)
    no256[256], no256[15] = 0, 15
    corpus.append(("missing_256", _bits_file(lambda bw: (dynamic_header(bw, no256, one, 1), bw.put(0, 64)), raw)))
    for hlit in (287, 288):
        corpus.append(("hlit_hdist", _bits_file(lambda bw, hl=hlit: (dynamic_header(bw, lit + [0] * (hl - 257), one, 1),
                                                                      put_tokens(bw, list(raw) + [("sym", 256)], canonical(lit), {})), raw)))
    for hdist in (31, 32):
        corpus.append(("hlit_hdist", _bits_file(lambda bw, hd=hdist: (dynamic_header(bw, lit, [5] * hd, 1),
                                                                       put_tokens(bw, list(raw) + [("sym", 256)], canonical(lit), {})), raw)))
    corpus.append(("repeat_no_previous", _bits_file(lambda bw: (dynamic_header(bw, lit, one, 1, cl_syms=[(16, 0)] + [(0, 0)] * 260),
                                                                bw.put(0, 64)), raw)))
    corpus.append(("repeat_overrun", _bits_file(lambda bw: (dynamic_header(bw, lit, one, 1, cl_syms=[(8, 0)] + [(18, 127)] * 3),
                                                            bw.put(0, 64)), raw)))
    corpus.append(("distance_too_far", _bits_file(lambda bw: fixed_block(bw, list(raw[:10]) + [("m", 3, 11)] + list(raw[13:]), 1), raw)))
    corpus.append(("distance_too_far", _bits_file(lambda bw: fixed_block(bw, [("m", 3, 1)] + list(raw[3:]), 1), raw)))
    for s in (286, 287):
        corpus.append(("bad_symbol", _bits_file(lambda bw, s=s: fixed_block(bw, list(raw[:10]) + [("sym", s)] + list(raw[10:]), 1), raw)))
    for ds in (30, 31):
        corpus.append(("bad_symbol", _bits_file(lambda bw, ds=ds: fixed_block(bw, list(raw[:10]) + [("mraw", 3, ds)] + list(raw[13:]), 1), raw)))
    corpus.append(("no_final_eob", _bits_file(lambda bw: (fixed_block(bw, list(raw), 1, eob=False), bw.put(0x7fffffff, 31)), raw)))
    return corpus
