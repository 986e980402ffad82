"""Alpha, palette and low-depth PNG files on the device (clipmi_png_decode_px8, clipmi_resize_crop_rgba8, clipmi_nearest_crop_p8)
against Pillow itself and the committed Pillow pixels. No tolerance: a file the device keeps (status 0) decodes to exactly
Pillow's own-mode pixels and transforms to exactly `decode_worker.load_uint8`'s bytes; a file Pillow refuses never comes back;
anything else is handed back and Pillow decides."""
import collections
import io
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from clipmi import png, png_parse
import png_cases
import png_mode_cases as M

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Palette images with Transparency")]
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_modes.npz")
WIDTHS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 32, 33, 300]          # sub-byte rows that end inside a byte; 4- and 2-byte pixel rows on
HEIGHTS = [1, 2, 63, 64, 65, 129]                              # either side of a 64-byte wave; heights on either side of a band
MODE_LIST = list(M.MODES)                                      # (colour type, depth)


def same(got, blob):
    """what decode_files(modes=True) returned for a file == Pillow's own-mode pixels (and palette)"""
    kind, ref = M.pillow_pixels(blob)
    if kind == "index":
        return isinstance(got, tuple) and np.array_equal(got[0], ref) and np.array_equal(got[1], M.pillow_palette(blob)[0])
    return not isinstance(got, tuple) and got.shape == ref.shape and np.array_equal(got, ref)


def live_batch():
    rng = np.random.default_rng(31)
    files = []
    k = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for _ in range(3):                                 # three of the nine modes per size, in turn: 216 files
                ctype, depth = MODE_LIST[k % len(MODE_LIST)]
                fmode, level = png_cases.MODES[(k // 2) % 8], png_cases.LEVELS[(k // 5) % 4]
                files.append((f"w{w}h{h}_c{ctype}d{depth}_f{fmode}_l{level}",
                              M.mode_file(rng, ctype, depth, h, w, k, fmode, with_trns=ctype == 3 and k % 2 == 0, level=level)))
                k += 1
    for ctype, depth in MODE_LIST:                             # each filter on every row and the cycling modes, every mode, two bands;
        for j, fmode in enumerate(png_cases.MODES):            # every filter mode at every level
            files.append((f"filter{fmode}_c{ctype}d{depth}", M.mode_file(rng, ctype, depth, 70, 37, k, fmode, level=png_cases.LEVELS[(j + depth) % 4])))
            k += 1
    for fmode in png_cases.MODES:
        for level in png_cases.LEVELS:
            ctype, depth = ((6, 8), (3, 4), (4, 8), (0, 2))[png_cases.LEVELS.index(level)]
            files.append((f"mode{fmode}_l{level}_c{ctype}", M.mode_file(rng, ctype, depth, 65, 17, k, fmode, level=level)))
            k += 1
    for what in ("RGBA", "LA", "P1", "P2", "P4", "P8", "P8t", "P4t", "1"):     # Pillow's own encoder: bits=, transparency=
        for (h, w) in ((1, 1), (5, 7), (64, 64), (65, 63), (13, 300), (224, 224)):
            files.append((f"pillow_{what}_{h}x{w}", M.pillow_mode_file(rng, what, h, w, k)))
            k += 1
    files.append(("idat1", M.mode_file(rng, 6, 8, 20, 21, 0, "cycle", idat=1)))
    files.append(("fixed_wb9", M.mode_file(rng, 3, 2, 65, 64, 1, "cycle4", strategy=zlib.Z_FIXED, wbits=9)))
    files.append(("short_palette", M.mode_file(rng, 3, 8, 40, 50, 1, "cycle1", entries=77)))
    files.append(("rgba_480x640", M.mode_file(rng, 6, 8, 480, 640, 2, "cycle", level=1)))      # over 1 MB of scanlines: the ring wraps
    return files


def test_device_decode_equals_pillow_live():
    """Every valid file of the writer and of Pillow's encoder, every kind: none may be handed back, all equal Pillow."""
    files = live_batch()
    assert len(files) >= 150
    kinds = collections.Counter()
    for name, b in files:
        p = png_parse.parse(b, modes=True)
        kinds[(p.ctype, p.depth)] += 1
    assert set(kinds) == set(M.MODES), kinds
    got = png.decode_files([b for _, b in files], DEV, modes=True)
    handed_back = [name for (name, _), g in zip(files, got) if g is None]
    assert not handed_back, handed_back
    wrong = [name for (name, b), g in zip(files, got) if not same(g, b)]
    assert not wrong, wrong
    # without the flag nothing of this comes back
    assert all(g is None for g in png.decode_files([b for _, b in files[::7]], DEV))


def test_widest_rows():
    """The widest rows the parser lets through fill the unfilter kernel's LDS row: RGBA 12288 pixels (49152 bytes), an 8-bit
    palette row of MAX_WIDTH; more than one band each"""
    rng = np.random.default_rng(32)
    rgba = np.concatenate([png_cases.screenshot(rng, 65, 12288, 3), M.alpha_plane(rng, 65, 12288, "smooth")[..., None]], axis=2)
    idx = (png_cases.screenshot(rng, 65, png_parse.MAX_WIDTH, 1).astype(np.int64) * 200 >> 8).astype(np.uint8)
    la = np.concatenate([png_cases.screenshot(rng, 66, png_parse.MAX_WIDTH - 1, 1), M.alpha_plane(rng, 66, png_parse.MAX_WIDTH - 1, "binary")[..., None]], axis=2)
    blobs = [M.write(rgba, 6, 8, "cycle1", level=1), M.write(idx, 3, 8, 4, palette=rng.integers(0, 256, (200, 3), dtype=np.uint8), level=1),
             M.write(la, 4, 8, "cycle4", level=1), M.mode_file(rng, 3, 1, 65, png_parse.MAX_WIDTH - 3, 0, "cycle", level=1)]
    got = png.decode_files(blobs, DEV, modes=True)
    for k, (b, g) in enumerate(zip(blobs, got)):
        assert g is not None and same(g, b), k


@pytest.fixture(scope="module")
def transform_cases():
    return M.transform_cases(np.random.default_rng(21))


@pytest.mark.parametrize("n_px", [32, 224])
def test_transform_equals_load_uint8(transform_cases, n_px):
    """decode + transform on the device, every size x every kind (the 8-bit grey and RGB kind included): the reference's
    transform, bit for bit. The sizes cover no resampling, one axis only, both, up and down; the alpha planes are noise, smooth
    and binary."""
    assert len(transform_cases) == len(M.SIZES) * (len(M.KINDS) + 2)
    got = png.transform_files([b for _, b in transform_cases], n_px, DEV)
    handed_back = [name for (name, _), g in zip(transform_cases, got) if g is None]
    assert not handed_back, handed_back
    wrong = []
    for (name, b), g in zip(transform_cases, got):
        ref = M.load_uint8_blob(b, n_px)
        if g.shape != ref.shape or not np.array_equal(g, ref):
            wrong.append((name, int((g != ref).sum()) if g.shape == ref.shape else g.shape))
    assert not wrong, wrong


def test_a_sample_beyond_the_palette_goes_back_to_pillow():
    rng = np.random.default_rng(33)
    pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    blobs, beyond = [], []
    for depth, entries, top in ((4, 5, 16), (8, 77, 256), (2, 3, 4), (1, 1, 2), (8, 255, 256)):
        for (h, w) in ((9, 13), (70, 37)):
            inside = rng.integers(0, entries, (h, w, 1), dtype=np.uint8)
            blobs.append(M.write(inside, 3, depth, "cycle", palette=pal[:entries]))
            beyond.append(False)
            out = inside.copy()
            out[h - 1, w - 1, 0] = entries                                    # one sample, the last one, just beyond the palette
            blobs.append(M.write(out, 3, depth, "cycle", palette=pal[:entries]))
            beyond.append(True)
            blobs.append(M.write(rng.integers(0, top, (h, w, 1), dtype=np.uint8) | (top - 1) * (rng.integers(0, 9, (h, w, 1)) == 0).astype(np.uint8),
                                 3, depth, "cycle1", palette=pal[:entries]))
            beyond.append(True)
    for b, far in zip(blobs, beyond):
        assert (M.cpu_decode(png_parse.parse(b, modes=True)) is None) == far
    got = png.decode_files(blobs, DEV, modes=True)
    for k, (b, g, far) in enumerate(zip(blobs, got, beyond)):
        if far:
            assert g is None, k
        else:
            assert g is not None and same(g, b), k
    back = png.transform_files(blobs, 32, DEV)
    assert [g is None for g in back] == beyond


def malformed_corpus(rng):
    """[(family, file)]: the damage of png_cases.malformed_corpus placed in RGBA and 4-bit palette files"""
    corpus = []
    pal = rng.integers(0, 256, (16, 3), dtype=np.uint8)
    base = [(6, 8, M.samples_for(rng, 6, 8, 30, 40, 1)[0], "cycle", 6, b""), (3, 4, rng.integers(0, 16, (64, 91, 1), dtype=np.uint8), "cycle1", 9, M.plte(pal)),
            (6, 8, M.samples_for(rng, 6, 8, 65, 22, 2)[0], 4, 1, b""), (3, 4, rng.integers(0, 16, (40, 41, 1), dtype=np.uint8), 0, 0, M.plte(pal) + M.trns([3, 4]))]
    for ctype, depth, s, fmode, level, before in base:
        h, w, ch = s.shape
        raw = M.scanlines(s, ctype, depth, fmode)
        stride = len(raw) // h
        z = png_cases.deflate(raw, level=level)

        def f(zz, **kw):
            return png_cases.assemble(w, h, ch, zz, before=before, depth=depth, ctype=ctype, **kw)

        for _ in range(12):
            zz = bytearray(z)
            k = int(rng.integers(2, len(zz)))
            zz[k] ^= 1 << int(rng.integers(0, 8))
            corpus.append(("bitflip", f(bytes(zz))))
        for _ in range(6):
            corpus.append(("truncated", f(z[:int(rng.integers(2, len(z) - 4))])))
        corpus.append(("truncated", f(z[:-8])))
        for ft in (5, 6, 17, 255):
            bad = bytearray(raw)
            bad[int(rng.integers(0, h)) * stride] = ft
            corpus.append(("filter_byte", f(png_cases.deflate(bytes(bad), level=level))))
        corpus.append(("adler_wrong", f(z[:-4] + struct.pack(">I", (zlib.adler32(raw) + 1) & 0xffffffff))))
        corpus.append(("adler_wrong", f(z[:-1] + bytes([z[-1] ^ 0x80]))))
        corpus.append(("adler_missing", f(z[:-4])))
        corpus.append(("extra_rows", f(png_cases.deflate(raw + raw[:2 * stride], level=level))))
        corpus.append(("short_data", f(png_cases.deflate(raw[:-5], level=level))))
        corpus.append(("harmless", f(z + b"garbage behind the stream")))
        corpus.append(("harmless", f(z, idat=1 << 30) + b"bytes after IEND"))
        corpus.append(("harmless", f(z, iend=False)))
        corpus.append(("harmless", f(z, after=png_cases.chunk(b"tEXt", b"k\0v", crc=12345))))
        corpus.append(("behind_idat", f(z, after=png_cases.chunk(b"sRGB", b""))))
    return corpus


def test_malformed_files_never_return_wrong_pixels():
    """Every status-0 file equals Pillow; a file Pillow refuses never comes back; the "harmless" files, which Pillow accepts, all
    come back from the device (so that handing everything back does not pass); a wrong Adler-32 always goes back."""
    corpus = malformed_corpus(np.random.default_rng(78))
    got = png.decode_files([b for _, b in corpus], DEV, modes=True)
    counts = collections.defaultdict(lambda: [0, 0, 0, 0])     # family -> [files, device pixels, handed back, Pillow refuses]
    for (fam, b), g in zip(corpus, got):
        c = counts[fam]
        c[0] += 1
        try:
            Image.open(io.BytesIO(b)).convert("RGB")
            refuses = False
        except Exception:
            refuses = True
        if refuses:
            c[3] += 1
            assert g is None, f"{fam}: the device returned pixels for a file Pillow refuses"
        elif g is None:
            c[2] += 1
        else:
            c[1] += 1
            assert same(g, b), f"{fam}: status 0 with pixels that are not Pillow's"
    for fam, (n, ok, back, refused) in sorted(counts.items()):
        print(f"{fam:20s} files {n:5d}  device pixels {ok:5d}  handed back {back:5d}  Pillow refuses {refused:5d}")
    assert counts["harmless"][0] == 16 and counts["harmless"][1] == 16
    assert counts["adler_wrong"][0] == 8 and counts["adler_wrong"][1] == 0
    assert counts["filter_byte"][0] == 16 and counts["filter_byte"][1] == 0
    assert counts["behind_idat"][3] == counts["behind_idat"][0] == 4
    assert counts["bitflip"][0] == 48 and counts["truncated"][0] == 28


def test_golden_files_give_the_committed_pillow_pixels():
    d = np.load(GOLDEN)
    n, n_px = int(d["n"]), int(d["n_px"])
    assert n >= 30 and os.path.getsize(GOLDEN) <= 282060
    blobs = [d[f"file_{i}"].tobytes() for i in range(n)]
    got = png.decode_files(blobs, DEV, modes=True)
    out = png.transform_files(blobs, n_px, DEV)
    kinds = set()
    for i in range(n):
        kind = str(d[f"kind_{i}"])
        kinds.add(kind)
        assert got[i] is not None and out[i] is not None, i
        if kind == "index":
            assert np.array_equal(got[i][0], d[f"px_{i}"]) and np.array_equal(got[i][1], d[f"palette_{i}"]), i
        else:
            assert np.array_equal(got[i], d[f"px_{i}"]), i
        assert np.array_equal(out[i], d[f"out_{i}"]), i
    assert kinds == {"alpha", "index"}
