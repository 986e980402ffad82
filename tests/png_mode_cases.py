"""PNG files of the modes behind `png_parse.parse(modes=True)` for the tests of the device decoder: RGBA, grey + alpha, palette
files at depth 1/2/4/8 with and without tRNS, grey at depth 1/2/4. No tests here.

A writer for them on top of png_cases (samples packed most significant bits first, the filter applied with the byte unit as
`ch`), Pillow's own encoder for the same modes, and the CPU restatement of what Pillow's transform does to such files: the
decode to the file's own-mode pixels, the premultiplied bicubic rule for images with alpha, the nearest rule for index images.
"""
import io

import numpy as np
from PIL import Image

from clipmi import decode_worker
import png_cases

SAMPLES = {6: 4, 4: 2, 3: 1, 0: 1}                             # colour type -> samples per pixel
# (colour type, depth) of every mode the flag adds, and the kind the parser gives it
MODES = {(6, 8): "alpha", (4, 8): "alpha", (0, 2): "alpha", (0, 4): "alpha",
         (3, 1): "index", (3, 2): "index", (3, 4): "index", (3, 8): "index", (0, 1): "index"}


# ---- the writer -------------------------------------------------------------------------------------------------------------
def pack_rows(samples, depth):
    """samples uint8 [h][w][ch], each < 1 << depth -> the scanlines' bytes uint8 [h][ceil(w * ch * depth / 8)], most significant
    bits first, the last byte of a row padded with zero bits"""
    h, w, ch = samples.shape
    flat = samples.reshape(h, w * ch)
    if depth == 8:
        return flat.copy()
    bits = ((flat[:, :, None] >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8).reshape(h, w * ch * depth)
    return np.packbits(bits, axis=1)


def plte(palette):
    return png_cases.chunk(b"PLTE", np.asarray(palette, np.uint8).reshape(-1, 3).tobytes())


def trns(alphas):
    return png_cases.chunk(b"tRNS", bytes(int(a) for a in alphas))


def scanlines(samples, ctype, depth, mode="cycle"):
    """the filtered scanlines of a file: the filter unit is the pixel's bytes, 1 below depth 8"""
    h = samples.shape[0]
    rows = pack_rows(samples, depth)
    unit = SAMPLES[ctype] if depth == 8 else 1
    return png_cases.filter_rows(rows.reshape(h, rows.shape[1] // unit, unit), png_cases.filters_for(mode, h))


def write(samples, ctype, depth, mode="cycle", palette=None, alphas=None, idat=8192, before=b"", **kw):
    """samples uint8 [h][w][samples per pixel] -> a PNG file of that colour type and depth. palette: [n][3] for colour type 3;
    alphas: a tRNS chunk behind it."""
    h, w, ch = samples.shape
    assert ch == SAMPLES[ctype]
    if ctype == 3:
        before = before + plte(palette) + (trns(alphas) if alphas is not None else b"")
    z = png_cases.deflate(scanlines(samples, ctype, depth, mode), **kw)
    return png_cases.assemble(w, h, ch, z, idat=idat, before=before, depth=depth, ctype=ctype)


# ---- images -----------------------------------------------------------------------------------------------------------------
def alpha_plane(rng, h, w, how):
    if how == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if how == "smooth":
        return png_cases.smooth(rng, h, w, 1)[..., 0]
    return (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)         # "binary"


def samples_for(rng, ctype, depth, h, w, k=0, entries=None):
    """-> (samples uint8 [h][w][ch], palette or None): k chooses among noise, smooth and screenshot-like content and among the
    alpha planes"""
    gen = (png_cases.noise, png_cases.smooth, png_cases.screenshot)[k % 3]
    if ctype in (6, 4):
        col = gen(rng, h, w, 3 if ctype == 6 else 1)
        a = alpha_plane(rng, h, w, ("noise", "smooth", "binary")[(k // 3) % 3])
        return np.concatenate([col, a[..., None]], axis=2), None
    top = 1 << depth
    if ctype == 3:
        entries = top if entries is None else entries
        idx = (gen(rng, h, w, 1).astype(np.int64) * entries >> 8).astype(np.uint8) if k % 2 else rng.integers(0, entries, (h, w, 1), dtype=np.uint8)
        return idx, rng.integers(0, 256, (entries, 3), dtype=np.uint8)
    return (gen(rng, h, w, 1) >> (8 - depth)).astype(np.uint8), None


def mode_file(rng, ctype, depth, h, w, k=0, mode="cycle", with_trns=False, entries=None, **kw):
    s, pal = samples_for(rng, ctype, depth, h, w, k, entries)
    alphas = rng.integers(0, 256, int(rng.integers(1, len(pal) + 1))) if with_trns else None
    return write(s, ctype, depth, mode, palette=pal, alphas=alphas, **kw)


def save(img, **kw):
    buf = io.BytesIO()
    img.save(buf, format="PNG", **kw)
    return buf.getvalue()


def pillow_mode_file(rng, what, h, w, k=0):
    """a file of Pillow's own encoder: what in "RGBA", "LA", "P1", "P2", "P4", "P8" (palette saved with bits=), "P8t" / "P4t"
    (with transparency=), "1" """
    if what in ("RGBA", "LA"):
        s, _ = samples_for(rng, 6 if what == "RGBA" else 4, 8, h, w, k)
        return save(Image.fromarray(s, what), compress_level=(0, 1, 6, 9)[k % 4])
    if what == "1":
        return save(Image.fromarray(png_cases.smooth(rng, h, w, 1)[..., 0] > 128))
    bits = int(what[1])
    s, pal = samples_for(rng, 3, bits, h, w, k)
    img = Image.fromarray(s[..., 0], "P")
    img.putpalette(pal.reshape(-1).tolist())
    kw = {"transparency": bytes(rng.integers(0, 256, len(pal), dtype=np.uint8))} if what.endswith("t") else {}
    return save(img, bits=bits, **kw)


# ---- Pillow as the reference ------------------------------------------------------------------------------------------------
def pillow_pixels(blob):
    """what decode_files(modes=True) has to return for a file, from Pillow: ("alpha", uint8 [h][w][4]) = convert("RGBA") of an
    RGBA, LA or L file; ("index", uint8 [h][w]) = the indices of a P file, 0 / 1 for a mode "1" file"""
    im = Image.open(io.BytesIO(blob))
    if im.mode in ("RGBA", "LA", "L"):
        return "alpha", np.asarray(im.convert("RGBA"))
    if im.mode == "P":
        return "index", np.asarray(im)
    assert im.mode == "1", im.mode
    return "index", np.asarray(im).astype(np.uint8)


def pillow_palette(blob):
    """the palette Pillow read, uint8 [256][3], zero beyond its entries; black, white for a mode "1" file"""
    im = Image.open(io.BytesIO(blob))
    pal = np.zeros((256, 3), np.uint8)
    if im.mode == "1":
        pal[1] = 255
        return pal, 2
    im.load()
    raw = np.frombuffer(im.palette.tobytes(), np.uint8).reshape(-1, 3)
    pal[:len(raw)] = raw
    return pal, len(raw)


# ---- the CPU restatement ----------------------------------------------------------------------------------------------------
def cpu_decode(p):
    """png_parse.Parsed of kind "alpha" or "index" -> uint8 [h][w][4] or uint8 [h][w] (None where the device would report the
    file: the rule of png_cases.cpu_decode, and an index beyond the palette)"""
    raw = png_cases.inflate_exact(p.stream, p.raw_bytes())
    if raw is None:
        return None
    unit = p.channels if p.depth == 8 else 1
    rows = png_cases.unfilter(raw, p.row_bytes() // unit, p.height, unit)
    if rows is None:
        return None
    rows = (rows[..., 0] if unit == 1 else rows).reshape(p.height, p.row_bytes())
    if p.depth < 8:
        bits = np.unpackbits(rows, axis=1)[:, :p.width * p.depth].reshape(p.height, p.width, p.depth)
        s = (bits.astype(np.int64) << np.arange(p.depth - 1, -1, -1)).sum(axis=2).astype(np.uint8)
    else:
        s = rows.reshape(p.height, p.width, p.channels)
    if p.kind == "index":
        s = s.reshape(p.height, p.width)
        return None if int(s.max()) >= p.n_entries else s
    if p.ctype == 6:
        return s
    if p.ctype == 4:
        return np.concatenate([np.repeat(s[..., :1], 3, axis=2), s[..., 1:]], axis=2)
    v = (s.reshape(p.height, p.width).astype(np.int64) * (85 if p.depth == 2 else 17)).astype(np.uint8)
    return np.stack([v, v, v, np.full_like(v, 255)], axis=2)


def _resample(img, first, count, kk, axis):
    """one pass of Pillow's 8-bit resampling along `axis` of img uint8 [h][w][c] (decode_worker.coeffs_window's tables)"""
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(first),) + img.shape[1:], np.int64)
    for o in range(len(first)):
        taps = img[first[o]:first[o] + count[o]]
        out[o] = (1 << 21) + np.tensordot(kk[o, :count[o]].astype(np.int64), taps, axes=1)
    return np.moveaxis(np.clip(out >> 22, 0, 255).astype(np.uint8), 0, axis)


def _blocks(plan, n_px):
    h = v = None
    if plan["need_h"]:
        c = plan["hcoef"]
        h = (c[:n_px], c[n_px:2 * n_px], c[2 * n_px:].reshape(n_px, plan["hk"]))
    if plan["need_v"]:
        c = plan["vcoef"]
        v = (c[:n_px], c[n_px:2 * n_px], c[2 * n_px:].reshape(n_px, plan["vk"]))
    return h, v


def premultiply(rgba):
    t = rgba[..., :3].astype(np.int64) * rgba[..., 3:].astype(np.int64) + 128
    return np.concatenate([(((t >> 8) + t) >> 8).astype(np.uint8), rgba[..., 3:]], axis=2)


def unpremultiply(rgba):
    c, a = rgba[..., :3].astype(np.int64), rgba[..., 3:].astype(np.int64)
    return np.where((a == 0) | (a == 255), c, np.minimum(255, 255 * c // np.maximum(a, 1))).astype(np.uint8)


def cpu_transform_alpha(rgba, n_px):
    """uint8 [h][w][4] -> the transform's uint8 [3][n_px][n_px]: resize in the premultiplied mode (where anything is resampled),
    centre crop, drop alpha"""
    h, w = rgba.shape[:2]
    plan = decode_worker.resize_plan(w, h, n_px)
    left, top = plan["left"], plan["top"]
    if not plan["need_h"] and not plan["need_v"]:
        return np.ascontiguousarray(rgba[top:top + n_px, left:left + n_px, :3].transpose(2, 0, 1))
    hb, vb = _blocks(plan, n_px)
    r0 = plan["r0"]                                            # (only the rows the window needs, as on the device)
    x = premultiply(rgba[r0:r0 + plan["nrows"]])
    x = _resample(x, *hb, axis=1) if hb else x[:, left:left + n_px]
    x = _resample(x, vb[0] - r0, vb[1], vb[2], axis=0) if vb else x[top - r0:top - r0 + n_px]
    return np.ascontiguousarray(unpremultiply(x).transpose(2, 0, 1))


def cpu_transform_index(idx, palette, n_px):
    """uint8 [h][w] indices, palette uint8 [256][3] -> the transform's uint8 [3][n_px][n_px]: nearest resize, centre crop, palette"""
    h, w = idx.shape
    plan = decode_worker.nearest_plan(w, h, n_px)
    return np.ascontiguousarray(palette[idx[plan["vcoef"]][:, plan["hcoef"]]].transpose(2, 0, 1))


def cpu_transform(p, n_px, px=None):
    px = cpu_decode(p) if px is None else px
    return cpu_transform_index(px, p.palette, n_px) if p.kind == "index" else cpu_transform_alpha(px, n_px)


SIZES = [(224, 224), (225, 223), (37, 70), (70, 37), (300, 260), (480, 640), (1, 5), (5, 1), (224, 500), (600, 230), (33, 33), (9, 200)]
# every kind of file, as (name, colour type, depth, tRNS): the "every kind" of the transform tests
KINDS = [("rgba", 6, 8, False), ("la", 4, 8, False), ("p8", 3, 8, False), ("p8t", 3, 8, True), ("p4", 3, 4, False), ("p4t", 3, 4, True),
         ("p2", 3, 2, False), ("p1", 3, 1, False), ("g1", 0, 1, False), ("g2", 0, 2, False), ("g4", 0, 4, False)]


OLD = ("l8_", "rgb8_")                                         # names of the 8-bit grey and RGB files among transform_cases


def transform_cases(rng):
    """[(name, file)]: SIZES x KINDS (alpha planes noise, smooth and binary in turn), plus the existing grey and RGB kind"""
    cases = []
    k = 0
    for (h, w) in SIZES:
        for name, ctype, depth, t in KINDS:
            entries = None if depth != 8 or k % 2 else 77          # 8-bit palettes: full, and short of 256 entries
            # (filters None, Sub and Up: the CPU restatement undoes them a row at a time; every filter is the decode tests' part)
            cases.append((f"{name}_{h}x{w}", mode_file(rng, ctype, depth, h, w, k, k % 3, with_trns=t, entries=entries if ctype == 3 else None,
                                                      level=(1, 6, 9)[k % 3])))
            k += 1
        for ch in (1, 3):
            cases.append((f"{OLD[ch == 3]}{h}x{w}", png_cases.write(png_cases.smooth(rng, h, w, ch), "cycle", level=6)))
    return cases


def load_uint8_blob(blob, n_px):
    return decode_worker.load_uint8(io.BytesIO(blob), n_px)
