"""JPEG files of the layouts `jpeg_parse.parse(layouts=True)` adds, for the tests: forged fixtures and a CPU restatement.

Pillow's encoder writes neither luma sampling 1x2 (4:4:0), 4x1 (4:1:1) or 1x4 nor RGB-coded files, so the fixtures are FORGED:
a Pillow file's frame header is relabelled so that the MCU count - and with it the entropy-coded data - stays valid. The picture is
scrambled, which does not matter to a decoder that has to reproduce Pillow's bytes of the very same file.

  layout  source file                      frame header edit
  1x2     subsampling=1 file of W x H      luma factor byte 0x12, frame width and height swapped           -> H x W
  4x1     subsampling=2 file of 2H x w     luma 0x41, width 2w or 2w - 1, height H                          -> H x W, w = ceil(W / 2)
  1x4     subsampling=2 file of h x 2W     luma 0x14, width W, height 2h or 2h - 1                          -> H x W, h = ceil(H / 2)
  rgb     any of the above, or a Pillow    the APP0 JFIF segment replaced by an APP14 Adobe segment with transform 0: libjpeg
          file as it is                    then takes the three components for R, G, B

Progressive files relabel the same way at their SOF2 marker; the block counts of their non-interleaved scans agree for 1x2 at
every size, and for 4x1 / 1x4 where the source's sides are multiples of 16 (`forge` asserts that).

restate(blob): what `Image.open(f).convert("RGB")` gives for such a file, from oracle/jpeg_oracle.py's entropy decode and IDCT
(progressive: tests/jpeg_progressive.py's) and libjpeg-turbo's upsampling rules for these layouts:
  1x2   h1v2_fancy_upsample: row 2cy = (3 p[cy] + p[cy - 1] + 1) >> 2, row 2cy + 1 = (3 p[cy] + p[cy + 1] + 2) >> 2, the neighbour
        row clamped to the chroma rows under the image; no horizontal filtering and no width condition
  4x1, 1x4   int_upsample: plain replication
  rgb   the three upsampled planes are the pixels
It is pinned against Pillow live and against the committed pixels in tests/test_jpeg_layouts.py.

tools/jpeg_layouts_ab.py imports `forge` from here for its 4:4:0 files (Pillow writes none): keep its signature when this changes.
"""
import io

import numpy as np
from PIL import Image, ImageFile

import jpeg_progressive
from clipmi import jpeg_parse
from oracle import jpeg_oracle

LAYOUTS = ("1x2", "4x1", "1x4")
FACTORS = {"1x2": (1, 2), "4x1": (4, 1), "1x4": (1, 4)}
ADOBE_RGB = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"            # APP14: version 100, flags 0 0, transform 0


def smooth(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 100 * np.sin(xx / 9.0 + yy / 17.0), 127 + 100 * np.cos(xx / 13.0 - yy / 7.0), (xx * 3 + yy * 2) % 256], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(a, **kw):
    buf = io.BytesIO()
    old, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, 1 << 24          # (Pillow's default buffer is too small for progressive noise)
    try:
        Image.fromarray(a).save(buf, format="JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return buf.getvalue()


def pillow(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def _sof(blob):
    """Offset of the file's SOF0 / SOF1 / SOF2 marker"""
    i = 2
    while True:
        assert blob[i] == 0xFF, "marker expected"
        m = blob[i + 1]
        if m in (0xC0, 0xC1, 0xC2):
            return i
        assert m != 0xDA, "no frame header"
        i += 2 + ((blob[i + 2] << 8) | blob[i + 3])


def relabel(blob, luma=None, width=None, height=None, comp=0):
    """blob with the frame header's size and the sampling factor byte of component `comp` replaced (None: left as it is)"""
    s = _sof(blob)
    b = bytearray(blob)
    if height is not None:
        b[s + 5:s + 7] = height.to_bytes(2, "big")
    if width is not None:
        b[s + 7:s + 9] = width.to_bytes(2, "big")
    if luma is not None:
        b[s + 11 + 3 * comp] = luma
    return bytes(b)


def rgb_coded(blob):
    """blob with its APP0 JFIF segment replaced by an APP14 Adobe segment with transform 0"""
    assert blob[2:4] == b"\xff\xe0" and blob[6:11] == b"JFIF\0"
    return blob[:2] + ADOBE_RGB + blob[4 + ((blob[4] << 8) | blob[5]):]


JFIF = b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"


def source_of(blob, layout, H, W, rgb=False):
    """forge's edits undone: a file jpeg_oracle.parse takes, with the forged file's tables and entropy-coded data"""
    if rgb:
        assert blob[2:2 + len(ADOBE_RGB)] == ADOBE_RGB
        blob = blob[:2] + JFIF + blob[2 + len(ADOBE_RGB):]
    if layout in FACTORS:
        (h, w), sub = source_shape(layout, H, W)
        blob = relabel(blob, luma=0x21 if sub == 1 else 0x22, width=w, height=h)
    return blob


def source_shape(layout, H, W):
    """The shape (h, w) and Pillow's `subsampling` of the file that relabels to an H x W file of `layout`"""
    if layout == "1x2":
        return (W, H), 1
    if layout == "4x1":
        return (2 * H, -(-W // 2)), 2
    if layout == "1x4":
        return (-(-H // 2), 2 * W), 2
    raise ValueError(layout)


def forge(layout, H, W, rng, noise=False, rgb=False, **kw):
    """-> (a valid H x W file of `layout` ("1x2", "4x1", "1x4"; or "1x1", "2x1", "2x2": a Pillow file as it is), the Pillow file
    it came from); rgb: RGB-coded as well; kw: Pillow's encoder arguments (quality, progressive, restart_marker_blocks, ...)"""
    kw = dict(dict(quality=85), **kw)
    if layout in FACTORS:
        (h, w), sub = source_shape(layout, H, W)
        if kw.get("progressive") and layout != "1x2":
            assert h % 16 == 0 and w % 16 == 0 and (H, W) == ((h // 2, 2 * w) if layout == "4x1" else (2 * h, w // 2)), \
                "the non-interleaved scans' block counts would not agree"
    else:
        (h, w), sub = (H, W), {"1x1": 0, "2x1": 1, "2x2": 2}[layout]
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if noise else smooth(rng, h, w)
    src = encode(a, subsampling=sub, **kw)
    out = src
    if layout in FACTORS:
        hs, vs = FACTORS[layout]
        out = relabel(src, luma=hs << 4 | vs, width=W, height=H)
    if rgb:
        out = rgb_coded(out)
    return out, src


# ---- the restatement

def _h1v2_fancy(p, dh):
    """jdsample.c h1v2_fancy_upsample with jdmainct.c's context rows, on the chroma rows p[:dh] -> [2 dh][columns]"""
    p = p[:dh].astype(np.int32)
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    dn = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * dh, p.shape[1]), np.int32)
    out[0::2] = (3 * p + up + 1) >> 2
    out[1::2] = (3 * p + dn + 2) >> 2
    return out


def pixels(planes, W, H, hs, vs, transform):
    """Three sample planes (luma [my vs 8][mx hs 8], chroma [my 8][mx 8]) -> uint8 [H][W][3]"""
    y = planes[0][:H, :W].astype(np.int32)
    dw, dh = -(-W // hs), -(-H // vs)
    ch = []
    for p in planes[1:]:
        if (hs, vs) == (1, 1):
            c = p.astype(np.int32)
        elif (hs, vs) == (2, 1):
            c = jpeg_oracle._h2v1_fancy(p, dw)
        elif (hs, vs) == (2, 2):
            c = jpeg_oracle._h2v2_fancy(p, dw, dh)
        elif (hs, vs) == (1, 2):
            c = _h1v2_fancy(p, dh)
        else:
            c = np.repeat(np.repeat(p.astype(np.int32), vs, axis=0), hs, axis=1)
        ch.append(c[:H, :W])
    if transform:
        return np.stack([y, ch[0], ch[1]], axis=-1).astype(np.uint8)
    cb, cr = ch[0] - 128, ch[1] - 128                     # jpeg_oracle.decode's jdcolor.c fixed-point tables
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def restate_baseline(src, layout, H, W, rgb=False):
    """The pixels of forge(layout, H, W, ...)'s baseline file, from the Pillow file `src` it came from: jpeg_oracle.parse of the
    source, its size and luma factors overwritten, jpeg_oracle._planes, the rules above"""
    info = jpeg_oracle.parse(src)
    hs, vs = FACTORS.get(layout, info["comps"][0][1:3])
    info["width"], info["height"] = W, H
    c0 = info["comps"][0]
    info["comps"] = [(c0[0], hs, vs, c0[3])] + list(info["comps"][1:])
    planes, _, _ = jpeg_oracle._planes(info)
    return pixels(planes, W, H, hs, vs, int(rgb))


def restate_progressive(blob):
    """The pixels of a progressive file of any layout parse_progressive(layouts=True) takes: tests/jpeg_progressive.py's final
    coefficients, jpeg_oracle's IDCT, the rules above"""
    p = jpeg_parse.parse_progressive(blob, layouts=True)
    assert p.ncomp == 3
    coef = jpeg_progressive.coefficients(p)
    mx, my, bpm, hv = jpeg_progressive.geometry(p)
    planes, first = [], 0
    for ci in range(3):
        h, v = (p.hs, p.vs) if ci == 0 else (1, 1)
        idx = (np.arange(mx * my)[:, None] * bpm + first + np.arange(h * v)[None, :]).reshape(-1)
        px = jpeg_oracle.idct_islow(coef[idx], p.quant[ci].astype(np.int64)).reshape(my, mx, v, h, 8, 8)
        planes.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(my * v * 8, mx * h * 8))
        first += h * v
    return pixels(planes, p.width, p.height, p.hs, p.vs, p.transform)


# ---- the fixtures both test files use. (layout, H, W, rgb, noise); the sizes of the issue

SIZES_1X2 = [(1, 1), (1, 31), (31, 1), (8, 16), (9, 17), (33, 47), (100, 75)]
SIZES_4X1 = [(h, w) for h in (8, 13) for w in (32, 33, 35, 63)]
SPECS = ([("1x2", h, w, False, False) for h, w in SIZES_1X2] + [("4x1", h, w, False, False) for h, w in SIZES_4X1] +
         [("1x4", w, h, False, False) for h, w in SIZES_4X1] +
         [("1x1", 40, 56, True, False), ("1x1", 1, 1, True, False), ("2x2", 33, 47, True, False), ("1x2", 33, 47, True, False)] +
         [("1x2", 24, 40, False, True), ("4x1", 16, 40, False, True), ("1x4", 40, 16, False, True), ("1x1", 16, 24, True, True)])
# progressive: 4x1 and 1x4 only where the scans' block counts agree
PROGRESSIVE_SPECS = ([("1x2", h, w, False, False) for h, w in SIZES_1X2] +
                     [("4x1", 8, 32, False, False), ("4x1", 16, 96, False, False), ("4x1", 32, 64, False, False)] +
                     [("1x4", 32, 8, False, False), ("1x4", 96, 16, False, False), ("1x4", 64, 32, False, False)] +
                     [("1x1", 40, 56, True, False), ("1x1", 1, 1, True, False), ("2x2", 33, 47, True, False), ("1x2", 33, 47, True, False)] +
                     [("1x2", 24, 40, False, True), ("4x1", 16, 64, False, True), ("1x4", 64, 16, False, True), ("1x1", 16, 24, True, True)])


class Fixture:
    __slots__ = ("name", "layout", "H", "W", "rgb", "blob", "src", "progressive")

    def hs_vs(self):
        return FACTORS.get(self.layout) or {"1x1": (1, 1), "2x1": (2, 1), "2x2": (2, 2)}[self.layout]

    def restate(self):
        return restate_progressive(self.blob) if self.progressive else restate_baseline(self.src, self.layout, self.H, self.W, self.rgb)


def fixtures(form="baseline", seed=71):
    """The files of one decode form: "baseline", "restart" (restart intervals of 3 MCUs) or "progressive" -> [Fixture]"""
    rng = np.random.default_rng(seed)
    kw = {"baseline": {}, "restart": dict(restart_marker_blocks=3), "progressive": dict(progressive=True)}[form]
    out = []
    for k, (layout, H, W, rgb, noise) in enumerate(PROGRESSIVE_SPECS if form == "progressive" else SPECS):
        f = Fixture()
        f.layout, f.H, f.W, f.rgb, f.progressive = layout, H, W, rgb, form == "progressive"
        f.name = f"{form} {layout}{' rgb' if rgb else ''}{' noise' if noise else ''} {H}x{W}"
        f.blob, f.src = forge(layout, H, W, rng, noise=noise, rgb=rgb, quality=(92, 75, 50)[k % 3], optimize=bool(k % 4 == 1), **kw)
        out.append(f)
    return out
