"""Four-component JPEG files (CMYK as stored, YCCK) for the tests of `jpeg_parse.parse(cmyk=True)` and the device path behind it:
Pillow-written files, the forms Pillow does not write forged from them, and a numpy restatement of the pixel rules.

Pillow's encoder, for `Image.fromarray(a, "CMYK").save(..., "JPEG", subsampling=s)`, writes one interleaved scan of four components
with ids C, M, Y, K, component 0 sampled 1x1 / 2x1 / 2x2 for s = 0 / 1 / 2 and the others 1x1, an Adobe marker with transform 0, one
quantisation table and one Huffman table pair for all four. The other forms:

  as_ycck(blob)        the Adobe segment's transform byte set to 2: libjpeg then converts (p0, p1, p2) as YCbCr
  without_adobe(blob)  the Adobe segment cut out: CMYK as stored, the same pixels as transform 0
  two_quant(a, ..)     saved with qtables=[q1, q2] (both DQT tables are written) and the frame header's table selector of
                       components 1 and 2 set to 1
  two_huffman(blob)    of an optimize=True file: every DHT table copied under id 1 with one unused symbol appended at code length
                       16, the scan header's selectors of components 1 and 2 set to 0x11. (With the Annex K tables the AC table has
                       no room for another code.)

The pixel rules (checked against Pillow in tests/test_jpeg_cmyk.py). Pillow reads libjpeg's CMYK output with rawmode CMYK;I, every
byte inverted, whatever the markers say. With p0..p3 the decoded, upsampled sample planes:
  CMYK as stored   (255 - p0, 255 - p1, 255 - p2, 255 - p3)
  YCCK             (R, G, B, 255 - p3), R G B libjpeg's fixed-point YCbCr -> RGB of (p0, p1, p2)
and `convert("RGB")` of a CMYK pixel is nk = 255 - K, out_c = clip8(nk - muldiv255(c, nk)), muldiv255(a, b): t = a b + 128,
((t >> 8) + t) >> 8.
"""
import io

import numpy as np
from PIL import Image

from jpeg_layouts import encode, pillow, relabel, smooth  # noqa: F401 (pillow, relabel: for the tests that import this module)

CMYK, YCCK = 2, 3                                          # jpeg_parse's transform values
FACTORS = {0: (1, 1), 1: (2, 1), 2: (2, 2)}                # Pillow's `subsampling` -> component 0's sampling factors


def smooth4(rng, h, w):
    """A smooth [h, w, 4] picture: jpeg_layouts.smooth and a fourth band"""
    yy, xx = np.mgrid[0:h, 0:w]
    k = np.clip(90 + 80 * np.sin(xx / 11.0 - yy / 5.0) + rng.normal(0, 10, (h, w)), 0, 255).astype(np.uint8)
    return np.concatenate([smooth(rng, h, w), k[..., None]], axis=-1)


def cmyk_file(a, **kw):
    """Pillow's encoder on an [H, W, 4] array taken as mode CMYK"""
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a), "CMYK").save(buf, format="JPEG", **dict(dict(quality=85), **kw))
    return buf.getvalue()


def pillow4(blob):
    """np.asarray(Image.open(f)) of a four-component file: [H, W, 4], mode CMYK"""
    im = Image.open(io.BytesIO(blob))
    assert im.mode == "CMYK"
    return np.asarray(im)


def _segments(blob):
    """(marker, offset of its 0xFF, length of the whole segment) of every segment in front of the scan data, SOS included"""
    i, out = 2, []
    while True:
        assert blob[i] == 0xFF, "marker expected"
        m, n = blob[i + 1], 2 + ((blob[i + 2] << 8) | blob[i + 3])
        out.append((m, i, n))
        if m == 0xDA:
            return out
        i += n


def _adobe(blob):
    for m, i, n in _segments(blob):
        if m == 0xEE and blob[i + 4:i + 9] == b"Adobe":
            return i, n
    raise AssertionError("no Adobe segment")


def with_adobe_transform(blob, tf):
    i, _ = _adobe(blob)
    b = bytearray(blob)
    b[i + 15] = tf
    return bytes(b)


def as_ycck(blob):
    return with_adobe_transform(blob, 2)


def without_adobe(blob):
    i, n = _adobe(blob)
    return blob[:i] + blob[i + n:]


def _qtable(base, quality):
    """A table that grows along both axes from `base`, scaled by `quality` as libjpeg's jpeg_quality_scaling does"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [max(1, min(255, ((base + (k % 8) + 2 * (k // 8)) * scale + 50) // 100)) for k in range(64)]


def two_quant(a, **kw):
    """A file of `a` with two quantisation tables: component 0 uses table 0, components 1 and 2 are set to table 1 (where Pillow
    itself names table 1 for components 1-3 the edit changes nothing; the selectors are pinned either way)"""
    quality = kw.pop("quality", 85)
    blob = cmyk_file(a, qtables=[_qtable(12, quality), _qtable(17, quality)], **kw)
    sof = next(i for m, i, _ in _segments(blob) if m in (0xC0, 0xC1))
    b = bytearray(blob)
    assert b[sof + 9] == 4
    b[sof + 12 + 3 * 1] = b[sof + 12 + 3 * 2] = 1
    return bytes(b)


def two_huffman(blob):
    """An optimize=True file with a second pair of Huffman tables (the first pair's codes + one unused symbol of 16 bits) that
    components 1 and 2 decode with: the same pixels"""
    segs = _segments(blob)
    extra = b""
    for m, i, n in segs:
        if m != 0xC4:
            continue
        k = i + 4
        while k < i + n:
            counts = bytearray(blob[k + 1:k + 17])
            cnt = sum(counts)
            syms = bytearray(blob[k + 17:k + 17 + cnt])
            assert blob[k] & 15 == 0
            unused = next(s for s in (range(16) if blob[k] >> 4 == 0 else range(1, 256)) if s not in syms)
            code = 0
            for n_l in counts:
                code = (code + n_l) << 1
            assert code >> 1 < 0xFFFF, "no room for another 16-bit code: the file's table is full (take a smaller picture)"
            counts[15] += 1
            extra += bytes([blob[k] | 1]) + bytes(counts) + bytes(syms) + bytes([unused])
            k += 17 + cnt
    sos = segs[-1][1]
    b = bytearray(blob)
    assert b[sos + 4] == 4
    b[sos + 6 + 2 * 1] = b[sos + 6 + 2 * 2] = 0x11
    dht = b"\xff\xc4" + (2 + len(extra)).to_bytes(2, "big") + extra
    return bytes(b[:sos]) + dht + bytes(b[sos:])


def like_ijg_ycck(blob):
    """A 2x2 Pillow file relabelled to IJG's own YCCK default, 2x2,1x1,1x1,2x2 (its data no longer fits: for the parser only)"""
    return relabel(blob, luma=0x22, comp=3)


# ---- the restatement

def planes_to_cmyk(p, transform):
    """Four upsampled sample planes [4][H][W] -> Pillow's mode-CMYK bytes [H][W][4]"""
    p = np.asarray(p).astype(np.int32)
    if transform == CMYK:
        return (255 - np.stack(list(p), axis=-1)).astype(np.uint8)
    assert transform == YCCK
    y, cb, cr = p[0], p[1] - 128, p[2] - 128              # jdcolor.c's fixed-point tables, as jpeg_layouts.pixels
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b, 255 - p[3]], axis=-1), 0, 255).astype(np.uint8)


def muldiv255(a, b):
    t = a * b + 128
    return ((t >> 8) + t) >> 8


def cmyk2rgb(px):
    """Pillow's convert("RGB") of mode-CMYK bytes [..., 4] -> [..., 3]"""
    px = np.asarray(px).astype(np.int32)
    nk = 255 - px[..., 3:4]
    return np.clip(nk - muldiv255(px[..., :3], nk), 0, 255).astype(np.uint8)


# ---- the files both test files use

FORMS = ("cmyk", "ycck", "no_adobe", "restart", "optimize", "two_quant", "two_huffman")
SIZES = [(1, 1), (8, 8), (17, 33), (45, 37)]              # (H, W); the first two for 1x1 sampling only (2x is refused below width 5)


def form_file(a, sub, form, quality=85):
    """The file of picture `a` at Pillow's subsampling `sub` in one of FORMS -> (blob, transform)"""
    if form == "two_quant":
        return two_quant(a, subsampling=sub, quality=quality), CMYK
    kw = dict(restart_marker_blocks=3) if form == "restart" else dict(optimize=True) if form in ("optimize", "two_huffman") else {}
    blob = cmyk_file(a, subsampling=sub, quality=quality, **kw)
    if form == "ycck":
        return as_ycck(blob), YCCK
    if form == "no_adobe":
        return without_adobe(blob), CMYK
    if form == "two_huffman":
        return two_huffman(blob), CMYK
    return blob, CMYK


def cases(seed=83):
    """Every (sampling, size, form) of the CPU tests -> [(name, blob, (hs, vs), transform, H, W)]"""
    rng = np.random.default_rng(seed)
    out = []
    for sub in (0, 1, 2):
        for H, W in SIZES if sub == 0 else SIZES[2:]:
            a = smooth4(rng, H, W)
            for form in FORMS:
                blob, tf = form_file(a, sub, form)
                out.append((f"{form} sub{sub} {H}x{W}", blob, FACTORS[sub], tf, H, W))
    return out
