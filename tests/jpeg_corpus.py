"""A seeded corpus of malformed baseline JPEG files for the device decoder's contract (tests/test_jpeg.py on the host parser,
tests/test_jpeg_gpu.py on the device): every file is built at test time from small Pillow encodes, nothing is committed.

The rule both suites check: a file the host parser (clipmi.jpeg_parse.parse) lets through, Pillow must decode; a file the
device then decodes (status 0) must give exactly Pillow's pixels. Anything else goes back to Pillow, which decides.

Families (`family` of every item):
  a:<segment>   one byte from offset 2 to the end of the SOS header replaced by b ^ 1, b ^ 0x80, 0, 0xFF or b + 1
  b:<kind>      damage to the entropy-coded data: bit and byte flips, truncations with and without EOI, a marker inserted
                inside the scan, RSTn markers out of turn, missing or duplicated
  c:<kind>      forged headers: Huffman tables whose canonical codes overflow, sampling factors 0 and 5, a quantisation step
                of 0, a second SOI, frames above Pillow's decompression-bomb limit
"""
import io
import warnings

import numpy as np
from PIL import Image

REPLACEMENTS = (("xor1", lambda b: b ^ 1), ("xor80", lambda b: b ^ 0x80), ("zero", lambda b: 0), ("ff", lambda b: 0xFF),
                ("inc", lambda b: (b + 1) & 0xFF))


def _image(rng, h, w, grey=False, noise=False):
    if noise:
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([127 + 100 * np.sin(xx / 5.0 + yy / 9.0), 127 + 90 * np.cos(xx / 7.0 - yy / 4.0), (xx * 7 + yy * 5) % 256], -1)
        a = np.clip(a + rng.normal(0, 10, (h, w, 3)), 0, 255).astype(np.uint8)
    return a[..., 0] if grey else a


def _encode(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def base_files():
    """[(name, file bytes)]: every sampling, grey, optimised tables, restart intervals of a few blocks and of one row, noise."""
    rng = np.random.default_rng(31)
    specs = [("s0", 16, 24, {}, dict(quality=75, subsampling=0)),
             ("s1", 24, 32, {}, dict(quality=85, subsampling=1)),
             ("s2", 32, 40, {}, dict(quality=60, subsampling=2)),
             ("grey", 24, 24, dict(grey=True), dict(quality=80)),
             ("s2_opt", 32, 32, {}, dict(quality=90, subsampling=2, optimize=True)),
             ("grey_opt", 20, 28, dict(grey=True), dict(quality=50, optimize=True)),
             ("s2_rst2", 32, 48, {}, dict(quality=80, subsampling=2, restart_marker_blocks=2)),
             ("s0_rstrow", 24, 40, {}, dict(quality=88, subsampling=0, restart_marker_rows=1)),
             ("grey_rst3", 24, 32, dict(grey=True), dict(quality=70, restart_marker_blocks=3)),
             ("s0_noise", 16, 16, dict(noise=True), dict(quality=95, subsampling=0))]
    return [(name, _encode(_image(rng, h, w, **ik), **kw)) for name, h, w, ik, kw in specs]


def segments(blob):
    """[(marker byte, start, end)] of the segments from offset 2 to the end of the SOS header (start: the 0xFF)"""
    out, i = [], 2
    while True:
        m = blob[i + 1]
        L = (blob[i + 2] << 8) | blob[i + 3]
        out.append((m, i, i + 2 + L))
        i += 2 + L
        if m == 0xDA:
            return out


_NAMES = {0xC0: "SOF", 0xC4: "DHT", 0xDA: "SOS", 0xDB: "DQT", 0xDD: "DRI", 0xE0: "APP0"}


def header_mutations(bases):
    """Family (a): [(family, base name, bytes)], one replaced byte each (replacements that leave the byte as it is skipped)."""
    out = []
    for name, blob in bases:
        for m, s, e in segments(blob):
            seg = _NAMES.get(m, f"{m:02X}")
            for k in range(s, e):
                where = "marker" if k < s + 4 else "body"
                for _, f in REPLACEMENTS:
                    v = f(blob[k])
                    if v != blob[k]:
                        out.append((f"a:{seg}:{where}", name, blob[:k] + bytes([v]) + blob[k + 1:]))
    return out


def _scan(blob):
    return segments(blob)[-1][2], len(blob) - 2            # the entropy-coded data: behind the SOS header, in front of the EOI


def entropy_damage(bases, seed=41):
    """Family (b)."""
    rng = np.random.default_rng(seed)
    out = []
    for name, blob in bases:
        s, e = _scan(blob)
        for _ in range(36):                                  # single-bit flips
            k = int(rng.integers(s, e))
            out.append(("b:bitflip", name, blob[:k] + bytes([blob[k] ^ (1 << int(rng.integers(0, 8)))]) + blob[k + 1:]))
        for _ in range(16):                                  # single-byte replacements
            k = int(rng.integers(s, e))
            v = int(rng.integers(0, 256))
            if v != blob[k]:
                out.append(("b:byte", name, blob[:k] + bytes([v]) + blob[k + 1:]))
        for _ in range(5):                                   # truncations
            k = int(rng.integers(s, e))
            out.append(("b:truncate", name, blob[:k]))
            out.append(("b:truncate+eoi", name, blob[:k] + b"\xff\xd9"))
        for mk in (0xC4, 0xD9, 0xDA, 0xE1, 0xFE, 0xD8):         # a marker inside the scan (not between a 0xFF and its 0x00)
            k = int(rng.integers(s + 1, e))
            while blob[k - 1] == 0xFF:
                k += 1
            out.append(("b:marker", name, blob[:k] + bytes([0xFF, mk]) + blob[k:]))
        rst = [k for k in range(s, e - 1) if blob[k] == 0xFF and 0xD0 <= blob[k + 1] <= 0xD7]
        for k in rst[:4] + rst[-1:]:
            nxt = 0xD0 + ((blob[k + 1] - 0xD0 + 1) & 7)
            out.append(("b:rst_order", name, blob[:k + 1] + bytes([nxt]) + blob[k + 2:]))
            out.append(("b:rst_missing", name, blob[:k] + blob[k + 2:]))
            out.append(("b:rst_duplicate", name, blob[:k + 2] + blob[k:]))
        if len(rst) >= 2:                                    # two markers swapped
            a, b = rst[0], rst[1]
            sw = bytearray(blob)
            sw[a + 1], sw[b + 1] = blob[b + 1], blob[a + 1]
            out.append(("b:rst_swapped", name, bytes(sw)))
    return out


def _dht_tables(blob):
    """[(Tc << 4 | Th, counts[16], symbols)] of every DHT segment, and the [start, end) of all of them (Pillow writes them together)"""
    tabs, span = [], None
    for m, s, e in segments(blob):
        if m != 0xC4:
            continue
        span = (s if span is None else span[0], e)
        k = s + 4
        while k < e:
            counts = list(blob[k + 1:k + 17])
            n = sum(counts)
            tabs.append((blob[k], counts, list(blob[k + 17:k + 17 + n])))
            k += 17 + n
    return tabs, span


def _dht_bytes(tabs):
    out = b""
    for tcth, counts, syms in tabs:
        body = bytes([tcth]) + bytes(counts) + bytes(syms)
        out += b"\xff\xc4" + (2 + len(body)).to_bytes(2, "big") + body
    return out


def _overflowing(counts, syms, extra, pool):
    """counts / symbols with codes added at the table's longest length until its last code + 1 - (1 << length) == extra:
    -1 a valid table, 0 the last code all ones, 1 one code too many (libjpeg refuses 0 and 1)"""
    counts, syms = list(counts), list(syms)
    last = max(k for k in range(16) if counts[k])
    code = 0
    for k in range(last):
        code = (code + counts[k]) << 1
    add = (1 << (last + 1)) + extra - (code + counts[last])
    assert add >= 0
    counts[last] += add
    fresh = [s for s in pool if s not in syms]
    syms = syms + (fresh * (1 + add // max(1, len(fresh))))[:add]
    return counts, syms


def _set_sof(blob, fn):
    for m, s, e in segments(blob):
        if m in (0xC0, 0xC1):
            seg = bytearray(blob[s:e])
            fn(seg)
            return blob[:s] + bytes(seg) + blob[e:]
    raise AssertionError("no SOF")


def forged_headers(bases):
    """Family (c)."""
    by = dict(bases)
    out = []
    for name in ("s2", "grey", "s2_opt"):
        blob = by[name]
        tabs, (s, e) = _dht_tables(blob)
        for cls in (0, 1):
            j = next(t for t, tab in enumerate(tabs) if tab[0] >> 4 == cls)
            pool = list(range(16)) if cls == 0 else list(range(256))
            for extra, label in ((0, "all_ones"), (1, "overflow"), (5, "overflow")):
                c, sy = _overflowing(tabs[j][1], tabs[j][2], extra, pool)
                if sum(c) > 256:
                    continue
                t2 = list(tabs)
                t2[j] = (tabs[j][0], c, sy)
                out.append((f"c:dht_{'dc' if cls == 0 else 'ac'}_{label}", name, blob[:s] + _dht_bytes(t2) + blob[e:]))
            c, sy = _overflowing(tabs[j][1], tabs[j][2], -1, pool)          # the same table one code short of it: valid
            t2 = list(tabs)
            t2[j] = (tabs[j][0], c, sy)
            out.append((f"c:dht_{'dc' if cls == 0 else 'ac'}_full", name, blob[:s] + _dht_bytes(t2) + blob[e:]))
    for name in ("grey", "s0", "s2"):
        for comp in ((0,) if name == "grey" else (0, 1)):
            for hv in (0x00, 0x01, 0x10, 0x51, 0x15, 0x55, 0x05):
                def f(seg, comp=comp, hv=hv):
                    seg[11 + 3 * comp] = hv
                out.append((f"c:sampling_{hv:02x}", name, _set_sof(by[name], f)))
    for name in ("s1", "grey"):
        for m, s, e in segments(by[name]):
            if m == 0xDB:
                for k in (0, 1, 17, 63):                     # (zigzag positions; the first table of the segment)
                    out.append(("c:dqt_zero", name, by[name][:s + 5 + k] + b"\0" + by[name][s + 6 + k:]))
                break
    for name in ("s0", "grey"):
        sof = next(s for m, s, e in segments(by[name]) if m == 0xC0)
        out.append(("c:second_soi", name, by[name][:sof] + b"\xff\xd8" + by[name][sof:]))
        out.append(("c:second_soi_first", name, by[name][:2] + b"\xff\xd8" + by[name][2:]))
    for name, (h, w) in (("s0", (20000, 20000)), ("grey", (20000, 20000)), ("s2", (65535, 65535)), ("s2", (1, 65504)),
                         ("s0", (65500, 1)), ("grey", (9000, 9000)), ("s0", (10000, 17896))):
        def f(seg, h=h, w=w):
            seg[5:9] = bytes([h >> 8, h & 255, w >> 8, w & 255])
        out.append((f"c:size_{w}x{h}", name, _set_sof(by[name], f)))
    return out


def corpus():
    bases = base_files()
    return header_mutations(bases) + entropy_damage(bases) + forged_headers(bases)


def pillow(blob):
    """Image.open(...).convert("RGB") as a uint8 array, None where Pillow raises (the reference skips such a file)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))
        except Exception:
            return None
