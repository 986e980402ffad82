"""A baseline JPEG writer for the tests: files Pillow's encoder never writes, from the coefficients of files it does.

write(blob, **options): a Pillow baseline file's quantised coefficients (jpeg_oracle.parse + decode_coefficients) written
again as one interleaved sequential scan, DC differenced anew per component and restart interval, every header byte written
here. The options choose what real encoders vary and Pillow's does not: the SHAPE of the Huffman tables (`tables`: named
length profiles, symbols assigned shortest-first by their frequency in the data), the table ids, the quantisation table ids,
SOF0 / SOF1, any restart interval, and the header layout. With the coefficients and steps unchanged Pillow decodes the result
to exactly the base file's pixels, which pins the writer without trusting any decoder of ours (tests/test_jpeg_baseline.py).
`coef` and `quant` rewrite the coefficients and the steps (synthetic blocks: long blocks, categories 11-15), `tamper` the
symbol events (runs past coefficient 63); Pillow live is the reference for those.

covered(bits) restates csrc/jpeg.hip jpeg_build_luts_kernel's predicate: a table whose every code longer than JP_FAST bits
sits under the last JP_LONG 10-bit prefixes is decoded by two look-ups, any other by jp_lookup's bit-by-bit walk.
"""
import io

import numpy as np
from PIL import Image

from oracle import jpeg_oracle
from jpeg_progressive import _bytes, _codes, _nbits, _seg, optimal_table

JP_FAST, JP_LONG = 10, 8
FIRST_LONG_PREFIX = (1 << JP_FAST) - JP_LONG                # 1016

# ITU T.81 Annex K.3: the luminance tables' counts per code length (K.3 DC, K.5 AC) and the AC symbols
ANNEXK_DC_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
ANNEXK_AC_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
ANNEXK_AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]           # 162
PROFILES = ("annexk", "optimal", "flat16", "flat11", "edge_covered", "edge_uncovered", "second_full")
# what each profile is meant to be, per table class; None: depends on the data (`optimal`)
NAMED_COVERED = {"annexk": True, "optimal": None, "flat16": False, "flat11": False, "edge_covered": True, "edge_uncovered": False,
                 "second_full": True}


def covered(bits):
    """The 16 counts of a DHT -> whether the device decodes the table without the bit-by-bit walk (JpLut.covered)"""
    code, cov = 0, True
    for l in range(1, 17):
        n = bits[l - 1]
        if n and l > JP_FAST and (code >> (l - JP_FAST)) < FIRST_LONG_PREFIX:
            cov = False
        code = (code + n) << 1
    return cov


def long_prefixes(bits, vals, used):
    """The 10-bit prefixes under which the codes longer than 10 bits of the symbols in `used` sit"""
    return sorted({c >> (l - JP_FAST) for s, (c, l) in _codes(bits, vals).items() if l > JP_FAST and s in used})


def _expand(bits):
    return [l + 1 for l, n in enumerate(bits) for _ in range(n)]


def _split_to(lengths, m, cap):
    """Ascending code lengths with the same Kraft sum and m codes: the shortest code below `cap` bits split in two"""
    lengths = sorted(lengths)
    while len(lengths) < m:
        k = next(i for i, l in enumerate(lengths) if l < cap)
        lengths[k:k + 1] = [lengths[k] + 1] * 2
        lengths.sort()
    return lengths


def profile_lengths(name, cls, n):
    """Ascending code lengths of the n symbols of a table of class cls (0 DC, 1 AC) under the named profile. AC tables take
    the shapes as named; DC tables hold 12-16 symbols, so their edge profiles reach the same prefixes with fewer short codes:
    lengths 1-7 end at prefix 1016 (covered), lengths 1-6, 8, 9, 10 at prefix 1015 (uncovered)."""
    if name == "annexk":
        ls = _expand(ANNEXK_AC_BITS) if cls else _expand(ANNEXK_DC_BITS) + [10, 11, 12, 13]
    elif name == "flat16":
        ls = [16] * n
    elif name == "flat11":
        ls = [11] * n
    elif name == "edge_covered":
        short = [1, 2, 3, 4, 5, 6] + [10] * 8 if cls else [1, 2, 3, 4, 5, 6, 7]
        ls = short + [16] * max(0, n - len(short))
    elif name == "edge_uncovered":
        short = [1, 2, 3, 4, 5, 6] + [10] * 7 if cls else [1, 2, 3, 4, 5, 6, 8, 9, 10]
        ls = short + [16] * max(0, n - len(short))
    elif name == "second_full":
        if cls:
            # 11-bit codes under prefixes 1016-1021, 12-bit under 1022, 13-, 14-, 15- and 16-bit under 1023: the fewest codes
            # (30 with the 14 short ones) that put a long code under every one of the eight
            long_ = [11] * 12 + [12] * 4 + [13] * 2 + [14] * 2 + [15] * 2 + [16] * 35
            ls = _split_to([1, 2, 3, 4, 5, 6] + [10] * 8, max(14, n - len(long_)), JP_FAST) + long_
        else:
            ls = [1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 14, 15] + [16] * max(0, n - 12)
    else:
        raise ValueError(name)
    assert len(ls) >= n, (name, cls, n)
    return ls[:n]


def check_canonical(bits):
    """jdhuff.c jpeg_make_d_derived_tbl's condition: no code of length l reaches 1 << l (all ones)"""
    code = 0
    for l in range(1, 17):
        code += bits[l - 1]
        assert code < 1 << l, bits
        code <<= 1


def profile_table(name, cls, freq):
    """symbol -> count in the data  ->  (bits[16], vals) of the named profile. The data's symbols come first, by falling
    frequency; DC tables are filled up to the 12 categories every encoder lists, the Annex K AC table to its 162 symbols
    (an unused standard symbol makes room where the data holds symbols Annex K does not: categories 11-15)."""
    used = sorted((s for s, f in freq.items() if f), key=lambda s: (-freq[s], s))
    if name == "optimal":
        bits, vals = optimal_table(freq)
    else:
        syms = list(used)
        if cls == 0:
            syms += [s for s in range(12) if s not in freq]
        elif name == "annexk":
            syms = (syms + [s for s in ANNEXK_AC_SYMBOLS if s not in freq])[:max(162, len(used))]
        elif len(syms) < 32:                                 # a smooth picture's few AC symbols: the shape needs its long codes
            syms = (syms + [s for s in ANNEXK_AC_SYMBOLS if s not in freq])[:32]
        ls = profile_lengths(name, cls, len(syms))
        bits, vals = [ls.count(l) for l in range(1, 17)], syms
    check_canonical(bits)
    assert len(vals) == sum(bits) and set(used) <= set(vals)
    return bits, vals


def events(coef, order, ri, ids):
    """-> per restart interval the list of events ('h', (class, table id), symbol) | ('b', value, nbits) of jchuff.c's
    encode_one_block, blocks in MCU order, DC predictions fresh in every interval"""
    nat = jpeg_oracle.NATURAL
    bpm = len(order)
    nm = len(coef) // bpm
    out, ev, pred = [], None, None
    for m in range(nm):
        if m % (ri or nm) == 0:
            ev, pred = [], [0, 0, 0]
            out.append(ev)
        for k, c in enumerate(order):
            zz = coef[m * bpm + k][nat].tolist()
            d, pred[c] = zz[0] - pred[c], zz[0]
            s = _nbits(abs(d))
            assert s <= 15
            ev.append(("h", (0, ids[c][0]), s))
            if s:
                ev.append(("b", (d if d >= 0 else d - 1) & ((1 << s) - 1), s))
            r, key = 0, (1, ids[c][1])
            for v in zz[1:]:
                if v == 0:
                    r += 1
                    continue
                while r > 15:
                    ev.append(("h", key, 0xF0))
                    r -= 16
                s = _nbits(abs(v))
                assert s <= 15
                ev.append(("h", key, (r << 4) | s))
                ev.append(("b", (v if v >= 0 else v - 1) & ((1 << s) - 1), s))
                r = 0
            if r:
                ev.append(("h", key, 0))
    return out


def block_bits(ev, codes):
    """Bits of every block of an interval's events (a block starts at its DC symbol)"""
    out = []
    for e in ev:
        if e[0] == "h":
            if e[1][0] == 0:
                out.append(0)
            out[-1] += codes[e[1]][e[2]][1]
        else:
            out[-1] += e[2]
    return out


LAYOUTS = ("merged", "extra_table", "redefined", "dri_before_sof", "fill", "com", "app1_thumb", "ids_123", "ids_012", "ids_YCc",
           "ids_RGB", "adobe", "adobe_tf0", "trailing")
_IDS = {"ids_123": (1, 2, 3), "ids_012": (0, 1, 2), "ids_YCc": (0x59, 0x43, 0x63), "ids_RGB": (0x52, 0x47, 0x42)}


def _thumbnail():
    buf = io.BytesIO()
    Image.fromarray(np.arange(16 * 16 * 3, dtype=np.uint8).reshape(16, 16, 3)).save(buf, format="JPEG", quality=50)
    return buf.getvalue()


def write(blob, tables="annexk", table_ids=None, quant_ids=None, sof=0xC0, ri=0, layout=(), coef=None, quant=None, tamper=None,
          report=None):
    """Baseline JPEG file -> a baseline file of the same (or rewritten) coefficients.
    tables     a profile name, or {"dc": name, "ac": name}
    table_ids  per component (DC id, AC id); default (0,0),(1,1),(1,1) as Pillow
    quant_ids  per component the id its quantisation table is written under (the steps stay the component's own)
    sof        0xC0 or 0xC1
    ri         restart interval in MCUs (0: no DRI)
    layout     names out of LAYOUTS
    coef       callable(int32 [blocks][64] natural order, DC absolute; component of every block) -> the array to encode
    quant      {component index: 64 steps in zigzag order} replacing the base file's
    tamper     callable(interval index, events) -> events, before the tables are built (every code stays valid)
    report     dict filled with what was written: tables {(class, id): (bits, vals)}, used {(class, id): symbols}, block_bits"""
    layout = (layout,) if isinstance(layout, str) else tuple(layout)
    assert all(x in LAYOUTS for x in layout), layout
    info = jpeg_oracle.parse(blob)
    c0, (mx, my, hmax, vmax, order) = jpeg_oracle.decode_coefficients(info)
    comps = info["comps"]
    nc = len(comps)
    c0 = c0.astype(np.int32)
    if coef is not None:
        c0 = np.asarray(coef(c0.copy(), np.tile(order, mx * my)), np.int32)
    ids = list(table_ids) if table_ids is not None else [(0, 0), (1, 1), (1, 1)][:nc]
    prof = tables if isinstance(tables, dict) else {"dc": tables, "ac": tables}
    evs = events(c0, order, ri, ids)
    if tamper is not None:
        evs = [tamper(k, ev) for k, ev in enumerate(evs)]
    freq = {}
    for ev in evs:
        for e in ev:
            if e[0] == "h":
                f = freq.setdefault(e[1], {})
                f[e[2]] = f.get(e[2], 0) + 1
    huff = {key: profile_table(prof["ac" if key[0] else "dc"], key[0], f) for key, f in sorted(freq.items())}
    codes = {key: _codes(*t) for key, t in huff.items()}
    if report is not None:
        report.update(tables=huff, used={k: set(f) for k, f in freq.items()}, block_bits=[b for ev in evs for b in block_bits(ev, codes)])

    fill = b"\xff\xff\xff" if "fill" in layout else b""

    def seg(m, payload):
        return fill + _seg(m, payload)

    def dht(items):
        return [bytes([(cls << 4) | tid]) + bytes(bits) + bytes(vals) for (cls, tid), (bits, vals) in items]

    qids = list(quant_ids) if quant_ids is not None else [c[3] for c in comps]
    qt = {}
    for ci, c in enumerate(comps):
        steps = list(quant[ci]) if quant is not None and ci in quant else info["qt"][c[3]]
        assert qt.setdefault(qids[ci], steps) == steps, "two components with different steps under one id"
    cids = next((_IDS[x] for x in layout if x in _IDS), tuple(c[0] for c in comps))[:nc]
    jfif = not any(x in _IDS or x.startswith("adobe") for x in layout)

    out = bytearray(b"\xff\xd8")
    if jfif:
        out += seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    if "adobe" in layout or "adobe_tf0" in layout:
        out += seg(0xEE, b"Adobe\0\x64\0\0\0\0" + bytes([1 if "adobe" in layout else 0]))
    if "com" in layout:
        out += seg(0xFE, b"written by tests/jpeg_baseline.py \xff\xd8\xff\xd9")
    if "app1_thumb" in layout:
        body = b"Exif\0\0II*\0\x08\0\0\0\0\0\0\0\0\0" + _thumbnail()
        out += seg(0xE1, body.ljust(65533, b"\0"))
    dqt = [bytes([tq]) + bytes(steps) for tq, steps in sorted(qt.items())]
    if "redefined" in layout:                                # a first definition that must not be used: the steps reversed
        dqt = [bytes([tq]) + bytes(steps[::-1]) for tq, steps in sorted(qt.items())] + dqt
    if "extra_table" in layout:
        dqt += [bytes([tq]) + bytes(range(1, 65)) for tq in range(4) if tq not in qt][:1]
    for d in ([b"".join(dqt)] if "merged" in layout else dqt):
        out += seg(0xDB, d)
    dri = seg(0xDD, ri.to_bytes(2, "big")) if ri else b""
    if "dri_before_sof" in layout:
        out += dri
    frame = bytes([8]) + info["height"].to_bytes(2, "big") + info["width"].to_bytes(2, "big") + bytes([nc])
    for ci, c in enumerate(comps):
        frame += bytes([cids[ci], (c[1] << 4) | c[2], qids[ci]])
    out += seg(sof, frame)
    if "dri_before_sof" not in layout:
        out += dri
    tabs = dht(sorted(huff.items()))
    if "redefined" in layout:                                # the same ids first with another valid table: the last one counts
        tabs = dht([(k, profile_table("flat11" if covered(t[0]) else "annexk", k[0], freq[k])) for k, t in sorted(huff.items())]) + tabs
    if "extra_table" in layout:
        spare = [(cls, tid) for cls in (0, 1) for tid in range(4) if (cls, tid) not in huff][:2]
        tabs += dht([(k, profile_table("annexk", k[0], {0: 1})) for k in spare])
    for d in ([b"".join(tabs)] if "merged" in layout else tabs):
        out += seg(0xC4, d)
    sos = bytes([nc])
    for ci in range(nc):
        sos += bytes([cids[ci], (ids[ci][0] << 4) | ids[ci][1]])
    out += seg(0xDA, sos + b"\x00\x3f\x00")
    for k, ev in enumerate(evs):
        if k:
            out += fill + bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        out += _bytes(ev, codes)
    out += fill + b"\xff\xd9"
    if "trailing" in layout:
        out += b"trailing bytes \xff\xd8 behind the end of the image"
    return bytes(out)


# ---- synthetic blocks and symbol rewrites

def ones(n=3):
    """quant= argument: a step of 1 everywhere, for n components"""
    return {c: [1] * 64 for c in range(n)}


def long_blocks(category, seed=0):
    """coef= callable: every block gets 63 non-zero AC coefficients of the category and a small DC. The signs are searched so
    that the block's IDCT (at a step of 1) stays inside the device's range where the category allows it (jpeg_oracle.idct_islow
    raises Reported outside): the pixels then come back and can be compared."""
    rng = np.random.default_rng(seed)
    lo = 1 << (category - 1)
    pats = []
    for _ in range(4000):
        b = np.zeros((1, 64), np.int64)
        b[0, 1:] = rng.integers(lo, lo + max(1, lo // 16), 63) * rng.choice([-1, 1], 63)
        try:
            for dc in (-40, 40):                             # (the blocks' DC values stay within +-32)
                b[0, 0] = dc
                jpeg_oracle.idct_islow(b, np.ones(64, np.int64))
            pats.append(b[0])
        except jpeg_oracle.Reported:
            if category >= 10 and not pats:                  # no sign pattern fits (Parseval): any pattern will do
                pats.append(b[0])
        if len(pats) == 4:
            break
    assert pats, "no block of 63 coefficients of this category stays in the IDCT's range"

    def f(c, comp):
        for k in range(len(c)):
            c[k] = pats[k % len(pats)]
            c[k, 0] = (k * 37) % 64 - 32
        return c
    return f


def one_coefficient(block, index, value, dc=0):
    """coef= callable: everything flat (DC `dc`, no AC) but natural-order coefficient `index` of block `block`"""
    def f(c, comp):
        c[:] = 0
        c[:, 0] = dc
        c[block, index] = value
        return c
    return f


def dc_steps(values):
    """coef= callable: flat blocks whose luma DC values walk through `values` (the differences are the symbols), chroma 0"""
    def f(c, comp):
        c[:] = 0
        luma = np.flatnonzero(comp == 0)
        c[luma, 0] = [values[k % len(values)] for k in range(len(luma))]
        return c
    return f


def run_overrun(k, ev):
    """tamper= callable: the first block of interval 0 that has an AC coefficient keeps its DC symbol and becomes three ZRL
    symbols and (15, s) with the value bits of its first coefficient - the index reaches 1 + 48 + 15 = 64 - and nothing else:
    the next block's DC symbol follows, so every later symbol keeps its meaning"""
    if k:
        return ev
    for i, e in enumerate(ev):
        if e[0] == "h" and e[1][0] == 1 and e[2] & 15:
            j = next((t for t in range(i, len(ev)) if ev[t][0] == "h" and ev[t][1][0] == 0), len(ev))
            return ev[:i] + [("h", e[1], 0xF0)] * 3 + [("h", e[1], 0xF0 | (e[2] & 15)), ev[i + 1]] + ev[j:]
    return ev


def dc_walk(c, comp):
    """coef= callable: the AC coefficients stay, every component's DC values walk 0, 1, -1, 3, -3, 7, ... 511, -511, 0, 0: DC
    differences of every category from 0 to 10 whatever the picture (bases of quality >= 90: |DC x step| / 8 stays below 200)"""
    walk = [0]
    for j in range(1, 10):
        walk += [(1 << j) - 1, -((1 << j) - 1)]
    walk += [0, 0]
    for ci in range(3):
        idx = np.flatnonzero(comp == ci)
        c[idx, 0] = [walk[k % len(walk)] for k in range(len(idx))]
    return c


# ---- the corpus: built once per process (the Python writer is the slow part)

def rich(rng, h, w):
    """A picture whose blocks differ in level by powers of two and whose noise grows towards one corner: many DC categories,
    long zero runs and large coefficients in one file"""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 60 * np.sin(xx / 9.0 + yy / 17.0), 127 + 60 * np.cos(xx / 13.0 - yy / 7.0), (xx * 3 + yy * 2) % 256], -1).astype(float)
    bh, bw = -(-h // 8), -(-w // 8)
    mag = 2.0 ** rng.integers(0, 8, (bh, bw, 3)) * rng.choice([-1, 1], (bh, bw, 3))
    step = np.kron(mag, np.ones((8, 8, 1)))[:h, :w]
    sigma = (xx / w * 70)[..., None] * (yy / h)[..., None]
    return np.clip(base + step + rng.normal(0, 1, (h, w, 3)) * sigma, 0, 255).astype(np.uint8)


def _encode(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", **kw)
    return buf.getvalue()


_cache = {}


def bases():
    """name -> (baseline file by Pillow, committed Pillow pixels or None): seeded pictures of 37 x 53 and 64 x 96 in the three
    samplings and grey, and files of tests/golden/jpeg_cases.npz, whose Pillow pixels are committed beside them"""
    if "bases" not in _cache:
        import os
        rng = np.random.default_rng(2024)
        out = {}
        for (h, w), q in (((37, 53), 95), ((64, 96), 92)):
            for sub in (0, 1, 2):
                out[f"{h}x{w}_{sub}"] = (_encode(rich(rng, h, w), quality=q, subsampling=sub), None)
            out[f"{h}x{w}_grey"] = (_encode(rich(rng, h, w)[..., 0], quality=q), None)
        d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz"))
        for i in (0, 1, 2, 9, 11, 18):
            out[f"golden{i}"] = (d[f"file_{i}"].tobytes(), d[f"rgb_{i}"])
        _cache["bases"] = out
    return _cache["bases"]


ID_CASES = {"ids_pillow": ((0, 0), (1, 1), (1, 1)), "ids_distinct": ((0, 0), (1, 1), (2, 2)), "ids_3": ((3, 3), (3, 2), (2, 3)),
            "ids_shared": ((1, 1), (1, 1), (1, 1)), "ids_crossed": ((0, 3), (3, 0), (0, 0))}
WELL_FORMED_LAYOUTS = ("merged", "extra_table", "redefined", "dri_before_sof", "fill", "com", "app1_thumb", "ids_123", "ids_012",
                       "ids_YCc", "adobe", "trailing")
# Layouts the parser refuses BY DESIGN, because libjpeg (jdapimin.c default_decompress_parms) takes such a file for RGB-coded
# and the device converts YCbCr only: component ids 'R','G','B' without a JFIF or Adobe marker; Adobe transform 0.
EXPECTED_UNSUPPORTED = ("ids_RGB", "adobe_tf0")


def _mcus(blob):
    info = jpeg_oracle.parse(blob)
    hm, vm = max(c[1] for c in info["comps"]), max(c[2] for c in info["comps"])
    return -(-info["width"] // (8 * hm)), -(-info["height"] // (8 * vm))


class Case:
    """family, name, base (a name in bases(), or None), opt (write's options), blob, rep (write's report)"""

    def __init__(self, family, name, base, opt):
        self.family, self.name, self.base, self.opt, self.blob, self.rep = family, name, base, opt, None, {}

    def profile(self, cls):
        t = self.opt.get("tables", "annexk")
        return t["ac" if cls else "dc"] if isinstance(t, dict) else t


def parity_cases():
    """Well-formed files whose coefficients and steps are the base file's: Pillow decodes each to the base file's pixels.
    The EXPECTED_UNSUPPORTED layouts are in the list too (family 'unsupported')."""
    B = bases()
    grey = ("37x53_grey", "64x96_grey", "golden18")
    cases = []

    def add(fam, name, n, **opt):
        cases.append(Case(fam, f"{name}/{n}", n, opt))

    for n in B:
        for prof in PROFILES:
            add("profile", prof, n, tables=prof)
        # the two classes under different profiles
        add("profile", "dc_flat16_ac_second_full", n, tables={"dc": "flat16", "ac": "second_full"})
        add("profile", "dc_edge_uncovered_ac_annexk", n, tables={"dc": "edge_uncovered", "ac": "annexk"})
    for k, n in enumerate(("37x53_0", "37x53_1", "37x53_2", "64x96_1", "golden2", "golden9")):
        for j, (name, ids) in enumerate(ID_CASES.items()):
            add("table_ids", name, n, table_ids=ids, tables=PROFILES[(k + j) % len(PROFILES)])
        add("quant_ids", "quant_123", n, quant_ids=(1, 2, 3), tables=PROFILES[k % len(PROFILES)])
        add("quant_ids", "quant_310", n, quant_ids=(3, 1, 0), table_ids=ID_CASES["ids_distinct"])
    for n in ("37x53_grey", "golden18"):
        add("table_ids", "ids_3", n, table_ids=((3, 2),), tables="edge_uncovered")
        add("quant_ids", "quant_2", n, quant_ids=(2,))
    for k, n in enumerate(B):
        add("sof1", "sof1", n, sof=0xC1, tables=PROFILES[k % len(PROFILES)])
    for k, n in enumerate(("37x53_0", "37x53_1", "37x53_2", "37x53_grey", "64x96_2", "golden11")):
        mx, my = _mcus(B[n][0])
        nondiv = next(r for r in range(2, mx + 3) if mx % r)
        for name, ri in (("ri_1", 1), ("ri_nondivisor", nondiv), ("ri_row", mx), ("ri_all", mx * my), ("ri_more", mx * my + 3),
                         ("ri_9", 9)):
            add("ri", f"{name}={ri}", n, ri=ri, tables=PROFILES[(k + ri) % len(PROFILES)])
    for k, n in enumerate(("37x53_2", "64x96_0", "golden1", "golden18")):
        for lay in WELL_FORMED_LAYOUTS + EXPECTED_UNSUPPORTED:
            if n in grey and (lay.startswith("ids_") or lay.startswith("adobe")):
                continue
            opt = dict(layout=lay, tables=PROFILES[k % len(PROFILES)])
            if lay == "dri_before_sof":
                opt["ri"] = 3
            add("unsupported" if lay in EXPECTED_UNSUPPORTED else "layout", lay, n, **opt)
        add("layout", "fill+ri", n, layout="fill", ri=4, tables="flat11")
        add("layout", "merged+redefined+extra+com", n, layout=("merged", "redefined", "extra_table", "com"), tables="second_full")
        if n not in grey:
            add("layout", "adobe+trailing+fill", n, layout=("adobe", "trailing", "fill"), table_ids=ID_CASES["ids_3"])
    return cases


def written():
    """parity_cases(), written once"""
    if "written" not in _cache:
        B = bases()
        out = parity_cases()
        for c in out:
            c.blob = write(B[c.base][0], report=c.rep, **c.opt)
        _cache["written"] = out
    return _cache["written"]


def big_flat16():
    """A 160 x 240 4:4:4 file under flat16: every symbol through the bit-by-bit walk, in a stream of many chunks of 128
    subsequences"""
    if "big" not in _cache:
        c = Case("profile", "flat16/160x240_0", None, dict(tables="flat16"))
        c.base_blob = _encode(rich(np.random.default_rng(7), 160, 240), quality=95, subsampling=0)
        c.blob = write(c.base_blob, report=c.rep, **c.opt)
        _cache["big"] = c
    return _cache["big"]


def _zero_step(comp, zigzag_index):
    q = ones()
    q[comp] = [1] * 64
    q[comp][zigzag_index] = 0
    return q


def synthetic_cases():
    """Files whose coefficients are made here, on the 64 x 96 4:4:4 base at a step of 1 (Pillow live is the reference):
      long_blocks  every block 63 AC coefficients of category 9 under flat16: 63 x 25 bits and the DC symbol, more than a
                   subsequence of 1 024 bits; signs chosen so that the IDCT stays in the device's range. By Parseval 63
                   coefficients of category 10 (>= 512 each) need pixels of more than +-508 rms, outside [-512, 511] for every
                   choice of signs: that file is in the `extreme` family, where the device may hand it back.
      dc_walk      DC differences of every category 0-10 under every profile (DC tables see few symbols in a small picture)
      extreme      single AC coefficients and DC differences of categories 11-15, under Annex K-shaped tables extended with
                   those symbols and under flat16 (code + value bits up to 31). At a step of 1 the IDCT's range admits AC
                   values up to 511 x the basis function's 1-norm (< 4 096: categories 11 and 12) and DC differences below
                   8 192 (category 13); every category also comes with a step of 0 at that coefficient, which libjpeg reads like
                   any other: the symbol is decoded, its value does not reach the pixels.
      overrun      a run that takes the coefficient index past 63 (libjpeg stores the value at 63 and ends the block)"""
    if "synthetic" in _cache:
        return _cache["synthetic"]
    B = bases()
    base = B["64x96_0"][0]
    out = []

    def add(fam, name, blob_of=base, **opt):
        c = Case(fam, name, None, opt)
        c.blob = write(blob_of, report=c.rep, **opt)
        out.append(c)

    add("long_blocks", "cat9/flat16", coef=long_blocks(9), quant=ones(), tables="flat16")
    add("long_blocks", "cat9/dc_annexk_ac_flat16/ri_more", coef=long_blocks(9, seed=1), quant=ones(), tables={"dc": "annexk", "ac": "flat16"}, ri=100)
    add("extreme", "long_blocks_cat10/flat16", coef=long_blocks(10), quant=ones(), tables="flat16")
    for prof in PROFILES:
        add("dc_walk", prof, coef=dc_walk, tables=prof)
        add("dc_walk", prof + "/420", blob_of=B["64x96_2"][0], coef=dc_walk, tables=prof)
    dc_values = {11: [0, 1500, -200, 1400], 12: [-1500, 1500, -1400, 1300], 13: [-3900, 3900, -3800, 3700], 14: [0, 10000, -2000, 9000],
                 15: [0, 16000, -16000, 100]}
    for s in range(11, 16):
        lo = 1 << (s - 1)
        for prof in ("annexk", "flat16"):
            for sign in (1, -1):
                add("extreme", f"ac{s}/{prof}/{sign:+d}", coef=one_coefficient(40, 1, sign * (lo + lo // 3)), quant=ones(), tables=prof)
                add("extreme", f"ac{s}/{prof}/{sign:+d}/step0", coef=one_coefficient(42, 8, sign * (2 * lo - 1), dc=5), quant=_zero_step(0, 2),
                    tables=prof)
            add("extreme", f"dc{s}/{prof}", coef=dc_steps(dc_values[s]), quant=ones(), tables=prof)
            add("extreme", f"dc{s}/{prof}/step0", coef=dc_steps(dc_values[s]), quant=_zero_step(0, 0), tables=prof)
    for n in ("37x53_0", "37x53_2", "64x96_1", "37x53_grey"):
        for prof in ("annexk", "flat16", "edge_uncovered"):
            add("overrun", f"{prof}/{n}", blob_of=B[n][0], tamper=run_overrun, tables=prof)
            add("overrun", f"{prof}/{n}/ri2", blob_of=B[n][0], tamper=run_overrun, tables=prof, ri=2)
    _cache["synthetic"] = out
    return out


def progressive_cases():
    """(name, progressive file, baseline file of the same coefficients): jpeg_progressive.write's split-band script under the
    profiles whose codes are longer than the progressive look-up's 10-bit table in ways no encoder produces"""
    if "progressive" not in _cache:
        import jpeg_progressive
        out = []
        for n in ("37x53_2", "64x96_0", "37x53_grey"):
            base = bases()[n][0]
            script = jpeg_progressive.scripts(1 if n.endswith("grey") else 3)["split_bands"]
            for prof in ("flat16", "flat11", "edge_covered", "edge_uncovered"):
                out.append((f"{prof}/{n}", jpeg_progressive.write(base, script, tables=prof), base))
        _cache["progressive"] = out
    return _cache["progressive"]
