"""Progressive JPEG for the tests: a CPU restatement of the device decoder and a progressive writer.

decode(data): plain Python / numpy restatement of what `Image.open(f).convert("RGB")` computes for the progressive files
`jpeg_parse.parse_progressive` lets through (ITU T.81 Annex G, as libjpeg's jdphuff.c decodes it): the scans' entropy decode
to final coefficients, then oracle.jpeg_oracle's jpeg_idct_islow, fancy upsampling and colour conversion. It is checked against
Pillow in tests/test_jpeg_progressive.py, and it is what a device mismatch is debugged against.

write(blob, script): a baseline file's quantised coefficients (jpeg_oracle.parse + decode_coefficients) rewritten as a
progressive file with an arbitrary scan script: per-scan optimal Huffman tables limited to 16 bits, EOB runs up to 0x7FFF,
refinement correction bits buffered as jcphuff.c does. Pillow decodes the result to exactly the baseline file's pixels when the
script is complete, which pins the writer without trusting any decoder of ours. It covers scripts Pillow never writes.
"""
import heapq
import io

import numpy as np
from PIL import Image

from clipmi import jpeg_parse
from oracle import jpeg_oracle

NAT = jpeg_oracle.NATURAL.tolist() + [63] * 16       # jutils.c jpeg_natural_order with its 16 guard entries


class Corrupt(Exception):
    """The device reports this file (status 1 or 2): Pillow decides."""


def geometry(p):
    """-> (mx, my, bpm, hv): MCU grid, blocks per MCU, luma blocks per MCU"""
    hs, vs = (p.hs, p.vs) if p.ncomp == 3 else (1, 1)
    hv = hs * vs
    return -(-p.width // (8 * hs)), -(-p.height // (8 * vs)), (hv + 2 if p.ncomp == 3 else 1), hv


def scan_blocks(p, scan):
    """The slots (MCU-order block indices, the layout jpeg_oracle / jpeg_idct_kernel use) a scan visits, in its order, with
    the component of each. Non-interleaved scans walk the component's own block grid, interleaved ones the MCUs."""
    mx, my, bpm, hv = geometry(p)
    hs, vs = (p.hs, p.vs) if p.ncomp == 3 else (1, 1)
    out = []
    if len(scan.comps) == 1:
        c = scan.comps[0]
        if c == 0:
            cw, ch = -(-p.width // 8), -(-p.height // 8)
            for by in range(ch):
                for bx in range(cw):
                    out.append((((by // vs) * mx + bx // hs) * bpm + (by % vs) * hs + bx % hs, c))
        else:
            cw, ch = -(-(-(-p.width // hs)) // 8), -(-(-(-p.height // vs)) // 8)
            for by in range(ch):
                for bx in range(cw):
                    out.append(((by * mx + bx) * bpm + hv + c - 1, c))
    else:
        for m in range(mx * my):
            for c in scan.comps:
                for k in range(hv if c == 0 else 1):
                    out.append((m * bpm + (k if c == 0 else hv + c - 1), c))
    return out


class _Bits:
    def __init__(self, stream):
        self.s = stream + b"\0" * 8
        self.n = 8 * len(stream)
        self.p = 0

    def get(self, k):
        if k == 0:
            return 0
        p = self.p
        w = int.from_bytes(self.s[p >> 3:(p >> 3) + 5], "big")
        self.p += k
        return (w >> (40 - (p & 7) - k)) & ((1 << k) - 1)

    def huff(self, lut):
        ln, sy = lut
        p = self.p
        w = (int.from_bytes(self.s[p >> 3:(p >> 3) + 3], "big") >> (8 - (p & 7))) & 0xFFFF
        if ln[w] == 0:
            raise Corrupt("bad Huffman code")
        self.p += ln[w]
        return sy[w]


def _lut(rec):
    bits = tuple(rec[:16])
    return jpeg_oracle._huff_lut(bits, tuple(rec[16:16 + sum(bits)]))


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _s16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def coefficients(p):
    """Progressive record -> int32 [blocks][64], natural order, blocks in MCU order; final values (DC absolute, every
    refinement applied), as jdphuff.c leaves them. Raises Corrupt where the device reports the file."""
    mx, my, bpm, hv = geometry(p)
    coef = np.zeros((mx * my * bpm, 64), np.int64)
    for sc in p.scans:
        br = _Bits(sc.stream)
        blocks = scan_blocks(p, sc)
        al = sc.al
        p1, m1 = 1 << al, -(1 << al)
        if sc.ss == 0:
            luts = {c: _lut(t) for c, t in zip(sc.comps, sc.dc)} if not sc.ah else {}
            pred = [0, 0, 0]
            for b, c in blocks:
                if sc.ah == 0:
                    s = br.huff(luts[c])
                    pred[c] += _extend(br.get(s), s)
                    coef[b, 0] = _s16(pred[c] << al)
                elif br.get(1):
                    coef[b, 0] = _s16(coef[b, 0] | p1)
        else:
            lut = _lut(sc.ac[0])
            eobrun = 0
            for b, _ in blocks:
                row = coef[b]
                if sc.ah == 0:
                    if eobrun:
                        eobrun -= 1
                        continue
                    k = sc.ss
                    while k <= sc.se:
                        rs = br.huff(lut)
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            if k > sc.se:
                                raise Corrupt("coefficient behind the band")
                            row[NAT[k]] = _s16(_extend(br.get(s), s) << al)
                        elif r == 15:
                            k += 15
                        else:
                            eobrun = (1 << r) + br.get(r) - 1
                            break
                        k += 1
                    continue
                k = sc.ss
                if not eobrun:
                    while k <= sc.se:
                        rs = br.huff(lut)
                        r, s = rs >> 4, rs & 15
                        if s:
                            if s != 1:
                                raise Corrupt("refinement value of more than one bit")
                            s = p1 if br.get(1) else m1
                        elif r != 15:
                            eobrun = (1 << r) + br.get(r)
                            break
                        while k <= sc.se:
                            z = NAT[k]
                            if row[z]:
                                if br.get(1) and not row[z] & p1:
                                    row[z] = _s16(row[z] + (p1 if row[z] >= 0 else m1))
                            else:
                                r -= 1
                                if r < 0:
                                    break
                            k += 1
                        if s:
                            if k > sc.se:
                                raise Corrupt("coefficient behind the band")
                            row[NAT[k]] = s
                        k += 1
                if eobrun:
                    while k <= sc.se:
                        z = NAT[k]
                        if row[z] and br.get(1) and not row[z] & p1:
                            row[z] = _s16(row[z] + (p1 if row[z] >= 0 else m1))
                        k += 1
                    eobrun -= 1
        if br.p > br.n:
            raise Corrupt("entropy-coded data ends early")
    return coef


def decode(data):
    """Progressive JPEG file bytes -> uint8 [H][W][3], the array of Image.open(...).convert("RGB"). Raises
    jpeg_parse.Unsupported (not for the device), Corrupt (the device reports it) or jpeg_oracle.Reported (IDCT range)."""
    p = data if isinstance(data, jpeg_parse.Progressive) else jpeg_parse.parse_progressive(data)
    coef = coefficients(p)
    mx, my, bpm, hv = geometry(p)
    hs, vs = (p.hs, p.vs) if p.ncomp == 3 else (1, 1)
    W, H = p.width, p.height
    planes, first = [], 0
    for ci in range(p.ncomp):
        h, v = (hs, vs) if ci == 0 else (1, 1)
        q = p.quant[ci].astype(np.int64)
        idx = (np.arange(mx * my)[:, None] * bpm + first + np.arange(h * v)[None, :]).reshape(-1)
        px = jpeg_oracle.idct_islow(coef[idx], q).reshape(my, mx, v, h, 8, 8)
        planes.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(my * v * 8, mx * h * 8))
        first += h * v
    if p.ncomp == 1:
        y = planes[0][:H, :W]
        return np.stack([y, y, y], axis=-1)
    y = planes[0][:H, :W].astype(np.int32)
    dw, dh = -(-W // hs), -(-H // vs)
    ch = []
    for pl in planes[1:]:
        if (hs, vs) == (1, 1):
            c = pl.astype(np.int32)
        elif (hs, vs) == (2, 1):
            c = jpeg_oracle._h2v1_fancy(pl, dw)
        else:
            c = jpeg_oracle._h2v2_fancy(pl, dw, dh)
        ch.append(c[:H, :W])
    cb, cr = ch[0] - 128, ch[1] - 128                     # jpeg_oracle.decode's jdcolor.c fixed-point tables
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


# ---- the writer

class _Geom:
    def __init__(self, info):
        comps = info["comps"]
        self.width, self.height, self.ncomp = info["width"], info["height"], len(comps)
        self.hs, self.vs = (comps[0][1], comps[0][2]) if len(comps) == 3 else (1, 1)


class _Scan:
    def __init__(self, comps):
        self.comps = comps


def optimal_table(freq):
    """symbol -> count  ->  (bits[16], vals): an optimal code limited to 16 bits with no all-ones code (jchuff.c
    jpeg_gen_optimal_table's reserved code point and length adjustment; ties broken differently, which no decoder cares about)"""
    syms = sorted(s for s, f in freq.items() if f)
    heap = [(freq[s], k, [s]) for k, s in enumerate(syms)] + [(1, len(syms), [256])]
    heapq.heapify(heap)
    size = {s: 0 for s in syms + [256]}
    uid = len(heap)
    while len(heap) > 1:
        f1, _, a = heapq.heappop(heap)
        f2, _, b = heapq.heappop(heap)
        for s in a + b:
            size[s] += 1
        heapq.heappush(heap, (f1 + f2, uid, a + b))
        uid += 1
    bits = [0] * 64
    for s, l in size.items():
        bits[max(l, 1)] += 1
    for i in range(63, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                     # the reserved code point: the longest, last code
    order = sorted(syms, key=lambda s: (size[s], s))
    return bits[1:17], order


def _codes(bits, vals):
    codes, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            codes[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return codes


def _nbits(v):
    return int(v).bit_length()


def _encode_scan(coef, geom, scan):
    """-> list of events: ('h', table key, symbol) | ('b', value, nbits), in jcphuff.c's order"""
    comps, ss, se, ah, al = scan
    ev = []
    blocks = scan_blocks(geom, _Scan(comps))
    if ss == 0:
        pred = [0, 0, 0]
        for b, c in blocks:
            v = int(coef[b, 0])
            if ah:
                ev.append(("b", (v >> al) & 1, 1))
                continue
            t = v >> al
            d, pred[c] = t - pred[c], t
            s = _nbits(abs(d))
            ev.append(("h", c, s))
            if s:
                ev.append(("b", (d if d >= 0 else d - 1) & ((1 << s) - 1), s))
        return ev
    state = dict(eobrun=0, be=[])

    def emit_eobrun():
        if state["eobrun"]:
            n = _nbits(state["eobrun"]) - 1
            ev.append(("h", 0, n << 4))
            if n:
                ev.append(("b", state["eobrun"] & ((1 << n) - 1), n))
            state["eobrun"] = 0
            ev.extend(("b", x, 1) for x in state["be"])
            state["be"] = []

    for b, _ in blocks:
        row = coef[b]
        if ah == 0:
            r = 0
            for k in range(ss, se + 1):
                v = int(row[NAT[k]])
                t = abs(v) >> al
                if t == 0:
                    r += 1
                    continue
                emit_eobrun()
                while r > 15:
                    ev.append(("h", 0, 0xF0))
                    r -= 16
                s = _nbits(t)
                ev.append(("h", 0, (r << 4) + s))
                ev.append(("b", (t if v >= 0 else ~t) & ((1 << s) - 1), s))
                r = 0
            if r > 0:
                state["eobrun"] += 1
                if state["eobrun"] == 0x7FFF:
                    emit_eobrun()
            continue
        absv = {k: abs(int(row[NAT[k]])) >> al for k in range(ss, se + 1)}
        eob = max([k for k in absv if absv[k] == 1], default=0)
        r, br = 0, []
        for k in range(ss, se + 1):
            t = absv[k]
            if t == 0:
                r += 1
                continue
            while r > 15 and k <= eob:
                emit_eobrun()
                ev.append(("h", 0, 0xF0))
                r -= 16
                ev.extend(("b", x, 1) for x in br)
                br = []
            if t > 1:
                br.append(t & 1)
                continue
            emit_eobrun()
            ev.append(("h", 0, (r << 4) + 1))
            ev.append(("b", 0 if row[NAT[k]] < 0 else 1, 1))
            ev.extend(("b", x, 1) for x in br)
            br = []
            r = 0
        if r > 0 or br:
            state["eobrun"] += 1
            state["be"] += br
            if state["eobrun"] == 0x7FFF or len(state["be"]) > 1000 - 64 + 1:
                emit_eobrun()
    emit_eobrun()
    return ev


def _bytes(ev, codes):
    acc, n, out = 0, 0, bytearray()
    for e in ev:
        if e[0] == "h":
            v, l = codes[e[1]][e[2]]
        else:
            v, l = e[1], e[2]
        acc = (acc << l) | v
        n += l
        while n >= 8:
            n -= 8
            out.append((acc >> n) & 255)
        acc &= (1 << n) - 1
    if n:
        out.append(((acc << (8 - n)) | ((1 << (8 - n)) - 1)) & 255)
    return bytes(out).replace(b"\xff", b"\xff\x00")


def _seg(m, payload):
    return bytes([0xFF, m]) + (len(payload) + 2).to_bytes(2, "big") + payload


def write(blob, script, tamper=None, tables=None):
    """Baseline JPEG file + scan script [(component indices, Ss, Se, Ah, Al), ...] -> progressive file with the same quantised
    coefficients. Every scan gets its own optimal tables (a DHT in front of it). tamper(scan index, scan, events) -> events:
    rewrites a scan's symbols before its tables are built (malformed files whose codes are all valid). tables: a length profile
    of jpeg_baseline.profile_table instead of the optimal one (codes no encoder writes: all at 16 bits, ...)."""
    info = jpeg_oracle.parse(blob)
    coef, _ = jpeg_oracle.decode_coefficients(info)
    geom = _Geom(info)
    comps = info["comps"]
    out = bytearray(b"\xff\xd8")
    out += _seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    for tq in sorted({c[3] for c in comps}):
        out += _seg(0xDB, bytes([tq]) + bytes(info["qt"][tq]))
    sof = bytes([8]) + info["height"].to_bytes(2, "big") + info["width"].to_bytes(2, "big") + bytes([len(comps)])
    for c in comps:
        sof += bytes([c[0], (c[1] << 4) | c[2], c[3]])
    out += _seg(0xC2, sof)
    for si, sc in enumerate(script):
        cs, ss, se, ah, al = sc
        ev = _encode_scan(coef, geom, sc)
        if tamper is not None:
            ev = tamper(si, sc, ev)
        keys = sorted({e[1] for e in ev if e[0] == "h"})
        codes, dht = {}, b""
        for key in keys:
            freq = {}
            for e in ev:
                if e[0] == "h" and e[1] == key:
                    freq[e[2]] = freq.get(e[2], 0) + 1
            if tables is None:
                bits, vals = optimal_table(freq)
            else:
                from jpeg_baseline import profile_table
                bits, vals = profile_table(tables, 0 if ss == 0 else 1, freq)
            codes[key] = _codes(bits, vals)
            dht += bytes([(0 if ss == 0 else 0x10) | key]) + bytes(bits) + bytes(vals)
        if dht:
            out += _seg(0xC4, dht)
        sos = bytes([len(cs)])
        for c in cs:
            t = c if ss == 0 else 0
            sos += bytes([comps[c][0], (t << 4) | t])
        out += _seg(0xDA, sos + bytes([ss, se, (ah << 4) | al]))
        out += _bytes(ev, codes)
    out += b"\xff\xd9"
    return bytes(out)


def scripts(ncomp):
    """Named scan scripts Pillow never writes; all complete"""
    cs = list(range(ncomp))
    chroma = [c for c in cs if c]
    out = {}
    # non-interleaved DC scans with successive approximation over two bits, then full bands
    out["dc_single_sa2"] = ([((c,), 0, 0, 0, 2) for c in cs] + [((c,), 0, 0, 2, 1) for c in cs] + [((c,), 0, 0, 1, 0) for c in cs]
                            + [((c,), 1, 63, 0, 0) for c in cs])
    # interleaved DC of the chroma pair beside luma's own; single-coefficient bands
    out["single_coef"] = ([((0,), 0, 0, 0, 0)] + ([(tuple(chroma), 0, 0, 0, 0)] if chroma else [])
                          + [((c,), k, k, 0, 0) for c in cs for k in range(1, 6)] + [((c,), 6, 63, 0, 0) for c in cs])
    # many split bands at Al = 1, one refinement over the whole band
    bands = [(1, 2), (3, 9), (10, 20), (21, 40), (41, 63)]
    out["split_bands"] = ([(tuple(cs), 0, 0, 0, 1)] + [((c,), a, b, 0, 1) for c in cs for a, b in bands] + [(tuple(cs), 0, 0, 1, 0)]
                          + [((c,), 1, 63, 1, 0) for c in cs])
    # deep successive approximation: three refinement steps everywhere, refinements in split bands
    out["deep_sa"] = ([(tuple(cs), 0, 0, 0, 3)] + [((c,), 1, 63, 0, 3) for c in cs]
                      + [s for al in (2, 1, 0) for s in [(tuple(cs), 0, 0, al + 1, al)] + [((c,), a, b, al + 1, al) for c in cs for a, b in ((1, 9), (10, 63))]])
    return out


def writer_cases(rng, big=True):
    """(file, name) of writer scripts over baseline files of every sampling, grey and odd sizes; with big, one 2 000 x 1 500
    grey file whose high band is one EOB run after another (runs reach 0x7FFF)."""
    out = []
    for (h, w), sub, grey in [((37, 53), 0, False), ((37, 53), 1, False), ((37, 53), 2, False), ((64, 96), 2, False),
                              ((29, 11), 0, True), ((100, 75), 1, False)]:
        y, x = np.mgrid[0:h, 0:w]
        a = np.clip(np.stack([120 + 90 * np.sin(x / 7.0 + y / 11.0), 128 + 60 * np.cos(y / 5.0), (x * 5 + y * 3) % 256], -1)
                    + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(a[..., 0] if grey else a).save(buf, format="JPEG", quality=int(rng.integers(40, 96)), subsampling=sub)
        base = buf.getvalue()
        for name, sc in scripts(1 if grey else 3).items():
            out.append((write(base, sc), f"{name}_{h}x{w}_{'grey' if grey else sub}"))
    if big:
        y, x = np.mgrid[0:1500, 0:2000]
        a = (128 + 100 * np.sin(x / 97.0) * np.cos(y / 61.0)).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=60)
        out.append((write(buf.getvalue(), [((0,), 0, 0, 0, 0), ((0,), 1, 9, 0, 0), ((0,), 10, 63, 0, 1), ((0,), 10, 63, 1, 0)]),
                    "long_eob_runs_2000x1500"))
    return out


def _eob_overrun(ev):
    """The scan's last EOBn symbol (and its run bits) -> EOB14 with all 14 run bits set"""
    for i in range(len(ev) - 1, -1, -1):
        e = ev[i]
        if e[0] == "h" and e[2] & 15 == 0 and e[2] >> 4 < 15:
            r = e[2] >> 4
            tail = ev[i + 2:] if r else ev[i + 1:]
            return ev[:i] + [("h", e[1], 14 << 4), ("b", (1 << 14) - 1, 14)] + tail
    return ev


def _run_overrun(ev):
    """The scan's first coefficient symbol (r, s) -> (15, s): a run past the band for all but the widest bands"""
    for i, e in enumerate(ev):
        if e[0] == "h" and e[2] & 15:
            return ev[:i] + [("h", e[1], 0xF0 | (e[2] & 15))] + ev[i + 1:]
    return ev


def malformed_corpus(rng):
    """(family, file) seeded malformed progressive files: bit flips and truncations inside individual scans, DHT mutations
    between scans, SOS parameter mutations, scans cut short before EOI, and writer files whose symbols were rewritten (tables
    built after the rewrite, so every code is valid) to EOB runs that overrun the scan and coefficient runs that overrun the
    band."""
    bases = []
    for (h, w), sub in [((48, 64), 0), ((40, 56), 1), ((64, 48), 2), ((33, 17), 2)]:
        y, x = np.mgrid[0:h, 0:w]
        a = np.clip(np.stack([128 + 80 * np.sin(x / 5.0), 128 + 50 * np.cos(y / 4.0), (x + y) * 3 % 256], -1)
                    + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=80, subsampling=sub, progressive=True)
        bases.append(buf.getvalue())
    bases += [b for b, _ in writer_cases(rng, big=False)[::3]]
    out = []
    for base in bases:
        p = jpeg_parse.parse_progressive(base)
        sos = [m.start() for m in jpeg_parse._MARKER.finditer(base) if base[m.start() + 1] == 0xDA]
        dht = [m.start() for m in jpeg_parse._MARKER.finditer(base) if base[m.start() + 1] == 0xC4 and m.start() > sos[0]]
        seg = []                                    # (first data byte, end) of every scan in the file
        for s0 in sos:
            L = int.from_bytes(base[s0 + 2:s0 + 4], "big")
            d0 = s0 + 2 + L
            e = jpeg_parse._MARKER.search(base, d0).start()
            seg.append((d0, e))
        for _ in range(12):
            d0, e = seg[int(rng.integers(len(seg)))]
            if e - d0 < 2:
                continue
            b = bytearray(base)
            for _ in range(int(rng.integers(1, 4))):
                k = int(rng.integers(d0, e))
                b[k] ^= 1 << int(rng.integers(8))
            out.append(("flip", bytes(b)))
            k = int(rng.integers(d0, e))
            out.append(("truncate", base[:k] + b"\xff\xd9"))
            out.append(("cut", base[:k]))
        for s0, (d0, e) in zip(sos, seg):          # a scan cut short: its data ends early, the rest of the file follows
            k = d0 + (e - d0) // 2
            out.append(("short_scan", base[:k] + base[e:]))
            b = bytearray(base)                     # SOS parameters: Ss, Se, Ah/Al
            ns = base[s0 + 4]
            k = s0 + 5 + 2 * ns + int(rng.integers(3))
            b[k] = int(rng.integers(256)) if rng.random() < 0.5 else (b[k] + int(rng.integers(1, 3))) & 255
            out.append(("sos", bytes(b)))
        for d in dht:
            L = int.from_bytes(base[d + 2:d + 4], "big")
            for _ in range(3):
                b = bytearray(base)
                k = int(rng.integers(d + 4, d + 2 + L))
                b[k] = (b[k] + int(rng.integers(1, 255))) & 255
                out.append(("dht", bytes(b)))
        assert p.scans
    # EOB runs that overrun the scan (the last EOBn of an AC scan rewritten to EOB14 with all run bits set: 32 767 blocks), and
    # runs that overrun the band (the first coefficient of a first AC scan moved 15 places further); every code stays valid
    y, x = np.mgrid[0:40, 0:56]
    for sub in (0, 2):
        a = np.clip(np.stack([128 + 80 * np.sin(x / 6.0), 128 + 40 * np.cos(y / 5.0), (x + 2 * y) % 256], -1)
                    + rng.normal(0, 8, (40, 56, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=70, subsampling=sub)
        base = buf.getvalue()
        for name, script in scripts(3).items():
            ac = [k for k, sc in enumerate(script) if sc[1]]
            for target in ac[::max(1, len(ac) // 4)]:
                out.append(("eob_scan", write(base, script, tamper=lambda si, sc, ev, t=target: _eob_overrun(ev) if si == t else ev)))
                if script[target][3] == 0:
                    out.append(("run_band", write(base, script, tamper=lambda si, sc, ev, t=target: _run_overrun(ev) if si == t else ev)))
    return out
