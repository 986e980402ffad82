"""The host side of the two PNG switches `chunks` and `deep` (png_parse.parse, png.pack, decode_worker.stage_png, device_stage's
records) on the CPU, against Pillow run live: a file Pillow refuses is never let through, a file let through gives the pixels of
the same file without the chunk, and the committed fixture still says what Pillow says."""
import io
import os

import numpy as np
import pytest
from PIL import Image

from clipmi import png, png_parse
import png_cases
import png_deep_cases as D
import png_mode_cases as M

pytestmark = pytest.mark.filterwarnings("ignore")
HANDLED = (b"iCCP", b"zTXt", b"iTXt", b"eXIf", b"tRNS", b"acTL", b"IHDR", b"PLTE")


def _parse(blob, **kw):
    try:
        return png_parse.parse(blob, **kw)
    except png_parse.Unsupported:
        return None


@pytest.fixture(scope="module")
def base():
    b = D.base_image(np.random.default_rng(310))
    return b, D.transform_ref(D.with_chunk(b, b"", "before"))


def _check(blob, free_ref, name):
    """the rule of every chunk test: Pillow raises -> refused; let through -> Pillow's pixels are those of the chunk-free file"""
    ref, p = D.transform_ref(blob), _parse(blob, chunks=True)
    if ref is None:
        assert p is None, f"{name}: Pillow refuses the file, the parser lets it through"
    if p is not None:
        assert ref is not None and np.array_equal(ref, free_ref), f"{name}: let through, and Pillow's pixels differ from the chunk-free file's"
    return ref, p


def test_the_base_file_is_what_the_issue_used(base):
    (w, h, _), ref = base
    assert (w, h) == (300, 260) and ref.shape == (3, 224, 224)
    assert png_parse.parse(D.with_chunk(base[0], b"", "before")).chunks == 0


@pytest.mark.parametrize("where", ["before", "after"])
def test_chunks_that_change_nothing_are_let_through(base, where):
    """valid metadata chunks, compressed chunks with bad or cut zlib data and the malformed shapes Pillow ignores: let through with
    chunks=True, marked, with the chunk-free file's pixels from Pillow and the chunk-free file's stream; refused without the flag
    wherever they are refused today"""
    b, free_ref = base
    free = png_parse.parse(D.with_chunk(b, b"", "before"))
    for name, chunk in D.valid_chunks() + D.broken_zlib_chunks() + D.tolerated_shapes():
        blob = D.with_chunk(b, chunk, where)
        ref, p = _check(blob, free_ref, f"{name} {where}")
        assert ref is not None, f"{name} {where}: Pillow was expected to open this file"
        assert p is not None, f"{name} {where}: not let through"
        needs = where == "before" or any(c in chunk for c in HANDLED)
        assert p.chunks == int(needs) and p.stream == free.stream and (p.width, p.height, p.kind, p.depth) == (300, 260, "rgb", 8)
        assert (_parse(blob) is None) == needs, f"{name} {where}: without the flag"


@pytest.mark.parametrize("where", ["before", "after"])
def test_chunks_that_make_pillow_fail_are_refused(base, where):
    b, free_ref = base
    for name, chunk, behind in D.failing_chunks():
        blob = D.with_chunk(b, chunk, where)
        ref, p = _check(blob, free_ref, f"{name} {where}")
        if behind is not None and (where == "before" or behind):          # (None: still refused, whatever Pillow makes of it)
            assert ref is None, f"{name} {where}: Pillow was expected to fail"
        if where == "before" or behind is not False:
            assert p is None, f"{name} {where}: let through"
            assert _parse(blob) is None


@pytest.mark.parametrize("where", ["before", "after"])
def test_the_inflate_is_bounded_like_pillows(base, where):
    """a profile or text that inflates to the cap minus one byte passes; one that reaches the cap is refused (Pillow accepts exactly
    the cap: the parser hands such a file back); the text total counts what was inflated"""
    b, free_ref = base
    for name, chunk in D.bound_chunks():
        ref, p = _check(D.with_chunk(b, chunk, where), free_ref, f"{name} {where}")
        assert (p is not None) == name.endswith("minus_1"), name
        assert ref is not None
    half = D.C(b"zTXt", b"k\0\0" + D.z(png_parse.MAX_TEXT_BYTES // 2))
    plain = D.C(b"iTXt", b"k\0\0\0\0\0" + b"t" * 16) + D.C(b"tEXt", b"k\0" + b"t" * 14)
    for chunks, ok in ((half + half, True), (half + half + D.C(b"tEXt", b"k\0v"), False), (half + half + D.C(b"iTXt", b"k\0\0\0\0\0v"), False),
                       (half + D.C(b"iTXt", b"k\0\1\0\0\0" + D.z(png_parse.MAX_TEXT_BYTES // 2 - 32)) + plain, True),
                       (half + D.C(b"iTXt", b"k\0\1\0\0\0" + D.z(png_parse.MAX_TEXT_BYTES // 2 - 32)) + plain + D.C(b"zTXt", b"k\0\0" + D.z(1)), False)):
        ref, p = _check(D.with_chunk(b, chunks, where), free_ref, f"text total {where}")
        assert (p is not None) == ok and ref is not None
    # split between the two sides of the image data: one total
    w, h, zz = b
    both = png_cases.assemble(w, h, 3, zz, before=half, after=half + D.C(b"zTXt", b"k\0\0" + D.z(1)))
    assert _parse(both, chunks=True) is None and _parse(png_cases.assemble(w, h, 3, zz, before=half, after=half), chunks=True) is not None


def test_trns_on_grey_and_rgb_files():
    """tRNS of exactly 2 bytes on 8-bit grey and of exactly 6 on RGB (depth 8 and 16), in front of and behind the image data; every other
    length, the alpha colour types and grey below depth 8 stay refused"""
    cases = D.trns_cases(np.random.default_rng(311))
    assert len(cases) == 24
    for name, blob, free in cases:
        ref = D.transform_ref(blob, 32)
        p = _parse(blob, chunks=True, modes=True, deep=True)
        assert (p is not None) == (name.split("_", 1)[1].rsplit("_", 1)[0] in ("grey8_2", "rgb8_6", "rgb16_6")), name
        if ref is None:
            assert p is None, name
        if p is not None:
            assert p.chunks == 1 and np.array_equal(ref, D.transform_ref(free, 32)), name
            assert p.stream == png_parse.parse(free, deep=True).stream
        assert _parse(blob, modes=True, deep=True) is None, name        # (the palette rule is the only tRNS let through without the flag)
    # the palette rule stays as it is: with the flag a palette file's tRNS is taken where it was, and refused where it was
    rng = np.random.default_rng(312)
    s, pal = M.samples_for(rng, 3, 8, 9, 9, 0, 20)
    good = M.write(s, 3, 8, palette=pal, alphas=[1, 2, 3])
    long = M.write(s, 3, 8, palette=pal, alphas=[7] * 21)
    behind = png_cases.assemble(9, 9, 1, png_cases.deflate(M.scanlines(s, 3, 8)), before=M.plte(pal), after=M.trns([1, 2]), depth=8, ctype=3)
    for kw in ({}, {"chunks": True}):
        assert _parse(good, modes=True, **kw).chunks == 0 and _parse(long, modes=True, **kw) is None and _parse(behind, modes=True, **kw) is None


def test_deep_files_are_parsed_by_kind():
    rng = np.random.default_rng(313)
    for ctype in D.CTYPES:
        ch = D.SAMPLES[ctype]
        for lace in (0, 1):
            s = D.samples16(rng, ctype, 19, 13, 1)
            blob = D.write16(s, ctype, lace=lace)
            kw = dict(modes=True, interlaced=True, deep=True)
            p = png_parse.parse(blob, **kw)
            assert (p.kind, p.channels, p.depth, p.ctype, p.interlace, p.chunks, p.px8) == (D.KIND[ctype], ch, 16, ctype, lace, 0, True)
            assert p.row_bytes() == 13 * ch * 2
            raw = D.lace_scanlines16(s) if lace else D.scanlines16(s)
            assert p.raw_bytes() == len(raw) and png_cases.inflate_exact(p.stream, p.raw_bytes()) == raw
            assert (p.raw_bytes() == 19 * (1 + 13 * ch * 2)) == (not lace)
            # refused without the flag, and without the flags of the file's other properties
            assert _parse(blob, modes=True, interlaced=True) is None and _parse(blob, modes=True, interlaced=True, chunks=True) is None
            assert (_parse(blob, deep=True, interlaced=True) is not None) == (ctype == 2)
            assert (_parse(blob, deep=True, modes=True) is not None) == (not lace)
            # Pillow opens it as the high bytes
            assert np.array_equal(D.pillow_pixels(blob), D.high_bytes(s, ctype))
    # 16-bit grey and a "16-bit palette" stay refused, whatever is on
    g = png_cases.assemble(13, 19, 1, png_cases.deflate(png_cases.filter_rows(png_cases.noise(rng, 19, 13, 2), [0] * 19)), depth=16, ctype=0)
    assert Image.open(io.BytesIO(g)).mode == "I;16"
    p16 = png_cases.assemble(13, 19, 1, png_cases.deflate(bytes(19 * 27)), before=M.plte(np.zeros((4, 3))), depth=16, ctype=3)
    for blob in (g, p16):
        assert _parse(blob, modes=True, interlaced=True, chunks=True, deep=True) is None
    # an 8-bit file is what it was
    old = png_cases.write(png_cases.smooth(rng, 9, 9, 3))
    a, b = png_parse.parse(old), png_parse.parse(old, deep=True, chunks=True)
    assert (a.kind, a.depth, a.px8, a.chunks, a.stream) == (b.kind, b.depth, b.px8, b.chunks, b.stream) == ("rgb", 8, False, 0, a.stream)


def test_deep_rows_up_to_the_lds_row():
    """rows of exactly 49152 bytes are taken, one pixel more is refused (the header decides: the stream is not looked at)"""
    z = png_cases.deflate(b"\0" * 64)
    for ctype in D.CTYPES:
        w = D.MAX_WIDTH[ctype]
        assert w * D.SAMPLES[ctype] * 2 == png_parse.MAX_ROW_BYTES
        p = png_parse.parse(png_cases.assemble(w, 2, 1, z, depth=16, ctype=ctype), modes=True, deep=True)
        assert p.row_bytes() == png_parse.MAX_ROW_BYTES and p.raw_bytes() == 2 * (1 + png_parse.MAX_ROW_BYTES)
        with pytest.raises(png_parse.Unsupported, match="rows too wide"):
            png_parse.parse(png_cases.assemble(w + 1, 2, 1, z, depth=16, ctype=ctype), modes=True, deep=True)


def test_pack_sends_deep_files_to_px8():
    rng = np.random.default_rng(314)
    blobs = [D.deep_file(rng, 2, 5, 7), D.deep_file(rng, 6, 3, 9, lace=1), D.deep_file(rng, 4, 8, 2), M.mode_file(rng, 6, 8, 4, 4)]
    items = [png_parse.parse(b, modes=True, interlaced=True, deep=True) for b in blobs]
    recs, streams, out_bytes, total_raw, max_raw = png.pack(items)
    assert [int(r["reserved"][0]) for r in recs] == [2 << 8 | 16, png.INTERLACE_BIT | 6 << 8 | 16, 4 << 8 | 16, 6 << 8 | 8]
    assert [int(r["channels"]) for r in recs] == [3, 4, 2, 4]
    assert list(recs["out_off"]) == [0, 112, 224, 288] and out_bytes == 352          # 5 x 7 x 3, 3 x 9 x 4, 8 x 2 x 4, 4 x 4 x 4, each rounded up to 16
    assert max_raw == max(it.raw_bytes() for it in items) and total_raw == sum((it.raw_bytes() + 15) // 16 * 16 for it in items)
    rgb, px8 = png._parsed(blobs + [png_cases.write(png_cases.noise(rng, 3, 3, 3))], True, True, False, True)
    assert [k for k, _ in rgb] == [4] and [k for k, _ in px8] == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="different entries"):
        png.decode_device([items[0], png_parse.parse(png_cases.write(png_cases.noise(rng, 3, 3, 3)))], "cuda:0")
    assert png._parsed(blobs[:3], True, True) == ([], [])     # without deep: none


def test_mode_bits_and_stager_switches():
    from clipmi import decode_worker as dw
    assert (dw.PNG_CHUNKS_BIT, dw.PNG_DEEP_BIT, dw.PNG_CHUNKS_STAT, dw.PNG_DEEP_STAT) == (256, 512, "png_chunk_files", "png_deep_files")
    others = [dw.LAYOUTS_BIT, dw.PNG_INTERLACED_BIT, dw.FULL_SIZE.bit] + sorted({k.bit for k in dw.ALL_PARSED})
    for bit in (dw.PNG_CHUNKS_BIT, dw.PNG_DEEP_BIT):
        assert bit & (bit - 1) == 0 and not any(bit & o for o in others)
    assert dw.PNG_CHUNKS_BIT != dw.PNG_DEEP_BIT and (dw.HDR.CHUNKS, dw.HDR.DEPTH, dw.HDR.CTYPE) == (27, 20, 21)
    every = dw.PNG_CHUNKS_BIT | dw.PNG_DEEP_BIT | dw.PNG_INTERLACED_BIT | dw.LAYOUTS_BIT
    assert dw._stager_switches(every | 8, "png") == {"interlaced": True, "chunks": True, "deep": True}
    assert dw._stager_switches(every | 2, "jpeg") == {"layouts": True}
    assert dw._stager_switches(dw.PNG_CHUNKS_BIT | 8, "png") == {"chunks": True} and dw._stager_switches(dw.PNG_DEEP_BIT | 24, "png") == {"deep": True}
    assert dw._stager_switches(8 | 16, "png") == {} and dw._stager_switches(dw.PNG_CHUNKS_BIT | dw.PNG_DEEP_BIT, "jpeg") == {}
    # the kinds are the ones there were: a 16-bit RGB file is a KIND_PNG region with a mark
    assert [k.kind for k in dw.ALL_PARSED] == [3, 4, 6, 7, 8, 9]


def test_stage_png_writes_what_device_stage_reads(clipmi, tmp_path):
    """stage_png with the switches: depth and colour type of a 16-bit file at HDR.DEPTH / HDR.CTYPE (a KIND_PNG region too), HDR.CHUNKS
    for a file that needed chunks=True; with the switches off the files are refused and the old files' regions are byte for byte what
    they were. device_stage sizes the scanlines, builds png.pack's records, keeps 8-bit and 16-bit KIND_PNG files apart and sends the
    latter to clipmi_png_decode_px8."""
    from clipmi import decode_worker as dw, device_stage
    rng = np.random.default_rng(315)
    icc = D.C(b"iCCP", b"p\0\0" + D.z(200))
    files = [("rgb8", png_cases.write(png_cases.smooth(rng, 50, 60, 3), "cycle"), 6),
             ("rgb16", D.deep_file(rng, 2, 40, 30, 1), 6),
             ("rgb8_icc", png_cases.write(png_cases.smooth(rng, 21, 22, 3), "cycle", before=icc), 6),
             ("rgb16_lace_icc", D.deep_file(rng, 2, 19, 13, 2, lace=1, before=icc + D.C(b"tRNS", b"\0\1\0\2\0\3")), 6),
             ("grey8_trns", png_cases.write(png_cases.smooth(rng, 30, 31, 1), "cycle", before=D.C(b"tRNS", b"\0\7")), 6),
             ("rgba16", D.deep_file(rng, 6, 33, 35, 0), 7), ("la16_lace", D.deep_file(rng, 4, 9, 20, 1, lace=1), 7),
             ("rgba8_exif", M.mode_file(rng, 6, 8, 20, 20, 1, before=D.C(b"eXIf", D.EXIF6)), 7),
             ("p4_unknown", M.mode_file(rng, 3, 4, 20, 21, 1, before=D.C(b"iDOT", b"1234")), 8)]
    n, cap, n_px = len(files), 64 << 10, 224
    on = dict(interlaced=True, chunks=True, deep=True)
    big = np.full(n * cap, 0xAB, np.uint8)
    stagers = {s.kind: s.stager for s in dw.PARSED}
    items = []
    for k, (name, blob, kind) in enumerate(files):
        region = big[k * cap:(k + 1) * cap]
        p = png_parse.parse(blob, modes=True, **on)
        items.append(p)
        new = p.depth == 16 or p.chunks
        for other in (6, 7, 8):                               # the stagers of the other kinds refuse the file
            if other != kind:
                with pytest.raises(png_parse.Unsupported):
                    stagers[other]("-", n_px, region, blob, **on)
        if new:
            with pytest.raises(png_parse.Unsupported):
                stagers[kind]("-", n_px, region, blob, interlaced=True)
            for drop in ("chunks", "deep"):
                if (drop == "chunks" and p.chunks) or (drop == "deep" and p.depth == 16):
                    with pytest.raises(png_parse.Unsupported):
                        stagers[kind]("-", n_px, region, blob, **{k_: v for k_, v in on.items() if k_ != drop})
            assert region.min() == 0xAB
        got = stagers[kind]("-", n_px, region, blob, **on)
        assert got[:2] == (p.width, p.height) and 0 < got[2] <= cap
        ints = np.frombuffer(region, np.int32, count=dw.JPEG_HDR_INTS)
        assert list(ints[:8]) == [kind, p.width, p.height, p.channels, 0, 0, len(p.stream), 0], name
        want = [16, 2, 0, 0] if name.startswith("rgb16") else [0, 0, 0, 0] if kind == 6 else [p.depth, p.ctype, p.n_entries, 0]
        assert list(ints[20:24]) == want, name
        assert list(ints[24:]) == [0, 0, p.interlace, p.chunks, 0, 0, 0, 0], name
        assert (ints[dw.HDR.CHUNKS], ints[dw.HDR.DEPTH] == 16) == (p.chunks, p.depth == 16)
        if not new:                                           # an old file: the region it got before
            old = np.full(cap, 0xAB, np.uint8)
            assert dw.stage_png("-", n_px, old, blob, modes=True) == got and np.array_equal(old, region)
    assert [it.chunks for it in items] == [0, 0, 1, 1, 1, 0, 0, 1, 1]
    for px, kind in ((3, 6), (4, 7), (1, 8)):
        slots = np.array([k for k, f in enumerate(files) if f[2] == kind])
        hd = device_stage._headers(big, n, cap, slots)
        mine = [items[k] for k in slots]
        assert list(device_stage._png_scanlines(hd, px)) == [it.raw_bytes() for it in mine]
        assert list(device_stage._png_deep(hd)) == [it.depth == 16 for it in mine]
        recs, jobs, out_sz, raw_sz = device_stage.png_records(big, n, cap, slots, np.arange(n), n_px, px=px)
        ref = png.pack(mine)[0]
        for f in ("stream_bytes", "width", "height", "channels", "raw_off", "out_off", "reserved"):
            assert np.array_equal(recs[f], ref[f]), (px, f)
    # KIND_PNG: the 16-bit files sort behind the 8-bit ones, groups are cut between them, and each goes to its entry
    slots = np.array([0, 1, 2, 3, 4])
    hd = device_stage._headers(big, n, cap, slots)
    deep = device_stage._png_deep(hd)
    order = slots[np.argsort(deep, kind="stable")]
    assert list(order) == [0, 2, 4, 1, 3]
    assert device_stage._split([(0, 5)], deep[np.argsort(deep, kind="stable")]) == [(0, 3), (3, 5)]
    assert device_stage._split([(0, 2), (2, 5)], np.array([False, False, True, True, True])) == [(0, 2), (2, 5)]
    assert device_stage._split([(0, 4)], np.zeros(4, bool)) == [(0, 4)] and device_stage._split([], np.zeros(0, bool)) == []
    L = clipmi._lib.lib()
    fmt = device_stage.all_formats()[dw.KIND_PNG]
    assert fmt.group(L, fmt.records(big, n, cap, order[:3], np.arange(n), n_px))[3] == "clipmi_png_decode_rgb8"
    assert fmt.group(L, fmt.records(big, n, cap, order[3:], np.arange(n), n_px))[3] == "clipmi_png_decode_px8"
    with pytest.raises(ValueError, match="mixes"):
        fmt.group(L, fmt.records(big, n, cap, order, np.arange(n), n_px))
    # a JPEG region keeps its restart interval where a PNG region keeps its depth: not taken for a 16-bit file
    fake = hd.copy()
    fake[:, dw.HDR.KIND], fake[:, dw.HDR.DEPTH] = dw.KIND_BASELINE, 16
    assert not device_stage._png_deep(fake).any()


def test_png_max_raw_counts_the_16_bit_scanlines(monkeypatch):
    from clipmi import decode_worker as dw
    blob = D.deep_file(np.random.default_rng(316), 2, 40, 50, 1)
    p = png_parse.parse(blob, deep=True)
    assert p.raw_bytes() == 40 * (1 + 50 * 6)
    region = np.zeros(1 << 16, np.uint8)
    monkeypatch.setattr(dw, "PNG_MAX_RAW", p.raw_bytes())
    assert dw.stage_png("-", 224, region, blob, deep=True)[2] > 0
    monkeypatch.setattr(dw, "PNG_MAX_RAW", p.raw_bytes() - 1)
    with pytest.raises(png_parse.Unsupported, match="PNG_MAX_RAW"):
        dw.stage_png("-", 224, region, blob, deep=True)


def test_encode_files_takes_the_switches():
    import inspect
    from clipmi import pipeline
    sig = inspect.signature(pipeline.encode_files)
    assert sig.parameters["device_png_chunks"].default is None and sig.parameters["device_png_deep"].default is None
    doc = pipeline.encode_files.__doc__
    for word in ("CLIPMI_DEVICE_PNG_CHUNKS", "CLIPMI_DEVICE_PNG_DEEP", "png_chunk_files", "png_deep_files"):
        assert word in doc, word


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_deep.npz")


def test_fixture_is_what_pillow_says_today():
    """tests/golden/png_deep.npz against Pillow run live: a difference here is Pillow's drift, not a device fault"""
    assert os.path.getsize(GOLDEN) < 200_000
    d = np.load(GOLDEN)
    n, n_px = int(d["n"]), int(d["n_px"])
    assert 10 <= n <= 16 and n_px == 32
    kinds = set()
    for i in range(n):
        blob = d[f"file_{i}"].tobytes()
        im = Image.open(io.BytesIO(blob))
        assert max(im.size) <= 40
        assert np.array_equal(np.asarray(im), d[f"px_{i}"]), i
        assert np.array_equal(M.load_uint8_blob(blob, n_px), d[f"out_{i}"]), i
        p = png_parse.parse(blob, modes=True, interlaced=True, chunks=True, deep=True)
        assert p.depth == 16 or p.chunks
        kinds.add((p.ctype, p.depth, p.interlace, p.chunks))
    assert {k[:3] for k in kinds} >= {(c, 16, lace) for c in D.CTYPES for lace in (0, 1)}
    assert (2, 8, 0, 1) in kinds and (0, 8, 0, 1) in kinds and (6, 16, 0, 1) in kinds
