"""The host side of Adam7-interlaced PNG files on the device (png_parse.parse(interlaced=True), png.pack, decode_worker.stage_png,
device_stage.png_records), and the numpy restatement of the interlaced decode (png_interlace_cases) against Pillow, which is the
oracle of the GPU tests in test_png_interlace_gpu.py. No GPU."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

from clipmi import png, png_parse
import png_cases
import png_interlace_cases as A
import png_mode_cases as M

pytestmark = pytest.mark.filterwarnings("ignore:Palette images with Transparency")
FIELDS = ("width", "height", "channels", "stream", "kind", "depth", "ctype", "n_entries")


@pytest.fixture(scope="module")
def files():
    return A.cases(np.random.default_rng(90))


def test_pass_geometry_against_a_brute_force_count():
    """adam7_passes and adam7_raw_bytes against counting the pixels of every (x % 8, y % 8) class (PNG 1.2, 8.2: the pattern
    1 6 4 6 2 6 4 6 / 7.. / 5 6 5 6.. / 7.. / 3 6 4 6 3 6 4 6 / 7.. / 5 6 5 6.. / 7..), all sizes 1..17 x 1..17"""
    pattern = ["16462646", "77777777", "56565656", "77777777", "36463646", "77777777", "56565656", "77777777"]
    assert [tuple(t) for t in png_parse.ADAM7] == list(A.PASSES)
    for w in range(1, 18):
        for h in range(1, 18):
            cols = [[set() for _ in range(7)], [set() for _ in range(7)]]
            for y in range(h):
                for x in range(w):
                    p = int(pattern[y % 8][x % 8]) - 1
                    cols[0][p].add(x)
                    cols[1][p].add(y)
            geo = png_parse.adam7_passes(w, h)
            assert len(geo) == 7
            for p, (x0, y0, dx, dy, pw, ph) in enumerate(geo):
                assert (x0, y0, dx, dy) == A.PASSES[p]
                xs, ys = sorted(cols[0][p]), sorted(cols[1][p])
                if xs:                                         # a non-empty pass: its pixels are exactly the class's
                    assert (pw, ph) == (len(xs), len(ys)) and xs == list(range(x0, w, dx)) and ys == list(range(y0, h, dy)), (w, h, p)
                else:
                    assert pw == 0 or ph == 0, (w, h, p)
            for bits in (1, 2, 4, 8, 16, 24, 32):
                want = sum(len(ys) * (1 + (len(xs) * bits + 7) // 8) for xs, ys in zip(*cols) if xs)
                assert png_parse.adam7_raw_bytes(w, h, bits) == want, (w, h, bits)
    w, h = np.array([1, 9, 17, 300]), np.array([1, 5, 17, 200])         # the array form device_stage uses
    assert list(png_parse.adam7_raw_bytes(w, h, np.array([8, 24, 4, 32]))) == [
        png_parse.adam7_raw_bytes(int(a), int(b), c) for a, b, c in zip(w, h, (8, 24, 4, 32))]


def test_interlaced_files_need_the_flag(files):
    """Without the flag every interlaced file is Unsupported, as before; with it the size, kind, depth, palette and raw_bytes()
    are right; alpha, palette and low-depth files still need modes=True; interlace methods above 1 stay refused."""
    seen = set()
    for name, b in files:
        depth, ctype = b[24], b[25]
        for kw in ({}, {"modes": True}):
            with pytest.raises(png_parse.Unsupported):
                png_parse.parse(b, **kw)
        old = depth == 8 and ctype in (0, 2)
        if not old:
            with pytest.raises(png_parse.Unsupported):
                png_parse.parse(b, interlaced=True)
        p = png_parse.parse(b, modes=True, interlaced=True)
        im = Image.open(io.BytesIO(b))
        assert p.interlace == 1 and im.info.get("interlace") == 1 and (p.width, p.height) == im.size, name
        assert (p.ctype, p.depth, p.channels, p.kind) == (ctype, depth, A.SAMPLES[ctype], A.MODES[(ctype, depth)]), name
        if p.kind == "index":
            pal, n = M.pillow_palette(b)
            assert p.n_entries == n and np.array_equal(p.palette, pal), name
        want = sum(len(range(y0, p.height, dy)) * (1 + (len(range(x0, p.width, dx)) * p.channels * p.depth + 7) // 8)
                   for x0, y0, dx, dy in A.PASSES if x0 < p.width and y0 < p.height)
        assert p.raw_bytes() == want and p.row_bytes() == (p.width * p.channels * p.depth + 7) // 8, name
        seen.add((ctype, depth))
    assert seen == set(A.MODES)
    b = bytearray(files[0][1])
    for lace in (2, 3, 255):
        b[28] = lace
        bad = bytes(b[:29]) + png_cases.chunk(b"IHDR", bytes(b[16:29]))[-4:] + bytes(b[33:])
        with pytest.raises(png_parse.Unsupported, match="interlaced"):
            png_parse.parse(bad, modes=True, interlaced=True)


def test_the_flag_changes_nothing_for_files_that_are_not_interlaced():
    rng = np.random.default_rng(91)
    blobs = [b for _, b in png_cases.writer_cases(rng)[::9]] + [b for _, b in M.transform_cases(rng)[::5]]
    assert len(blobs) > 30
    for b in blobs:
        for modes in (False, True):
            try:
                ref = png_parse.parse(b, modes=modes)
            except png_parse.Unsupported:
                with pytest.raises(png_parse.Unsupported):
                    png_parse.parse(b, modes=modes, interlaced=True)
                continue
            p = png_parse.parse(b, modes=modes, interlaced=True)
            assert p.interlace == 0 and ref.interlace == 0 and all(getattr(p, f) == getattr(ref, f) for f in FIELDS)
            assert (p.palette is None) == (ref.palette is None) and (p.palette is None or np.array_equal(p.palette, ref.palette))
            assert p.raw_bytes() == ref.raw_bytes() == p.height * (1 + p.row_bytes())


def test_restatement_equals_pillow(files):
    """The numpy restatement of the interlaced decode gives Pillow's pixels in the file's own mode and after convert("RGB"), for
    every file of the list the GPU test decodes - and the hand-written files are ones Pillow reads."""
    for name, b in files:
        p = png_parse.parse(b, modes=True, interlaced=True)
        got = A.cpu_decode(p)
        assert got is not None, name
        assert A.same((got, p.palette) if p.kind == "index" else got, b), name
        rgb = p.palette[got] if p.kind == "index" else got[..., :3]        # (convert("RGB") of an alpha file drops alpha)
        assert np.array_equal(rgb, np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))), name


def test_restatement_on_the_malformed_corpus():
    """The corpus of the GPU test holds what it says: the restatement accepts every "harmless" file and none with a wrong
    Adler-32, a filter byte above 4, rows too many or bytes too few, or scanlines in the other order; where it accepts, Pillow
    decodes the file to the same pixels."""
    corpus = A.malformed_corpus(np.random.default_rng(92))
    fams = {}
    for fam, b in corpus:
        p = png_parse.parse(b, modes=True, interlaced=True)
        got = A.cpu_decode(p) if p.interlace else (png_cases.cpu_decode(p) if p.kind == "rgb" else M.cpu_decode(p))
        c = fams.setdefault(fam, [0, 0])
        c[0] += 1
        if got is not None:
            c[1] += 1
            assert A.same((got, p.palette) if p.kind == "index" else got, b), fam
    assert fams["harmless"] == [20, 20] and fams["bitflip"][0] == 48 and fams["truncated"] == [28, 0]
    for fam, n in (("filter_byte", 12), ("adler_wrong", 8), ("adler_missing", 4), ("extra_rows", 4), ("short_data", 4), ("wrong_order", 8)):
        assert fams[fam] == [n, 0], (fam, fams[fam])


def test_pack_sets_the_bit_and_the_sizes(files):
    items = [png_parse.parse(b, modes=True, interlaced=True) for _, b in files[::3]]
    rng = np.random.default_rng(93)
    plain = [png_parse.parse(png_cases.write(png_cases.smooth(rng, 9, 9, 3))), png_parse.parse(M.mode_file(rng, 3, 4, 9, 13), modes=True)]
    for group in ([it for it in items if it.kind == "rgb"] + plain[:1], [it for it in items if it.kind != "rgb"] + plain[1:]):
        recs, streams, out_bytes, total_raw, max_raw = png.pack(group)
        roff = ooff = 0
        for r, it in zip(recs, group):
            low = 0 if it.kind == "rgb" else it.ctype << 8 | it.depth
            assert int(r["reserved"][0]) == (png.INTERLACE_BIT if it.interlace else 0) | low and png.INTERLACE_BIT == 1 << 16
            assert int(r["reserved"][1]) == (0 if it.kind == "rgb" else it.n_entries)
            assert (int(r["raw_off"]), int(r["out_off"])) == (roff, ooff)
            roff += (it.raw_bytes() + 15) // 16 * 16
            ooff += (it.width * it.height * png.PX_BYTES[it.kind] + 15) // 16 * 16
        assert (out_bytes, total_raw, max_raw) == (ooff, roff, max(it.raw_bytes() for it in group))
        assert int(recs[-1]["reserved"][0]) & png.INTERLACE_BIT == 0


def test_stage_png_marks_an_interlaced_region(tmp_path):
    """stage_png with the switch off refuses an interlaced file as before; with it on the region has the layout of any PNG
    region and HDR.INTERLACE says 1; a file that is not interlaced gets byte for byte the region it got without the switch; and
    device_stage sizes the scanlines and builds the records png.pack builds."""
    from clipmi import decode_worker as dw, device_stage
    rng = np.random.default_rng(94)
    assert dw.HDR.INTERLACE == 26 and dw.PNG_INTERLACED_BIT == 64 and dw.PNG_INTERLACED_STAT == "png_interlaced_files"
    assert not dw.PNG_INTERLACED_BIT & (dw.LAYOUTS_BIT | dw.FULL_SIZE.bit | sum({k.bit for k in dw.PARSED}))
    assert dw._stager_switches(dw.PNG_INTERLACED_BIT | 8, "png") == {"interlaced": True} and dw._stager_switches(8 | dw.LAYOUTS_BIT, "png") == {}
    assert dw._stager_switches(dw.PNG_INTERLACED_BIT | 2, "jpeg") == {} and dw._stager_switches(dw.LAYOUTS_BIT, "jpeg") == {"layouts": True}
    specs = [(2, 8, 64, 96, 6), (0, 8, 33, 70, 6), (6, 8, 40, 30, 7), (3, 4, 37, 41, 8), (0, 2, 21, 19, 7), (3, 1, 9, 200, 8)]
    n, cap, n_px = len(specs), 128 << 10, 224
    for px, kinds in ((3, (6,)), (4, (7,)), (1, (8,))):
        big = np.full(n * cap, 0xAB, np.uint8)
        slots, items = [], []
        for k, (ctype, depth, h, w, kind) in enumerate(specs):
            if kind not in kinds:
                continue
            blob = A.lace_file(rng, ctype, depth, h, w, k)
            path = tmp_path / f"f{px}_{k}.png"
            path.write_bytes(blob)
            region = big[k * cap:(k + 1) * cap]
            for kw in ({}, {"modes": True}):
                with pytest.raises(png_parse.Unsupported):
                    dw.stage_png(str(path), n_px, region, **kw)
            assert region.min() == 0xAB                        # (a refused file leaves its region alone)
            stager = {s.kind: s.stager for s in dw.PARSED}[kind]
            with pytest.raises(png_parse.Unsupported):
                stager(str(path), n_px, region)
            got = stager(str(path), n_px, region, interlaced=True)
            p = png_parse.parse(blob, modes=True, interlaced=True)
            assert got[:2] == (w, h) and 0 < got[2] <= cap
            ints = np.frombuffer(region, np.int32, count=dw.JPEG_HDR_INTS)
            assert list(ints[:8]) == [kind, w, h, p.channels, 0, 0, len(p.stream), 0]
            assert list(ints[20:24]) == ([0, 0, 0, 0] if kind == 6 else [depth, ctype, p.n_entries, 0])
            assert list(ints[24:]) == [0, 0, 1, 0, 0, 0, 0, 0]
            o = int(ints[dw.HDR.DATA_OFF])
            assert bytes(region[o:o + len(p.stream)]) == p.stream and not region[o + len(p.stream):got[2]].any()
            slots.append(k)
            items.append(p)
        # a file that is not interlaced, beside them: the same region with the switch on and off
        if px == 3:
            blob = png_cases.write(png_cases.smooth(rng, 50, 60, 3), "cycle")
        else:
            blob = M.mode_file(rng, 6 if px == 4 else 3, 8, 50, 60, 1)
        path = tmp_path / f"plain{px}.png"
        path.write_bytes(blob)
        a, b = np.full(cap, 0xAB, np.uint8), np.full(cap, 0xAB, np.uint8)
        assert dw.stage_png(str(path), n_px, a, modes=True) == dw.stage_png(str(path), n_px, b, modes=True, interlaced=True)
        assert np.array_equal(a, b) and np.frombuffer(b, np.int32, count=dw.JPEG_HDR_INTS)[dw.HDR.INTERLACE] == 0
        free = [k for k in range(n) if k not in slots][0]
        big[free * cap:(free + 1) * cap] = b
        slots.append(free)
        items.append(png_parse.parse(blob, modes=True))
        order = np.argsort(slots)
        slots, items = [slots[i] for i in order], [items[i] for i in order]
        recs, jobs, out_sz, raw_sz = device_stage.png_records(big, n, cap, slots, np.arange(n), n_px, px=px)
        ref = png.pack(items)[0]
        for f in ("stream_bytes", "width", "height", "channels", "raw_off", "out_off", "reserved"):
            assert np.array_equal(recs[f], ref[f]), (px, f)
        hd = device_stage._headers(big, n, cap, np.asarray(slots))
        assert list(device_stage._png_scanlines(hd, px)) == [it.raw_bytes() for it in items]
        assert list(raw_sz) == [(it.raw_bytes() + 15) // 16 * 16 for it in items]
        assert list(hd[:, dw.HDR.INTERLACE]) == [it.interlace for it in items]


def test_stage_png_applies_png_max_raw_to_the_passes(tmp_path, monkeypatch):
    from clipmi import decode_worker as dw
    blob = A.lace_file(np.random.default_rng(95), 2, 8, 40, 50, 1)
    p = png_parse.parse(blob, interlaced=True)
    assert p.raw_bytes() > p.height * (1 + p.row_bytes())       # the passes carry more filter bytes than the rows
    region = np.zeros(1 << 16, np.uint8)
    monkeypatch.setattr(dw, "PNG_MAX_RAW", p.raw_bytes())
    assert dw.stage_png("-", 224, region, blob, interlaced=True)[2] > 0
    monkeypatch.setattr(dw, "PNG_MAX_RAW", p.raw_bytes() - 1)
    with pytest.raises(png_parse.Unsupported, match="PNG_MAX_RAW"):
        dw.stage_png("-", 224, region, blob, interlaced=True)


def test_bindings_check_their_arguments_without_a_launch(clipmi):
    """Both entries refuse bad arguments before they look at a record, interlaced or not; the ABI version stays 8."""
    L = clipmi._lib.lib()
    assert L.clipmi_abi_version() == 8 and clipmi._lib.ABI_VERSION == 8
    fake = C.c_void_p(4096)
    EINVAL, EWORKSPACE = 1, 2
    for size_of, decode, who in ((L.clipmi_png_workspace_bytes, L.clipmi_png_decode_rgb8, "png_decode_rgb8"),
                                 (L.clipmi_png_px8_workspace_bytes, L.clipmi_png_decode_px8, "png_decode_px8")):
        need = size_of(4, 1 << 20)
        assert decode(fake, fake, 0, 1 << 20, 1 << 10, fake, fake, fake, need, None) == EINVAL
        for hole in range(5):
            ptrs = [fake] * 5
            ptrs[hole] = None
            rc = decode(ptrs[0], ptrs[1], 4, 1 << 20, 1 << 10, ptrs[2], ptrs[3], ptrs[4], need, None)
            assert rc == EINVAL and who in clipmi._lib.last_error()
        assert decode(fake, fake, 4, 1 << 20, (1 << 20) + 1, fake, fake, fake, need, None) == EINVAL
        assert decode(fake, fake, 4, 1 << 20, 0, fake, fake, fake, need, None) == EINVAL
        assert decode(C.c_void_p(4096), fake, 4, 1 << 20, 1 << 10, fake, fake, C.c_void_p(4100), need, None) == EINVAL      # workspace not 16-aligned
        rc = decode(fake, fake, 4, 1 << 20, 1 << 10, fake, fake, fake, need - 1, None)
        assert rc in (EINVAL, EWORKSPACE) and "workspace" in clipmi._lib.last_error()
    with pytest.raises(Exception, match="no CPU fallback"):
        png.decode_device([png_parse.parse(A.lace_file(np.random.default_rng(96), 2, 8, 3, 3), interlaced=True)], "cpu")
