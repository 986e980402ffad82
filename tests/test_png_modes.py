"""The host side of the device decode of alpha, palette and low-depth PNG files, without a GPU: png_parse.parse(modes=True)
against Pillow, its chunk rules, the CPU restatement of the decode and of the two transform rules (png_mode_cases) against
Pillow's own pixels and `decode_worker.load_uint8`, the new entry points' argument checks, and the worker's region layout."""
import ctypes as C
import io
import struct

import numpy as np
import pytest
from PIL import Image

from clipmi import decode_worker, png, png_parse
import png_cases
import png_mode_cases as M

pytestmark = pytest.mark.filterwarnings("ignore:Palette images with Transparency")


def _refused(blob, **kw):
    with pytest.raises(png_parse.Unsupported):
        png_parse.parse(blob, **kw)


def small_files(rng):
    """[(name, file)] of every new mode, from the writer and from Pillow's encoder, a few sizes each"""
    files = []
    k = 0
    for (ctype, depth) in M.MODES:
        for (h, w) in ((1, 1), (5, 7), (17, 9), (3, 33)):
            for t in ((False, True) if ctype == 3 else (False,)):
                files.append((f"w_c{ctype}d{depth}_{h}x{w}_t{int(t)}", M.mode_file(rng, ctype, depth, h, w, k, M.png_cases.MODES[k % 8],
                                                                                  with_trns=t, level=(0, 1, 6, 9)[k % 4])))
                k += 1
    for what in ("RGBA", "LA", "P1", "P2", "P4", "P8", "P8t", "P4t", "1"):
        for (h, w) in ((1, 1), (6, 5), (20, 33)):
            files.append((f"pillow_{what}_{h}x{w}", M.pillow_mode_file(rng, what, h, w, k)))
            k += 1
    return files


@pytest.fixture(scope="module")
def files():
    return small_files(np.random.default_rng(11))


def test_without_the_flag_every_new_mode_is_still_refused(files):
    assert len(files) >= 70
    for name, blob in files:
        _refused(blob)
        _refused(blob, modes=False)


def test_with_the_flag_size_kind_palette_and_samples_are_pillows(files):
    kinds = set()
    for name, blob in files:
        p = png_parse.parse(blob, modes=True)
        kind, ref = M.pillow_pixels(blob)
        assert p.kind == kind and (p.height, p.width) == ref.shape[:2], name
        assert (p.ctype, p.depth) in M.MODES and M.MODES[(p.ctype, p.depth)] == kind and p.channels == M.SAMPLES[p.ctype], name
        assert p.raw_bytes() == p.height * (1 + (p.width * p.channels * p.depth + 7) // 8), name
        if kind == "index":
            pal, n = M.pillow_palette(blob)
            assert p.n_entries == n and p.palette.dtype == np.uint8 and np.array_equal(p.palette, pal), name
        else:
            assert p.palette is None and p.n_entries == 0, name
        got = M.cpu_decode(p)
        assert got is not None and np.array_equal(got, ref), name
        kinds.add((p.ctype, p.depth))
    assert kinds == set(M.MODES)


def test_the_flag_changes_nothing_for_grey_and_rgb_files():
    rng = np.random.default_rng(12)
    for ch in (1, 3):
        blob = png_cases.write(png_cases.smooth(rng, 9, 11, ch), "cycle")
        a, b = png_parse.parse(blob), png_parse.parse(blob, modes=True)
        assert (a.kind, b.kind) == ("rgb", "rgb") and a.depth == 8 and a.ctype == (2 if ch == 3 else 0)
        assert (a.width, a.height, a.channels, a.stream) == (b.width, b.height, b.channels, b.stream)
        assert a.raw_bytes() == 9 * (1 + 11 * ch)
    trns = png_cases.write(png_cases.smooth(rng, 9, 11, 3), "cycle", before=png_cases.chunk(b"tRNS", b"\0\1\0\2\0\3"))
    _refused(trns, modes=True)                                  # tRNS on colour types 0 and 2 stays out of scope
    _refused(png_cases.write(png_cases.smooth(rng, 9, 11, 1), "cycle", before=png_cases.chunk(b"tRNS", b"\0\1")), modes=True)


def _index_file(rng, depth=4, entries=None, before=b"", after=b"", w=9, h=6):
    entries = (1 << depth) if entries is None else entries
    s = rng.integers(0, min(entries, 1 << depth), (h, w, 1), dtype=np.uint8)
    z = png_cases.deflate(M.scanlines(s, 3, depth, "cycle"))
    return png_cases.assemble(w, h, 1, z, before=before, after=after, depth=depth, ctype=3)


def _opens(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def test_chunk_rules():
    rng = np.random.default_rng(13)
    pal16 = rng.integers(0, 256, (16, 3), dtype=np.uint8)
    P, T = M.plte, M.trns
    ok = [_index_file(rng, before=P(pal16)), _index_file(rng, before=P(pal16) + T([1, 2, 3])), _index_file(rng, before=P(pal16) + T(range(16))),
          _index_file(rng, before=png_cases.chunk(b"gAMA", struct.pack(">I", 45455)) + P(pal16) + png_cases.chunk(b"bKGD", b"\1") + T([9])),
          _index_file(rng, entries=5, before=P(pal16[:5])), _index_file(rng, entries=1, before=P(pal16[:1]) + T([7])),
          _index_file(rng, depth=8, before=P(rng.integers(0, 256, (256, 3), dtype=np.uint8)) + T(range(256))),
          _index_file(rng, depth=1, before=P(pal16[:2])), _index_file(rng, depth=2, before=P(pal16[:4]) + T([0]))]
    for k, blob in enumerate(ok):
        p = png_parse.parse(blob, modes=True)
        ref = _opens(blob)                                         # tRNS changes no pixel of convert("RGB")
        assert p.kind == "index" and np.array_equal(p.palette[M.cpu_decode(p)], ref), k
    refused = {
        "no PLTE": _index_file(rng),
        "two PLTE": _index_file(rng, before=P(pal16) + P(pal16)),
        "PLTE not whole entries": _index_file(rng, before=png_cases.chunk(b"PLTE", pal16.tobytes()[:-1])),
        "empty PLTE": _index_file(rng, before=png_cases.chunk(b"PLTE", b"")),
        "PLTE of 257 entries": _index_file(rng, depth=8, before=png_cases.chunk(b"PLTE", bytes(771))),
        "PLTE beyond the depth": _index_file(rng, depth=2, before=P(pal16[:5])),
        "PLTE beyond depth 1": _index_file(rng, depth=1, before=P(pal16[:3])),
        "PLTE behind IDAT": _index_file(rng, after=P(pal16)),
        "PLTE in front and behind": _index_file(rng, before=P(pal16), after=P(pal16)),
        "tRNS in front of PLTE": _index_file(rng, before=T([1]) + P(pal16)),
        "tRNS without PLTE": _index_file(rng, before=T([1])),
        "tRNS longer than the palette": _index_file(rng, entries=5, before=P(pal16[:5]) + T(range(6))),
        "two tRNS": _index_file(rng, before=P(pal16) + T([1]) + T([2])),
        "tRNS behind IDAT": _index_file(rng, before=P(pal16), after=T([1])),
        "PLTE with a bad CRC": _index_file(rng, before=png_cases.chunk(b"PLTE", pal16.tobytes(), crc=5)),
        "iCCP": _index_file(rng, before=P(pal16) + png_cases.chunk(b"iCCP", b"x\0\0abc")),
        "hIST": _index_file(rng, before=P(pal16) + png_cases.chunk(b"hIST", bytes(32))),
        "eXIf behind IDAT": _index_file(rng, before=P(pal16), after=png_cases.chunk(b"eXIf", b"\0" * 6)),
    }
    for why, blob in refused.items():
        with pytest.raises(png_parse.Unsupported):
            png_parse.parse(blob, modes=True)
        pytest.raises(png_parse.Unsupported, png_parse.parse, blob)
    # PLTE and tRNS stay refused for every other colour type, 16-bit, Adam7 and APNG files for every one
    for ctype, depth in ((6, 8), (4, 8), (0, 4), (0, 1)):
        s, _ = M.samples_for(rng, ctype, depth, 6, 9)
        z = png_cases.deflate(M.scanlines(s, ctype, depth))
        good = png_cases.assemble(9, 6, 1, z, depth=depth, ctype=ctype)
        assert png_parse.parse(good, modes=True).kind == M.MODES[(ctype, depth)]
        _opens(good)
        for before in (P(pal16[:2]), T([0, 1]), T([0, 1, 0, 2, 0, 3])):
            _refused(png_cases.assemble(9, 6, 1, z, before=before, depth=depth, ctype=ctype), modes=True)
        for after in (P(pal16[:2]), T([0, 1])):
            _refused(png_cases.assemble(9, 6, 1, z, after=after, depth=depth, ctype=ctype), modes=True)
        _refused(png_cases.assemble(9, 6, 1, z, depth=depth, ctype=ctype, lace=1), modes=True)
        _refused(png_cases.assemble(9, 6, 1, z, depth=16, ctype=ctype), modes=True)
    for ctype, depth in ((6, 4), (4, 4), (6, 1), (2, 4), (3, 16), (0, 3), (3, 3), (5, 8), (1, 8), (7, 8)):    # no such PNG file
        _refused(png_cases.assemble(9, 6, 1, b"\x78\x01" + bytes(20), depth=depth, ctype=ctype, before=P(pal16[:2]) if ctype == 3 else b""), modes=True)
    rgba = Image.fromarray(png_cases.noise(rng, 8, 8, 4), "RGBA")
    apng = M.save(rgba, save_all=True, append_images=[rgba.rotate(90)])
    assert Image.open(io.BytesIO(apng)).is_animated
    _refused(apng, modes=True)
    sixteen = M.save(Image.fromarray(rng.integers(0, 65536, (8, 8)).astype(np.uint16)))
    _refused(sixteen, modes=True)


def test_width_cap_is_the_unfilter_kernels_lds_row():
    """Row bytes without the filter byte <= 49152: RGBA up to 12288 pixels; MAX_WIDTH for every other mode"""
    assert png_parse.MAX_ROW_BYTES == 49152
    z = b"\x78\x01" + bytes(16)
    for ctype, depth, widest in ((6, 8, 12288), (4, 8, png_parse.MAX_WIDTH), (3, 8, png_parse.MAX_WIDTH), (3, 1, png_parse.MAX_WIDTH),
                                 (0, 2, png_parse.MAX_WIDTH)):
        before = M.plte(np.zeros((2, 3), np.uint8)) if ctype == 3 else b""
        p = png_parse.parse(png_cases.assemble(widest, 1, 1, z, depth=depth, ctype=ctype, before=before), modes=True)
        assert p.width == widest and p.row_bytes() <= 49152
        _refused(png_cases.assemble(widest + 1, 1, 1, z, depth=depth, ctype=ctype, before=before), modes=True)


@pytest.fixture(scope="module")
def transform_files():
    cases = M.transform_cases(np.random.default_rng(21))
    return [(name, blob) for name, blob in cases if not name.startswith(M.OLD)]


def test_cpu_restatement_of_the_transform_equals_load_uint8(transform_files):
    """The two rules (premultiplied bicubic for alpha, nearest with Pillow's accumulated float64 coordinate for index images) on
    top of decode_worker.resize_plan against the reference's transform itself, every size x every kind, n_px 32 and 224."""
    assert len(transform_files) == len(M.SIZES) * len(M.KINDS)
    checked = 0
    for name, blob in transform_files:
        p = png_parse.parse(blob, modes=True)
        px = M.cpu_decode(p)
        for n_px in (32, 224):
            assert np.array_equal(M.cpu_transform(p, n_px, px), M.load_uint8_blob(blob, n_px)), (name, n_px)
            checked += 1
    assert checked == 2 * len(M.SIZES) * len(M.KINDS)


def test_nearest_tables_are_pillows_columns_and_rows():
    """nearest_window against Pillow's NEAREST resize of an image whose pixel value is its own coordinate, sizes where
    multiplication and accumulation of the step differ in the last bit"""
    differs = 0
    for in_size, out_size in ((5, 224), (200, 32), (37, 70), (70, 37), (640, 298), (230, 224), (1000, 999), (255, 254), (3, 7), (241, 77)):
        row = (np.arange(in_size) % 251).astype(np.uint8)
        got = decode_worker.nearest_window(in_size, out_size, 0, out_size)
        ref = np.asarray(Image.fromarray(np.tile(row, (2, 1)), "P").resize((out_size, 2), Image.BICUBIC))[0]
        assert np.array_equal(row[got], ref), (in_size, out_size)
        col = np.asarray(Image.fromarray(np.tile(row[:, None], (1, 2)), "P").resize((2, out_size), Image.BICUBIC))[:, 0]
        assert np.array_equal(row[got], col), (in_size, out_size)
        mult = ((np.arange(out_size) + 0.5) * (in_size / out_size)).astype(np.int64)
        differs += int((mult != got).any())
        assert np.array_equal(decode_worker.nearest_window(in_size, out_size, 3, min(5, out_size - 3)), got[3:8][:min(5, out_size - 3)])
    print("sizes where multiplying instead of accumulating picks another pixel:", differs)


def test_pack_carries_mode_and_sizes_per_kind():
    rng = np.random.default_rng(14)
    blobs = [M.mode_file(rng, 6, 8, 5, 7), M.mode_file(rng, 4, 8, 6, 3), M.mode_file(rng, 3, 2, 9, 9, entries=3), M.mode_file(rng, 0, 4, 4, 5),
             M.mode_file(rng, 0, 1, 3, 10)]
    items = [png_parse.parse(b, modes=True) for b in blobs]
    recs, streams, out_bytes, total_raw, max_raw = png.pack(items)
    assert [int(r["reserved"][0]) for r in recs] == [6 << 8 | 8, 4 << 8 | 8, 3 << 8 | 2, 4, 1]
    assert [int(r["reserved"][1]) for r in recs] == [0, 0, 3, 0, 2] and list(recs["channels"]) == [4, 2, 1, 1, 1]
    sizes = [5 * 7 * 4, 6 * 3 * 4, 81, 4 * 5 * 4, 30]
    assert out_bytes == sum((s + 15) // 16 * 16 for s in sizes)
    raws = [5 * 29, 6 * 7, 9 * 4, 4 * 4, 3 * 3]
    assert [it.raw_bytes() for it in items] == raws and max_raw == max(raws) and total_raw == sum((r + 15) // 16 * 16 for r in raws)
    with pytest.raises(ValueError):
        png.decode_device([items[0], png_parse.parse(png_cases.write(png_cases.noise(rng, 3, 3)))], "cuda:0")
    with pytest.raises(Exception, match="no CPU fallback"):
        png.decode_device(items, "cpu")


def test_new_bindings_check_their_arguments_without_a_launch(clipmi):
    L = clipmi._lib.lib()
    for name in ("clipmi_png_px8_workspace_bytes", "clipmi_png_decode_px8", "clipmi_resize_crop_rgba8", "clipmi_nearest_crop_p8"):
        assert hasattr(L, name) and name in clipmi._lib.SYMBOLS
    assert L.clipmi_abi_version() == 8
    need = L.clipmi_png_px8_workspace_bytes(4, 1 << 20)
    assert need == L.clipmi_png_workspace_bytes(4, 1 << 20) and L.clipmi_png_px8_workspace_bytes(-1, 16) < 0
    fake = C.c_void_p(4096)
    EINVAL, EWORKSPACE = 1, 2
    assert L.clipmi_png_decode_px8(fake, fake, 0, 1 << 20, 1 << 10, fake, fake, fake, need, None) == EINVAL
    for hole in range(5):
        ptrs = [fake] * 5
        ptrs[hole] = None
        rc = L.clipmi_png_decode_px8(ptrs[0], ptrs[1], 4, 1 << 20, 1 << 10, ptrs[2], ptrs[3], ptrs[4], need, None)
        assert rc == EINVAL and "png_decode_px8" in clipmi._lib.last_error()
    rc = L.clipmi_png_decode_px8(fake, fake, 4, 1 << 20, 1 << 10, fake, fake, fake, need - 1, None)
    assert rc in (EINVAL, EWORKSPACE) and "workspace" in clipmi._lib.last_error()
    assert L.clipmi_resize_crop_rgba8(fake, fake, 0, 1, fake, 224, fake, fake, None) == 0          # no jobs: nothing to do
    assert L.clipmi_resize_crop_rgba8(None, fake, 2, 1, fake, 224, fake, fake, None) == EINVAL
    assert L.clipmi_resize_crop_rgba8(fake, fake, 2, 0, fake, 224, fake, fake, None) == EINVAL
    assert "resize_crop_rgba8" in clipmi._lib.last_error()
    assert L.clipmi_nearest_crop_p8(fake, fake, 0, fake, 224, fake, None) == 0
    assert L.clipmi_nearest_crop_p8(fake, None, 2, fake, 224, fake, None) == EINVAL
    assert L.clipmi_nearest_crop_p8(fake, fake, 2, C.c_void_p(4097), 224, fake, None) == EINVAL
    assert L.clipmi_nearest_crop_p8(fake, fake, 2, fake, 0, fake, None) == EINVAL and "nearest_crop_p8" in clipmi._lib.last_error()


def test_stage_png_region_layout_with_the_bit_on_and_off(tmp_path):
    rng = np.random.default_rng(15)
    dw = decode_worker
    kinds = {k.kind: k for k in dw.PARSED}
    assert (dw.KIND_PNG_ALPHA, dw.KIND_PNG_INDEX) == (7, 8)
    for kind in (7, 8):
        assert (kinds[kind].bit, kinds[kind].magic, kinds[kind].stat, kinds[kind].counts) == (16, "png", "png_mode_files", "decoded")
    assert kinds[dw.KIND_PNG].stager is dw.stage_png and kinds[dw.KIND_PNG].bit == 8 and b"7" in dw.REGION_TAGS and b"8" in dw.REGION_TAGS
    n_px = 224
    for k, (ctype, depth, h, w, t) in enumerate([(6, 8, 300, 260, False), (4, 8, 224, 224, False), (3, 4, 70, 37, True), (3, 8, 225, 223, False),
                                                 (0, 1, 40, 300, False), (0, 2, 230, 500, False)]):
        blob = M.mode_file(rng, ctype, depth, h, w, k, with_trns=t)
        path = tmp_path / f"f{k}.png"
        path.write_bytes(blob)
        p = png_parse.parse(blob, modes=True)
        region = np.full(1 << 20, 0xAB, np.uint8)
        with pytest.raises(png_parse.Unsupported):             # the bit off: as ever
            dw.stage_png(str(path), n_px, region)
        assert (region == 0xAB).all()
        got = dw.stage_png(str(path), n_px, region, modes=True)
        assert got[:2] == (w, h) and 0 < got[2] <= region.size and got[2] % 16 == 0
        want_kind = dw.KIND_PNG_INDEX if p.kind == "index" else dw.KIND_PNG_ALPHA
        # the stager of the file's own kind lays out the same region; the other one leaves the file alone
        other = np.full(1 << 20, 0xAB, np.uint8)
        assert kinds[want_kind].stager(str(path), n_px, other, blob) == got and np.array_equal(other, region)
        with pytest.raises(png_parse.Unsupported):
            kinds[15 - want_kind].stager(str(path), n_px, other, blob)
        ints = np.frombuffer(region, np.int32, count=dw.JPEG_HDR_INTS)
        assert list(ints[:8]) == [want_kind, w, h, p.channels, 0, 0, len(p.stream), 0]
        assert (ints[dw.HDR.DEPTH], ints[dw.HDR.CTYPE], ints[dw.HDR.ENTRIES]) == (depth, ctype, p.n_entries) and not ints[23:].any()
        plan = dw.nearest_plan(w, h, n_px) if p.kind == "index" else dw.resize_plan(w, h, n_px)
        assert list(ints[8:18]) == [plan["r0"], plan["nrows"], plan["need_h"], plan["need_v"], plan["left"], plan["top"], plan["hk"],
                                    plan["vk"], plan["hcoef"].size, plan["vcoef"].size]
        o_stream, o_coef = int(ints[18]), int(ints[19])
        assert o_stream % 16 == 0 and o_coef == dw.JPEG_COEF_OFF
        nh, nv = plan["hcoef"].size, plan["vcoef"].size
        co = np.frombuffer(region, np.int32, count=nh + nv, offset=o_coef)
        assert np.array_equal(co[:nh], plan["hcoef"]) and np.array_equal(co[nh:], plan["vcoef"])
        if p.kind == "index":
            assert (nh, nv) == (n_px, n_px) and 0 <= co[:nh].min() and co[:nh].max() < w and 0 <= co[nh:].min() and co[nh:].max() < h
            assert plan["r0"] == co[nh:].min() and plan["r0"] + plan["nrows"] - 1 == co[nh:].max()
            assert np.array_equal(region[dw.JPEG_TABLES_OFF:dw.JPEG_TABLES_OFF + 768], p.palette.reshape(-1))
            assert dw.JPEG_TABLES_OFF + 768 <= dw.JPEG_COEF_OFF
        assert bytes(region[o_stream:o_stream + len(p.stream)]) == p.stream
        assert got[2] >= o_stream + len(p.stream) + 16 and not region[o_stream + len(p.stream):got[2]].any() and region[got[2]] == 0xAB
        assert dw.stage_png(str(path), n_px, np.zeros(o_stream + 8, np.uint8), modes=True) == (w, h, -got[2])
    rgb = tmp_path / "rgb.png"
    rgb.write_bytes(png_cases.write(png_cases.smooth(rng, 40, 30, 3), "cycle"))
    a, b = np.zeros(1 << 16, np.uint8), np.zeros(1 << 16, np.uint8)
    assert dw.stage_png(str(rgb), n_px, a) == dw.stage_png(str(rgb), n_px, b, modes=True) and np.array_equal(a, b) and a[0] == dw.KIND_PNG
    for kind in (7, 8):                                            # a grey / RGB file is KIND_PNG's, whatever the request allows
        with pytest.raises(png_parse.Unsupported):
            kinds[kind].stager(str(rgb), n_px, a)


def test_records_the_parent_builds_from_the_regions(tmp_path):
    """device_stage._FORMATS' records for the two new kinds, out of a batch's regions: field for field png.pack's, the jobs resize_plan's
    or the nearest tables' where the regions hold them"""
    from clipmi import device_stage
    dw = decode_worker
    rng = np.random.default_rng(16)
    n_px, cap = 224, 256 << 10
    for kind, px, specs in ((dw.KIND_PNG_ALPHA, 4, [(6, 8, 64, 96), (4, 8, 260, 300), (0, 4, 224, 224), (0, 2, 300, 260)]),
                            (dw.KIND_PNG_INDEX, 1, [(3, 8, 64, 96), (3, 1, 260, 300), (0, 1, 224, 224), (3, 4, 300, 260)])):
        n = len(specs) + 2
        big = np.full(n * cap, 0xAB, np.uint8)
        slots, items = [], []
        for k, (ctype, depth, h, w) in enumerate(specs):
            blob = M.mode_file(rng, ctype, depth, h, w, k)
            path = tmp_path / f"k{kind}_{k}.png"
            path.write_bytes(blob)
            slot = k + (1 if k >= 2 else 0)
            assert 0 < dw.stage_png(str(path), n_px, big[slot * cap:(slot + 1) * cap], modes=True)[2] <= cap
            slots.append(slot)
            items.append(png_parse.parse(blob, modes=True))
        records, decoder_bytes, group, fpx, entry = device_stage._FORMATS[kind]
        assert fpx == px and entry == ("clipmi_nearest_crop_p8" if px == 1 else "clipmi_resize_crop_rgba8")
        recs, jobs, out_sz, raw_sz = records(big, n, cap, slots, np.arange(n), n_px)
        ref = png.pack(items)[0]
        for f in ("stream_bytes", "width", "height", "channels", "raw_off", "out_off", "reserved"):
            assert np.array_equal(recs[f], ref[f]), f
        hd = device_stage._headers(big, n, cap, np.asarray(slots))
        assert list(decoder_bytes(hd)) == [it.raw_bytes() for it in items]
        assert list(out_sz) == [(it.width * it.height * px + 15) // 16 * 16 for it in items]
        assert list(raw_sz) == [(it.raw_bytes() + 15) // 16 * 16 for it in items]
        for k, (r, it, slot) in enumerate(zip(recs, items, slots)):
            o, nb = int(r["stream_off"]), int(r["stream_bytes"])
            assert slot * cap <= o and o + nb + 16 <= (slot + 1) * cap and big[o:o + nb].tobytes() == it.stream
            j = jobs[k]
            assert int(j["src_off"]) == int(r["out_off"]) and int(j["out_index"]) == slot and (int(j["w"]), int(j["h"])) == (it.width, it.height)
            if px == 1:
                plan = dw.nearest_plan(it.width, it.height, n_px)
                assert np.array_equal(np.frombuffer(big, np.int32, count=n_px, offset=4 * int(j["col_off"])), plan["hcoef"])
                assert np.array_equal(np.frombuffer(big, np.int32, count=n_px, offset=4 * int(j["row_off"])), plan["vcoef"])
                assert np.array_equal(big[int(j["pal_off"]):int(j["pal_off"]) + 768], it.palette.reshape(-1))
            else:
                plan = dw.resize_plan(it.width, it.height, n_px)
                assert (int(j["r0"]), int(j["nrows"]), int(j["need_h"]), int(j["need_v"]), int(j["left"]), int(j["top"]), int(j["hk"]),
                        int(j["vk"])) == (plan["r0"], plan["nrows"], plan["need_h"], plan["need_v"], plan["left"], plan["top"], plan["hk"], plan["vk"])
                hc = np.frombuffer(big, np.int32, count=plan["hcoef"].size, offset=4 * int(j["hcoef_off"]))
                vc = np.frombuffer(big, np.int32, count=plan["vcoef"].size, offset=4 * int(j["vcoef_off"]))
                assert np.array_equal(hc, plan["hcoef"]) and np.array_equal(vc, plan["vcoef"])
        if px == 4:
            tmp = jobs["nrows"].astype(np.int64) * n_px * 4
            assert np.array_equal(jobs["tmp_off"], np.cumsum(tmp) - tmp)
