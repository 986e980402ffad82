"""Four-component JPEG files on the host side of the device path (no GPU here): jpeg_parse.parse(cmyk=True) against Pillow, the forged
forms of tests/jpeg_cmyk.py pinned against Pillow alone, the numpy restatement of the pixel rules, jpeg.pack's guards and record,
decode_worker.stage_jpeg_cmyk's regions and the records device_stage builds from them, and the committed fixture against Pillow live."""
import io
import os
import subprocess
import warnings

import numpy as np
import pytest
from PIL import Image

import jpeg_cmyk as jc
from clipmi import decode_worker, jpeg_parse
from clipmi.decode_worker import load_uint8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_cmyk_cases.npz")
Unsupported = jpeg_parse.Unsupported


@pytest.fixture(scope="module")
def cases():
    return jc.cases()


def _dqt(blob):
    """{table id: 64 steps in zigzag order} and the frame header's selector per component, read off the file"""
    tabs, sel = {}, None
    for m, i, n in jc._segments(blob):
        if m == 0xDB:
            k = i + 4
            while k < i + n:
                tabs[blob[k] & 15] = np.frombuffer(blob[k + 1:k + 65], np.uint8)
                k += 65
        elif m in (0xC0, 0xC1):
            sel = [blob[i + 12 + 3 * c] for c in range(blob[i + 9])]
    return tabs, sel


def test_parser_against_pillow(cases):
    assert len(cases) == (4 + 2 + 2) * len(jc.FORMS)
    seen = set()
    for name, blob, (hs, vs), tf, H, W in cases:
        for ks in (False, True):
            p = jpeg_parse.parse(blob, keep_stuffing=ks, cmyk=True)
            assert (p.ncomp, p.hs, p.vs, p.transform, p.height, p.width) == (4, hs, vs, tf, H, W), name
            assert p.blocks() == p.mcus() * (hs * vs + 3) and p.mcus() == -(-W // (8 * hs)) * -(-H // (8 * vs)), name
            assert len(p.tables) == 8 and p.quant.shape == (4, 64), name
        tabs, sel = _dqt(blob)
        for c in range(4):                                  # the step rows as written, natural order
            assert np.array_equal(p.quant[c][jpeg_parse._NATURAL], tabs[sel[c]]), (name, c)
        form = name.split()[0]
        assert (len(set(sel)) == 2) == (form == "two_quant"), name
        assert (len(set(p.tables)) == 4) == (form == "two_huffman") and len(set(p.tables)) in (2, 4), name
        assert (p.ri == 3) == (form == "restart"), name
        assert Image.open(io.BytesIO(blob)).mode == "CMYK", name
        for layouts in (False, True):
            with pytest.raises(Unsupported):
                jpeg_parse.parse(blob, layouts=layouts)
            assert jpeg_parse.parse(blob, layouts=layouts, cmyk=True).ncomp == 4
        seen.add((form, hs, vs, tf))
    assert {s[3] for s in seen} == {jc.CMYK, jc.YCCK} and len(seen) == 3 * len(jc.FORMS)


def test_what_stays_with_pillow():
    rng = np.random.default_rng(3)
    a = jc.smooth4(rng, 45, 37)
    b = jc.cmyk_file(a, subsampling=2)
    assert jpeg_parse.parse(jc.with_adobe_transform(b, 2), cmyk=True).transform == jc.YCCK
    for label, bad in (("Adobe transform 1", jc.with_adobe_transform(b, 1)), ("Adobe transform 3", jc.with_adobe_transform(b, 3)),
                       ("progressive", jc.cmyk_file(a, subsampling=2, progressive=True)),
                       ("2x2,1x1,1x1,2x2", jc.like_ijg_ycck(b)),
                       ("component 2 sampled 2x1", jc.relabel(b, luma=0x21, comp=2))):
        with pytest.raises(Unsupported):
            jpeg_parse.parse(bad, cmyk=True)
        with pytest.raises(Unsupported):
            jpeg_parse.parse(bad, cmyk=True, layouts=True)
    with pytest.raises(Unsupported):
        jpeg_parse.parse_progressive(jc.cmyk_file(a, subsampling=2, progressive=True), layouts=True)
    # the narrow rule: 2x sampling below width 5
    for sub in (1, 2):
        for W in (1, 2, 3, 4):
            with pytest.raises(Unsupported, match="narrow"):
                jpeg_parse.parse(jc.cmyk_file(jc.smooth4(rng, 9, W), subsampling=sub), cmyk=True)
        assert jpeg_parse.parse(jc.cmyk_file(jc.smooth4(rng, 9, 5), subsampling=sub), cmyk=True).width == 5
    assert jpeg_parse.parse(jc.cmyk_file(jc.smooth4(rng, 9, 2), subsampling=0), cmyk=True).width == 2
    # component 0 at one of the layouts' samplings: only with both switches
    tall = jc.relabel(jc.cmyk_file(jc.smooth4(rng, 24, 40), subsampling=1), luma=0x12, width=24, height=40)
    with pytest.raises(Unsupported):
        jpeg_parse.parse(tall, cmyk=True)
    p = jpeg_parse.parse(tall, cmyk=True, layouts=True)
    assert (p.hs, p.vs, p.ncomp) == (1, 2, 4) and jpeg_parse.is_layout(p)
    # a JFIF marker plays no part
    jfif = b[:2] + b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00" + b[2:]
    assert jpeg_parse.parse(jfif, cmyk=True).transform == jc.CMYK and jpeg_parse.parse(jc.as_ycck(jfif), cmyk=True).transform == jc.YCCK


def test_three_component_and_grey_files_parse_the_same_with_the_keyword():
    rng = np.random.default_rng(4)
    for blob in (jc.encode(jc.smooth(rng, 33, 47), quality=85, subsampling=2), jc.encode(jc.smooth(rng, 20, 31), quality=70, subsampling=0),
                 jc.encode(jc.smooth(rng, 24, 40), quality=85, subsampling=1, restart_marker_blocks=2), jc.encode(jc.smooth(rng, 30, 26)[..., 0])):
        for ks in (False, True):
            a, b = jpeg_parse.parse(blob, keep_stuffing=ks), jpeg_parse.parse(blob, keep_stuffing=ks, cmyk=True)
            for f in jpeg_parse.Parsed.__slots__:
                x, y = getattr(a, f), getattr(b, f)
                assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, f
            assert a.quant.shape == (3, 64) and len(a.tables) == 6 and not jpeg_parse.is_layout(a)


def test_the_forge_helpers_are_pinned_against_pillow_alone():
    rng = np.random.default_rng(5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for sub in (0, 1, 2):
            a = jc.smooth4(rng, 45, 37)
            for q in (30, 95):
                b = jc.cmyk_file(a, subsampling=sub, quality=q, optimize=True)
                th = jc.two_huffman(b)
                assert th != b and np.array_equal(jc.pillow4(th), jc.pillow4(b))
                huff = {}
                for m, i, n in jc._segments(th):
                    if m == 0xC4:
                        jpeg_parse._dht(th, i + 4, i + n, huff)
                assert sorted(huff) == [0x00, 0x01, 0x10, 0x11]
                assert jc.pillow4(jc.as_ycck(b)).shape == (45, 37, 4) and not np.array_equal(jc.pillow4(jc.as_ycck(b)), jc.pillow4(b))
                assert jc.pillow4(jc.two_quant(a, subsampling=sub, quality=q)).shape == (45, 37, 4)
                assert np.array_equal(jc.pillow4(jc.without_adobe(b)), jc.pillow4(b))


def test_the_restatement_of_the_pixel_rules_against_pillow(cases):
    """planes -> Pillow's CMYK bytes for both transforms, and cmyk2rgb. The planes come from the file's CMYK form, whose pixels are
    the inverted planes; the same planes under Adobe transform 2 must give the YCCK form's pixels."""
    rng = np.random.default_rng(6)
    for sub in (0, 1, 2):
        for H, W in jc.SIZES if sub == 0 else jc.SIZES[2:]:
            for kw in ({}, dict(restart_marker_blocks=3), dict(optimize=True)):
                b = jc.cmyk_file(jc.smooth4(rng, H, W), subsampling=sub, **kw)
                planes = (255 - jc.pillow4(b).astype(np.int32)).transpose(2, 0, 1)
                assert np.array_equal(jc.planes_to_cmyk(planes, jc.CMYK), jc.pillow4(b))
                assert np.array_equal(jc.planes_to_cmyk(planes, jc.CMYK), jc.pillow4(jc.without_adobe(b)))
                assert np.array_equal(jc.planes_to_cmyk(planes, jc.YCCK), jc.pillow4(jc.as_ycck(b)))
    for name, blob, _, _, _, _ in cases:
        assert np.array_equal(jc.cmyk2rgb(jc.pillow4(blob)), jc.pillow(blob)), name
    every = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), -1).reshape(256, 256, 2)
    px = np.concatenate([every[..., :1], every[..., :1], 255 - every[..., :1], every[..., 1:]], -1).astype(np.uint8)      # every (c, K) pair
    assert np.array_equal(jc.cmyk2rgb(px), np.asarray(Image.fromarray(px, "CMYK").convert("RGB")))


def test_the_transform_resamples_in_mode_cmyk_band_by_band(tmp_path):
    """load_uint8 of a four-component file = four plain bands resampled and cropped, then cmyk2rgb (no premultiplication)"""
    rng = np.random.default_rng(7)
    for k, (H, W) in enumerate([(40, 33), (33, 50), (32, 32)]):
        b = jc.as_ycck(jc.cmyk_file(jc.smooth4(rng, H, W), subsampling=2)) if k == 1 else jc.cmyk_file(jc.smooth4(rng, H, W), subsampling=k)
        path = tmp_path / f"{k}.jpg"
        path.write_bytes(b)
        px = jc.pillow4(b)
        bands = np.stack([load_uint8_band(px[..., c], 32) for c in range(4)], -1)
        assert np.array_equal(load_uint8(str(path), 32), jc.cmyk2rgb(bands).transpose(2, 0, 1))


def load_uint8_band(band, n_px):
    """decode_worker.load_uint8's geometry on one 8-bit band"""
    img = Image.fromarray(np.ascontiguousarray(band), "L")
    w, h = img.size
    if not (w <= h and w == n_px) and not (h <= w and h == n_px):
        nw, nh = (n_px, int(n_px * h / w)) if w <= h else (int(n_px * w / h), n_px)
        img = img.resize((nw, nh), Image.BICUBIC)
        w, h = nw, nh
    left, top = int(round((w - n_px) / 2.0)), int(round((h - n_px) / 2.0))
    return np.asarray(img.crop((left, top, left + n_px, top + n_px)))


def test_pack_guards_and_the_four_component_record(clipmi):
    from clipmi import jpeg
    rng = np.random.default_rng(8)
    four = [jpeg_parse.parse(jc.cmyk_file(jc.smooth4(rng, 17, 33), subsampling=s), cmyk=True) for s in (0, 1, 2)]
    four.append(jpeg_parse.parse(jc.as_ycck(jc.cmyk_file(jc.smooth4(rng, 45, 37), subsampling=2, restart_marker_blocks=3)), cmyk=True))
    three = jpeg_parse.parse(jc.encode(jc.smooth(rng, 33, 47), quality=85, subsampling=2))
    with pytest.raises(Unsupported, match="cmyk=True"):
        jpeg.pack(four)
    with pytest.raises(Unsupported, match="cmyk=True"):
        jpeg.pack(four, layouts=True)
    with pytest.raises(Unsupported, match="one batch"):
        jpeg.pack(four + [three], cmyk=True)
    assert jpeg.pack([three], cmyk=True)[0].dtype == jpeg.IMAGE            # the keyword alone changes nothing for other records
    recs, tables, streams, out_bytes, total, most, pixels = jpeg.pack(four, cmyk=True)
    assert recs.dtype == jpeg.IMAGE4 and len(recs) == 4 and tables.shape[1] == jpeg_parse.TABLE_BYTES
    sizes = [(it.width * it.height * 4 + 15) // 16 * 16 for it in four]
    assert out_bytes == sum(sizes) and list(recs["out_off"]) == list(np.cumsum(sizes) - sizes)
    assert total == sum(it.blocks() for it in four) and most == max(it.blocks() for it in four) and pixels == 45 * 37
    assert list(recs["coef_off"]) == list(np.cumsum([it.blocks() for it in four]) - [it.blocks() for it in four])
    for r, it in zip(recs, four):
        assert (r["ncomp"], r["hs"], r["vs"], r["reserved"], r["width"], r["height"]) == (4, it.hs, it.vs, it.transform, it.width, it.height)
        assert np.array_equal(r["quant"], it.quant) and r["quant"].shape == (4, 64)
        assert [tables[i].tobytes() for i in r["dc_tbl"]] == it.tables[0::2] and [tables[i].tobytes() for i in r["ac_tbl"]] == it.tables[1::2]
        assert streams[r["stream_off"]:r["stream_off"] + r["stream_bytes"]].tobytes() == bytes(it.stream)
    assert recs[3]["restart_interval"] == 3 and recs[3]["n_intervals"] == len(four[3].starts) and list(recs["reserved"]) == [2, 2, 2, 3]
    with pytest.raises(Exception, match="no CPU fallback"):
        jpeg.decode_device(four, "cpu", cmyk=True)


def test_image4_is_the_headers_record_and_the_entries_check_their_arguments(clipmi, tmp_path):
    import ctypes as C
    from clipmi import jpeg
    src = tmp_path / "t.c"
    fields = list(jpeg.IMAGE4.names)
    body = "\n".join(f'printf("{f} %zu\\n", offsetof(clipmi_jpeg_image4, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipmi.h"\nint main(){'
                   'printf("sizeof %zu\\n", sizeof(clipmi_jpeg_image4));printf("sizeof3 %zu\\n", sizeof(clipmi_jpeg_image));' + body + 'return 0;}')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["sizeof"]) == jpeg.IMAGE4.itemsize == 360 and int(out["sizeof3"]) == jpeg.IMAGE.itemsize
    for f in fields:
        assert int(out[f]) == jpeg.IMAGE4.fields[f][1], f
    L = clipmi._lib.lib()
    for name in ("clipmi_jpeg_decode_cmyk8", "clipmi_resize_crop_cmyk8"):
        assert hasattr(L, name) and name in clipmi._lib.SYMBOLS
    assert L.clipmi_abi_version() == 8
    fake = C.c_void_p(4096)
    EINVAL = 1
    need = L.clipmi_jpeg_workspace_bytes(100, 8)
    assert L.clipmi_jpeg_decode_cmyk8(fake, fake, 0, fake, 8, 100, 50, 400, fake, fake, fake, need, None) == 0      # no images: nothing to do
    for hole in range(6):
        ptrs = [fake] * 6
        ptrs[hole] = None
        rc = L.clipmi_jpeg_decode_cmyk8(ptrs[0], ptrs[1], 2, ptrs[2], 8, 100, 50, 400, ptrs[3], ptrs[4], ptrs[5], need, None)
        assert rc == EINVAL and "jpeg_decode_cmyk8" in clipmi._lib.last_error()
    assert L.clipmi_jpeg_decode_cmyk8(fake, fake, 2, fake, 8, 100, 50, 400, fake, fake, fake, need - 1, None) != 0
    assert "workspace" in clipmi._lib.last_error()
    assert L.clipmi_resize_crop_cmyk8(fake, fake, 0, 1, fake, 224, fake, fake, None) == 0
    assert L.clipmi_resize_crop_cmyk8(None, fake, 2, 1, fake, 224, fake, fake, None) == EINVAL
    assert L.clipmi_resize_crop_cmyk8(fake, fake, 2, 0, fake, 224, fake, fake, None) == EINVAL
    assert "resize_crop_cmyk8" in clipmi._lib.last_error()


def test_the_new_kind_stands_beside_the_five(clipmi):
    from clipmi import device_stage
    dw = decode_worker
    assert [k.kind for k in dw.PARSED] == [3, 4, 6, 7, 8] and dw.ALL_PARSED == dw.PARSED + dw.PARSED_MORE
    (k,) = dw.PARSED_MORE
    assert (k.kind, k.bit, k.magic, k.stager, k.stat, k.counts) == (9, 128, "jpeg", dw.stage_jpeg_cmyk, "jpeg_cmyk_files", "staged")
    assert dw.KIND_JPEG_CMYK == 9 and b"9" in dw.REGION_TAGS and 9 in dw.PARSED_KINDS and dw.WANTED_TAG not in dw.REGION_TAGS
    bits = {p.bit for p in dw.ALL_PARSED}
    assert not bits & {dw.LAYOUTS_BIT, dw.PNG_INTERLACED_BIT, dw.FULL_SIZE.bit} and dw.LAYOUTS_BIT != dw.PNG_INTERLACED_BIT
    assert len({p.kind for p in dw.ALL_PARSED}) == len(dw.ALL_PARSED) and dw.FULL_SIZE.kind not in dw.PARSED_KINDS
    for fused in (False, True):
        assert set(device_stage.formats(fused)) == {p.kind for p in dw.PARSED}
        every = device_stage.all_formats(fused)
        assert set(every) == {p.kind for p in dw.ALL_PARSED}
        assert all(every[kind] is device_stage.formats(fused)[kind] for kind in device_stage.formats(fused))
        fmt = every[9]
        assert (fmt.px, fmt.tmp_px, fmt.entry) == (4, 4, "clipmi_resize_crop_cmyk8")
    # the regions' parts do not overlap
    assert dw.CMYK_QUANT_OFF >= 4 * dw.JPEG_HDR_INTS and dw.CMYK_TABLES_OFF >= dw.CMYK_QUANT_OFF + 256
    assert dw.CMYK_COEF_OFF >= dw.CMYK_TABLES_OFF + 8 * jpeg_parse.TABLE_BYTES and dw.CMYK_COEF_OFF % 16 == 0
    assert (dw.JPEG_QUANT_OFF, dw.JPEG_TABLES_OFF, dw.JPEG_COEF_OFF) == (128, 320, 2048)


def test_stage_jpeg_cmyk_regions_and_the_records_built_from_them(clipmi, tmp_path):
    """stage_jpeg_cmyk into regions of a segment -> records field for field jpeg.pack(..., cmyk=True)'s, jobs resize_plan's"""
    from clipmi import device_stage, jpeg
    dw = decode_worker
    rng = np.random.default_rng(9)
    n_px, cap = 224, 256 << 10
    specs = [("cmyk", 2, 300, 260), ("ycck", 0, 64, 96), ("restart", 1, 224, 224), ("two_huffman", 2, 45, 37), ("two_quant", 1, 250, 224)]
    n = len(specs) + 2
    big = np.full(n * cap, 0xAB, np.uint8)
    slots, items = [], []
    three = tmp_path / "three.jpg"
    three.write_bytes(jc.encode(jc.smooth(rng, 40, 30), quality=85, subsampling=2))
    for k, (form, sub, H, W) in enumerate(specs):
        blob, tf = jc.form_file(jc.smooth4(rng, H, W), sub, form)
        path = tmp_path / f"{k}.jpg"
        path.write_bytes(blob)
        slot = k + (1 if k >= 2 else 0)
        region = big[slot * cap:(slot + 1) * cap]
        with pytest.raises(Unsupported):                       # a four-component file is not stage_jpeg's, with any switch
            dw.stage_jpeg(str(path), n_px, region, layouts=True)
        assert (region == 0xAB).all()
        got = dw.stage_jpeg_cmyk(str(path), n_px, region)
        assert got[:2] == (W, H) and 0 < got[2] <= cap and got[2] % 16 == 0 and region[got[2]] == 0xAB
        it = jpeg_parse.parse(blob, keep_stuffing=True, cmyk=True)
        ints = np.frombuffer(region, np.int32, count=dw.JPEG_HDR_INTS)
        assert list(ints[:8]) == [dw.KIND_JPEG_CMYK, W, H, 4, it.hs, it.vs, len(it.stream), it.blocks()]
        assert ints[dw.HDR.COEF_OFF] == dw.CMYK_COEF_OFF and ints[dw.HDR.TRANSFORM] == tf and ints[dw.HDR.LAYOUT] == 0
        assert ints[dw.HDR.STUFFED] == it.stuffed and ints[dw.HDR.RESTART_INTERVAL] == it.ri
        assert dw.stage_jpeg_cmyk(str(path), n_px, np.zeros(dw.CMYK_COEF_OFF + 8, np.uint8)) == (W, H, -got[2])
        slots.append(slot)
        items.append(it)
    with pytest.raises(Unsupported):                           # three components: stage_jpeg's file
        dw.stage_jpeg_cmyk(str(three), n_px, np.zeros(cap, np.uint8))
    assert dw.stage_jpeg(str(three), n_px, np.zeros(cap, np.uint8))[2] > 0
    records, decoder_bytes, group, px, entry = device_stage.all_formats()[dw.KIND_JPEG_CMYK]
    recs, tables, jobs, out_sz, blocks, nt = records(big, n, cap, slots, np.arange(n), n_px)
    ref, ref_tables = jpeg.pack(items, cmyk=True)[:2]
    assert recs.dtype == jpeg.IMAGE4
    for f in ("stream_bytes", "width", "height", "ncomp", "hs", "vs", "coef_off", "out_off", "restart_interval", "n_intervals", "stuffed",
              "reserved", "quant"):
        assert np.array_equal(recs[f], ref[f]), f
    tables = tables.reshape(-1, jpeg_parse.TABLE_BYTES)
    assert nt == len(tables) == len(ref_tables)
    for f in ("dc_tbl", "ac_tbl"):
        assert [[tables[i].tobytes() for i in row] for row in recs[f]] == [[ref_tables[i].tobytes() for i in row] for row in ref[f]], f
    hd = device_stage._headers(big, n, cap, np.asarray(slots))
    assert list(decoder_bytes(hd)) == [192 * it.blocks() for it in items] and list(blocks) == [it.blocks() for it in items]
    assert list(out_sz) == [(it.width * it.height * 4 + 15) // 16 * 16 for it in items]
    for k, (r, it, slot) in enumerate(zip(recs, items, slots)):
        o, nb = int(r["stream_off"]), int(r["stream_bytes"])
        assert slot * cap <= o and o + nb + 16 <= (slot + 1) * cap and big[o:o + nb].tobytes() == bytes(it.stream)
        if it.ri:
            io_ = int(r["intervals_off"])
            assert np.array_equal(np.frombuffer(big, np.uint32, count=len(it.starts), offset=io_), it.starts)
        j = jobs[k]
        assert int(j["src_off"]) == int(r["out_off"]) and int(j["out_index"]) == slot and (int(j["w"]), int(j["h"])) == (it.width, it.height)
        plan = dw.resize_plan(it.width, it.height, n_px)
        assert (int(j["r0"]), int(j["nrows"]), int(j["need_h"]), int(j["need_v"]), int(j["left"]), int(j["top"]), int(j["hk"]),
                int(j["vk"])) == (plan["r0"], plan["nrows"], plan["need_h"], plan["need_v"], plan["left"], plan["top"], plan["hk"], plan["vk"])
        hc = np.frombuffer(big, np.int32, count=plan["hcoef"].size, offset=4 * int(j["hcoef_off"]))
        vc = np.frombuffer(big, np.int32, count=plan["vcoef"].size, offset=4 * int(j["vcoef_off"]))
        assert np.array_equal(hc, plan["hcoef"]) and np.array_equal(vc, plan["vcoef"])
    tmp = jobs["nrows"].astype(np.int64) * n_px * 4
    assert np.array_equal(jobs["tmp_off"], np.cumsum(tmp) - tmp)


def test_the_worker_answers_with_the_new_tag_only_where_the_bit_allows(tmp_path):
    """serve(): a four-component file is tagged b"9" with bit 128 in the mode, and decoded by Pillow (b"1") without it"""
    import struct
    from multiprocessing import shared_memory
    dw = decode_worker
    rng = np.random.default_rng(10)
    n_px, cap = 32, 64 << 10
    four, three = tmp_path / "four.jpg", tmp_path / "three.jpg"
    four.write_bytes(jc.cmyk_file(jc.smooth4(rng, 40, 33), subsampling=2))
    three.write_bytes(jc.encode(jc.smooth(rng, 40, 33), quality=85, subsampling=2))
    small = shared_memory.SharedMemory(create=True, size=4 * 3 * n_px * n_px)
    big = shared_memory.SharedMemory(create=True, size=4 * cap)
    try:
        lines = []
        for slot, (path, mode) in enumerate([(four, 2 | 128), (four, 2), (three, 2 | 128), (four, 2 | 4 | 32 | 128)]):
            lines.append(b"%d\t%s\t%d\t%s\t%d\t%d\t%d\t" % (n_px, small.name.encode(), slot * 3 * n_px * n_px, big.name.encode(), slot * cap, cap, mode)
                         + str(path).encode().hex().encode() + b"\n")
        fout = io.BytesIO()
        dw.serve(io.BytesIO(b"".join(lines)), fout)
        raw = fout.getvalue()
        assert len(raw) == 17 * 4
        tags = [raw[17 * k:17 * k + 1] for k in range(4)]
        assert tags == [b"9", b"1", b"3", b"9"]
        assert struct.unpack_from("<iiq", raw, 1)[:2] == (33, 40)
        got = np.frombuffer(small.buf, np.uint8, count=3 * n_px * n_px, offset=3 * n_px * n_px).reshape(3, n_px, n_px)
        assert np.array_equal(got, load_uint8(str(four), n_px))
        del got
    finally:
        for seg in (small, big):
            seg.close()
            seg.unlink()


def test_the_committed_files_against_pillow_live(tmp_path):
    d = np.load(GOLDEN)
    n, n_px = int(d["n"]), int(d["n_px"])
    assert n >= 12 and n_px == 32
    forms = {str(name).split()[0] for name in d["names"]}
    assert forms == set(jc.FORMS)
    for i in range(n):
        blob = d[f"file_{i}"].tobytes()
        p = jpeg_parse.parse(blob, keep_stuffing=True, cmyk=True)
        assert p.ncomp == 4 and d[f"cmyk_{i}"].shape == (p.height, p.width, 4), str(d["names"][i])
        assert np.array_equal(jc.pillow4(blob), d[f"cmyk_{i}"]), str(d["names"][i])
        path = tmp_path / f"{i}.jpg"
        path.write_bytes(blob)
        assert np.array_equal(load_uint8(str(path), n_px), d[f"transform_{i}"]), str(d["names"][i])
