"""The host side of the PNG decode on the device, without a GPU: the chunk parser (cli-p_amd/png_parse.py) against Pillow, the
CPU restatement of the decoder (png_cases.cpu_decode: zlib.decompressobj(-15) plus a numpy unfilter) against Pillow's pixels,
the two new entry points' argument checks, and the worker's region layout."""
import ctypes as C
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from clipmi import png, png_parse
import png_cases


def pillow(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def save(img, **kw):
    buf = io.BytesIO()
    img.save(buf, format="PNG", **kw)
    return buf.getvalue()


def pillow_saved(rng, sizes=((1, 1), (5, 7), (64, 64), (65, 63), (13, 300), (300, 13), (224, 224))):
    """[(name, file)]: smooth and noise images, L and RGB, as Pillow's own encoder writes them"""
    out = []
    k = 0
    for (h, w) in sizes:
        for ch in (1, 3):
            for name, gen in (("smooth", png_cases.smooth), ("noise", png_cases.noise)):
                a = gen(rng, h, w, ch)
                kw = [{"compress_level": 0}, {"compress_level": 1}, {"compress_level": 6}, {"compress_level": 9}, {"optimize": True}][k % 5]
                out.append((f"pillow_{name}_{h}x{w}_c{ch}_{k % 5}", save(Image.fromarray(a[..., 0] if ch == 1 else a), **kw)))
                k += 1
    return out


@pytest.fixture(scope="module")
def valid_files():
    rng = np.random.default_rng(1)
    return png_cases.writer_cases(rng) + pillow_saved(rng)


def test_accepted_files_decode_to_pillows_pixels(valid_files):
    """parse accepts every valid writer case and every Pillow-saved L / RGB file, Pillow opens every one of them, and inflate plus
    unfilter of the parsed stream gives Pillow's pixels."""
    assert len(valid_files) >= 200
    for name, blob in valid_files:
        ref = pillow(blob)
        p = png_parse.parse(blob)
        assert (p.height, p.width) == ref.shape[:2] and p.channels in (1, 3), name
        got = png_cases.cpu_decode(p)
        assert got is not None and np.array_equal(got, ref), name


def test_every_pillow_compress_level_and_optimize():
    rng = np.random.default_rng(2)
    for mode_ch in (1, 3):
        a = png_cases.smooth(rng, 33, 47, mode_ch)
        img = Image.fromarray(a[..., 0] if mode_ch == 1 else a)
        for kw in ({"compress_level": 0}, {"compress_level": 1}, {"compress_level": 6}, {"compress_level": 9}, {"optimize": True}):
            blob = save(img, **kw)
            assert np.array_equal(png_cases.cpu_decode(png_parse.parse(blob)), pillow(blob))


def _refused(blob):
    with pytest.raises(png_parse.Unsupported):
        png_parse.parse(blob)


def test_parser_refuses_what_the_device_does_not_decode():
    """For each refused file that Pillow opens, Pillow's mode or flags confirm the reason."""
    rng = np.random.default_rng(3)
    rgb = Image.fromarray(png_cases.smooth(rng, 20, 30))
    for img, mode in ((rgb.convert("P"), "P"), (rgb.convert("LA"), "LA"), (rgb.convert("RGBA"), "RGBA"), (rgb.convert("1"), "1"),
                      (Image.fromarray(rng.integers(0, 65536, (20, 30)).astype(np.uint16)), "I;16")):
        blob = save(img)
        assert Image.open(io.BytesIO(blob)).mode == mode
        _refused(blob)
    a = png_cases.smooth(rng, 16, 16)
    raw = png_cases.filter_rows(a, [0] * 16)
    z = png_cases.deflate(raw)
    good = png_cases.assemble(16, 16, 3, z)
    assert np.array_equal(png_cases.cpu_decode(png_parse.parse(good)), pillow(good))
    laced = png_cases.assemble(16, 16, 3, z, lace=1)
    assert Image.open(io.BytesIO(laced)).info.get("interlace") == 1
    _refused(laced)
    trns = png_cases.assemble(16, 16, 3, z, before=png_cases.chunk(b"tRNS", b"\0\1\0\2\0\3"))
    im = Image.open(io.BytesIO(trns))
    assert im.mode == "RGB" and "transparency" in im.info
    _refused(trns)
    apng = save(rgb, save_all=True, append_images=[rgb.rotate(90)])
    assert Image.open(io.BytesIO(apng)).is_animated
    _refused(apng)
    for before in (png_cases.chunk(b"PLTE", bytes(range(48))), png_cases.chunk(b"iCCP", b"x\0\0" + zlib.compress(b"profile")),
                   png_cases.chunk(b"zzZz", b"private"), png_cases.chunk(b"gAMA", struct.pack(">I", 45455), crc=1),
                   png_cases.chunk(b"gAMA", b"\0\0")):
        _refused(png_cases.assemble(16, 16, 3, z, before=before))
    bad_ihdr = bytearray(good)
    bad_ihdr[29] ^= 1                                          # the IHDR chunk's CRC
    with pytest.raises(Exception):
        Image.open(io.BytesIO(bytes(bad_ihdr)))
    _refused(bytes(bad_ihdr))
    for header in (b"\x78\x02", b"\x88\x1c", b"\x79\x18", b"\x78\x20"):     # FCHECK, CINFO 8, CM 9, FDICT (+ FCHECK)
        _refused(png_cases.assemble(16, 16, 3, header + z[2:]))
    _refused(png_cases.assemble(16, 16, 3, b"\x78"))
    apart = png_cases.assemble(16, 16, 3, z[:40], after=png_cases.chunk(b"tEXt", b"k\0v") + png_cases.chunk(b"IDAT", z[40:]))
    _refused(apart)                                            # IDAT chunks that are not consecutive
    _refused(png_cases.assemble(0, 16, 3, z))
    _refused(png_cases.assemble(16, 0, 3, z))
    _refused(png_cases.assemble(16, 16, 3, z, depth=16))
    _refused(png_cases.assemble(16, 16, 3, z, ctype=3))
    _refused(b"not a PNG file at all")
    _refused(save(rgb)[:30])
    buf = io.BytesIO()
    rgb.save(buf, format="JPEG")
    _refused(buf.getvalue())


def test_chunks_behind_the_image_data():
    """What Pillow refuses because of a chunk behind the IDAT run (its refusal confirmed per file) the parser refuses too, although
    stream and checksum are intact; what Pillow ignores there (bad CRCs, unknown chunks that fit, garbage shorter than a chunk
    header or without a chunk type, anything behind IEND) is let through and decodes to Pillow's pixels."""
    refused, accepted = png_cases.behind_idat_cases(np.random.default_rng(8))
    img = png_cases.smooth(np.random.default_rng(9), 16, 16)
    z = png_cases.deflate(png_cases.filter_rows(img, [1] * 16))
    refused.append(("tEXt_70MiB", png_cases.assemble(16, 16, 3, z, after=png_cases.chunk(b"tEXt", b"k\0" + bytes(70 << 20)))))
    assert len(refused) >= 11 and len(accepted) >= 6
    for name, blob in refused:
        with pytest.raises(Exception):
            pillow(blob)
        with pytest.raises(png_parse.Unsupported):
            png_parse.parse(blob)
    for name, blob in accepted:
        assert np.array_equal(png_cases.cpu_decode(png_parse.parse(blob)), pillow(blob)), name
    for cid in (b"PLTE", b"eXIf", b"zTXt", b"iTXt", b"tRNS", b"IDAT"):      # handlers outside the reasoned list: handed to Pillow
        _refused(png_cases.assemble(16, 16, 3, z, after=png_cases.chunk(b"tEXt", b"k\0v") + png_cases.chunk(cid, b"\0" * 6)))
    _refused(png_cases.assemble(png_parse.MAX_WIDTH + 1, 1, 1, z))


def test_parse_keeps_the_trailer_and_what_follows():
    a = png_cases.noise(np.random.default_rng(4), 5, 6)
    raw = png_cases.filter_rows(a, [1] * 5)
    z = png_cases.deflate(raw)
    p = png_parse.parse(png_cases.assemble(6, 5, 3, z + b"tail", idat=7))
    assert p.stream == z[2:] + b"tail" and (p.width, p.height, p.channels) == (6, 5, 3) and p.raw_bytes() == len(raw)
    recs, streams, out_bytes, total_raw, max_raw = png.pack([p, p])
    assert recs["stream_off"][1] % 16 == 0 and recs["stream_off"][1] >= len(p.stream) + 16
    assert bytes(streams[:len(p.stream)]) == p.stream and not streams[len(p.stream):recs["stream_off"][1]].any()
    assert total_raw == 2 * ((len(raw) + 15) // 16 * 16) and max_raw == len(raw) and recs["raw_off"][1] % 16 == 0
    assert out_bytes == 2 * ((5 * 6 * 3 + 15) // 16 * 16)


def test_bindings_check_their_arguments_without_a_launch(clipmi):
    L = clipmi._lib.lib()
    assert hasattr(L, "clipmi_png_workspace_bytes") and hasattr(L, "clipmi_png_decode_rgb8")
    assert L.clipmi_abi_version() == 8 and clipmi._lib.ABI_VERSION == 8
    need = L.clipmi_png_workspace_bytes(4, 1 << 20)
    assert need >= (1 << 20) + 16
    assert L.clipmi_png_workspace_bytes(-1, 16) < 0 and L.clipmi_png_workspace_bytes(1, -1) < 0
    fake = C.c_void_p(4096)
    EINVAL, EWORKSPACE = 1, 2
    assert L.clipmi_png_decode_rgb8(fake, fake, 0, 1 << 20, 1 << 10, fake, fake, fake, need, None) == EINVAL
    assert L.clipmi_png_decode_rgb8(fake, fake, -3, 1 << 20, 1 << 10, fake, fake, fake, need, None) == EINVAL
    for hole in range(5):
        ptrs = [fake] * 5
        ptrs[hole] = None
        rc = L.clipmi_png_decode_rgb8(ptrs[0], ptrs[1], 4, 1 << 20, 1 << 10, ptrs[2], ptrs[3], ptrs[4], need, None)
        assert rc == EINVAL and "png_decode_rgb8" in clipmi._lib.last_error()
    assert L.clipmi_png_decode_rgb8(fake, fake, 4, 1 << 20, (1 << 20) + 1, fake, fake, fake, need, None) == EINVAL
    rc = L.clipmi_png_decode_rgb8(fake, fake, 4, 1 << 20, 1 << 10, fake, fake, fake, need - 1, None)
    assert rc in (EINVAL, EWORKSPACE) and "workspace" in clipmi._lib.last_error()


def test_decode_device_refuses_the_cpu():
    p = png_parse.parse(png_cases.write(png_cases.noise(np.random.default_rng(5), 3, 3)))
    with pytest.raises(Exception, match="no CPU fallback"):
        png.decode_device([p], "cpu")


def test_stage_png_round_trips_a_file_through_a_region(tmp_path):
    from clipmi import decode_worker
    rng = np.random.default_rng(6)
    for k, (h, w, ch) in enumerate([(300, 500, 3), (224, 224, 1), (40, 30, 3)]):
        blob = png_cases.write(png_cases.smooth(rng, h, w, ch), "cycle")
        path = tmp_path / f"f{k}.png"
        path.write_bytes(blob)
        p = png_parse.parse(blob)
        region = np.full(1 << 20, 0xAB, np.uint8)
        got = decode_worker.stage_png(str(path), 224, region)
        assert got[:2] == (w, h) and 0 < got[2] <= region.size and got[2] % 16 == 0
        ints = np.frombuffer(region, np.int32, count=decode_worker.JPEG_HDR_INTS)
        plan = decode_worker.resize_plan(w, h, 224)
        assert list(ints[:8]) == [6, w, h, ch, 0, 0, len(p.stream), 0]
        assert list(ints[8:18]) == [plan["r0"], plan["nrows"], plan["need_h"], plan["need_v"], plan["left"], plan["top"], plan["hk"],
                                    plan["vk"], plan["hcoef"].size, plan["vcoef"].size]
        o_stream, o_coef = int(ints[18]), int(ints[19])
        assert o_stream % 16 == 0 and o_coef == decode_worker.JPEG_COEF_OFF
        nh, nv = plan["hcoef"].size, plan["vcoef"].size
        co = np.frombuffer(region, np.int32, count=nh + nv, offset=o_coef)
        assert np.array_equal(co[:nh], plan["hcoef"]) and np.array_equal(co[nh:], plan["vcoef"])
        assert bytes(region[o_stream:o_stream + len(p.stream)]) == p.stream
        assert got[2] >= o_stream + len(p.stream) + 16 and not region[o_stream + len(p.stream):got[2]].any()
        assert region[got[2]] == 0xAB
        small = np.zeros(o_stream + 8, np.uint8)
        assert decode_worker.stage_png(str(path), 224, small) == (w, h, -got[2])
    bad = tmp_path / "rgba.png"
    Image.fromarray(png_cases.noise(rng, 8, 8, 4), "RGBA").save(bad)
    with pytest.raises(png_parse.Unsupported):
        decode_worker.stage_png(str(bad), 224, np.zeros(1 << 16, np.uint8))


def test_worker_regions_and_the_png_records_built_from_them(tmp_path):
    """What a decode worker lays out for PNG files (decode_worker.stage_png) and what the parent builds out of a batch's regions
    (device_stage.png_records) is, field for field, what png.pack builds from the parsed files, with the streams in place in the
    segment; the resize jobs are resize_plan's, with the coefficient blocks where the jobs point."""
    from clipmi import decode_worker as dw, device_stage
    rng = np.random.default_rng(7)
    specs = [(64, 96, 3), (260, 300, 1), (224, 224, 3), (300, 260, 1)]          # (h, w, channels)
    n, cap, n_px = len(specs) + 2, 256 << 10, 224
    big = np.full(n * cap, 0xAB, np.uint8)
    slots, items = [], []
    for k, (h, w, ch) in enumerate(specs):
        blob = png_cases.write(png_cases.smooth(rng, h, w, ch), "cycle")
        path = tmp_path / f"f{k}.png"
        path.write_bytes(blob)
        slot = k + (1 if k >= 2 else 0)                           # slot 2 holds no PNG file: a gap in the batch
        got = dw.stage_png(str(path), n_px, big[slot * cap:(slot + 1) * cap])
        assert got[:2] == (w, h) and 0 < got[2] <= cap
        slots.append(slot)
        items.append(png_parse.parse(blob))
    comp = np.arange(n)
    recs, jobs, out_sz, raw_sz = device_stage.png_records(big, n, cap, slots, comp, n_px)
    ref = png.pack(items)[0]
    for f in ("stream_bytes", "width", "height", "channels", "raw_off", "out_off"):
        assert np.array_equal(recs[f], ref[f]), f
    assert list(out_sz) == [(it.width * it.height * 3 + 15) // 16 * 16 for it in items]
    assert list(raw_sz) == [(it.raw_bytes() + 15) // 16 * 16 for it in items]
    for k, (r, it, slot) in enumerate(zip(recs, items, slots)):
        o, nb = int(r["stream_off"]), int(r["stream_bytes"])
        assert slot * cap <= o and o + nb + 16 <= (slot + 1) * cap and o % 16 == 0
        assert big[o:o + nb].tobytes() == it.stream and not big[o + nb:o + nb + 16].any()
        plan = dw.resize_plan(it.width, it.height, n_px)
        j = jobs[k]
        assert (int(j["w"]), int(j["h"]), int(j["r0"]), int(j["nrows"]), int(j["need_h"]), int(j["need_v"]), int(j["left"]), int(j["top"]),
                int(j["hk"]), int(j["vk"])) == (it.width, it.height, plan["r0"], plan["nrows"], plan["need_h"], plan["need_v"], plan["left"],
                                                plan["top"], plan["hk"], plan["vk"])
        assert int(j["src_off"]) == int(r["out_off"]) and int(j["out_index"]) == slot
        hc = np.frombuffer(big, np.int32, count=plan["hcoef"].size, offset=4 * int(j["hcoef_off"]))
        vc = np.frombuffer(big, np.int32, count=plan["vcoef"].size, offset=4 * int(j["vcoef_off"]))
        assert np.array_equal(hc, plan["hcoef"]) and np.array_equal(vc, plan["vcoef"])
    tmp = jobs["nrows"].astype(np.int64) * n_px * 3
    assert np.array_equal(jobs["tmp_off"], np.cumsum(tmp) - tmp)
