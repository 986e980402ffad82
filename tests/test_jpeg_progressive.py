"""Progressive JPEG files on the CPU: the host parser (jpeg_parse.parse_progressive), the CPU restatement of the device
decoder (tests/jpeg_progressive.py) against Pillow live and the committed Pillow pixels, and the progressive writer."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image, ImageFile

import clipmi
import jpeg_progressive
from clipmi import jpeg_parse
from test_jpeg import smooth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_progressive_cases.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def big_encode_buffer(monkeypatch):
    # Pillow's default encoder buffer is too small for progressive noise files of a few hundred pixels a side
    monkeypatch.setattr(ImageFile, "MAXBLOCK", 1 << 24)


def pillow(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def encode(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def segments(blob):
    """[(marker, start)] of the file's marker segments and SOS headers, in order"""
    return [(blob[m.start() + 1], m.start()) for m in jpeg_parse._MARKER.finditer(blob) if blob[m.start() + 1] not in (0xFF,)]


def test_parser_accepts_pillow_progressive_files():
    rng = np.random.default_rng(3)
    for sub in (0, 1, 2):
        for opt in (False, True):
            a = smooth(rng, 37, 53)
            p = jpeg_parse.parse_progressive(encode(a, quality=80, subsampling=sub, optimize=opt, progressive=True))
            assert (p.ncomp, p.hs, p.vs) == (3, (1, 2, 2)[sub], (1, 1, 2)[sub])
            assert len(p.scans) == 10 and p.scans[0].comps == (0, 1, 2) and (p.scans[0].ss, p.scans[0].al) == (0, 1)
            assert all(len(s.comps) == 1 for s in p.scans if s.ss)
    p = jpeg_parse.parse_progressive(encode(smooth(rng, 30, 20)[..., 0], quality=70, progressive=True))
    assert p.ncomp == 1 and len(p.scans) == 6
    for blob, name in jpeg_progressive.writer_cases(rng, big=False):
        assert jpeg_parse.parse_progressive(blob).scans, name


def test_baseline_parser_still_refuses_progressive_and_vice_versa():
    rng = np.random.default_rng(4)
    a = smooth(rng, 40, 40)
    with pytest.raises(jpeg_parse.Unsupported):
        jpeg_parse.parse(encode(a, quality=80, progressive=True))
    with pytest.raises(jpeg_parse.Unsupported):
        jpeg_parse.parse_progressive(encode(a, quality=80))


def _sos_params(blob, n, ss=None, se=None, ahal=None):
    """blob with the n-th SOS header's Ss / Se / Ah-Al bytes replaced"""
    s0 = [k for m, k in segments(blob) if m == 0xDA][n]
    ns = blob[s0 + 4]
    b = bytearray(blob)
    for off, v in ((0, ss), (1, se), (2, ahal)):
        if v is not None:
            b[s0 + 5 + 2 * ns + off] = v
    return bytes(b)


def _refused(blob):
    with pytest.raises(jpeg_parse.Unsupported):
        jpeg_parse.parse_progressive(blob)


def test_parser_refuses_what_the_device_does_not_vouch_for():
    rng = np.random.default_rng(5)
    base = encode(smooth(rng, 48, 64), quality=80, subsampling=2, progressive=True)
    jpeg_parse.parse_progressive(base)
    # an incomplete script: the file ends after the first six scans (DC and luma not at Al = 0)
    sos = [k for m, k in segments(base) if m == 0xDA]
    _refused(base[:sos[6]] + b"\xff\xd9")
    # restart intervals
    _refused(encode(smooth(rng, 48, 64), quality=80, progressive=True, restart_marker_blocks=4))
    # bogus progressions and invalid scan parameters (jdphuff.c)
    _refused(_sos_params(base, 0, se=3))                 # DC scan with Se != 0
    _refused(_sos_params(base, 1, ss=6, se=5))           # Ss > Se
    _refused(_sos_params(base, 1, se=64))                # Se > 63
    _refused(_sos_params(base, 1, ahal=0x0E))            # Al > 13
    _refused(_sos_params(base, 5, ahal=0x20))            # a refinement from Al 2 to 0: Ah != Al + 1
    _refused(_sos_params(base, 5, ahal=0x10))            # Ah 1: not the bit the coefficients reached
    _refused(_sos_params(base, 1, ahal=0x32))            # a refinement before its first scan
    _refused(_sos_params(base, 0, ss=1, se=63))          # an AC scan of three components / before the DC scan
    # SOF10 (arithmetic) and SOF6 frames
    for m in (0xCA, 0xC6):
        b = bytearray(base)
        b[[k for mm, k in segments(base) if mm == 0xC2][0] + 1] = m
        _refused(bytes(b))
    # DQT between scans; DNL between scans; a missing EOI; truncation inside a scan
    dqt = [k for m, k in segments(base) if m == 0xDB][0]
    L = int.from_bytes(base[dqt + 2:dqt + 4], "big")
    _refused(base[:sos[3]] + base[dqt:dqt + 2 + L] + base[sos[3]:])
    _refused(base[:sos[3]] + b"\xff\xdc\x00\x04\x00\x30" + base[sos[3]:])
    _refused(base[:-2])
    _refused(base[:sos[4] + 40])


def test_parser_refuses_more_than_max_scans_and_too_much_work(monkeypatch):
    """A valid, complete script of 190 single-coefficient scans is refused for its count alone (a script of 64 such scans is
    taken); a file whose serial walk would exceed MAX_WORK coefficient steps is refused for that."""
    base = encode(smooth(np.random.default_rng(9), 24, 32), quality=80, subsampling=2)
    many = jpeg_progressive.write(base, [((0, 1, 2), 0, 0, 0, 0)] + [((c,), k, k, 0, 0) for c in range(3) for k in range(1, 64)])
    assert np.array_equal(pillow(many), pillow(base))
    with pytest.raises(jpeg_parse.Unsupported, match="too many scans"):
        jpeg_parse.parse_progressive(many)
    grey = encode(smooth(np.random.default_rng(9), 24, 32)[..., 0], quality=80)
    assert len(jpeg_parse.parse_progressive(jpeg_progressive.write(grey, [((0,), 0, 0, 0, 0)] + [((0,), k, k, 0, 0) for k in range(1, 64)])).scans) == 64
    blob = encode(smooth(np.random.default_rng(9), 48, 64), quality=80, subsampling=2, progressive=True)
    p = jpeg_parse.parse_progressive(blob)
    steps = sum(sum((48 if c == 0 else 12) for c in s.comps) * (s.se - s.ss + 1) for s in p.scans)       # 6 x 8 luma, 3 x 4 chroma blocks
    monkeypatch.setattr(jpeg_parse, "MAX_WORK", steps)
    jpeg_parse.parse_progressive(blob)
    monkeypatch.setattr(jpeg_parse, "MAX_WORK", steps - 1)
    with pytest.raises(jpeg_parse.Unsupported, match="too much work"):
        jpeg_parse.parse_progressive(blob)


def test_worker_regions_give_the_records_pack_progressive_gives(tmp_path):
    """decode_worker.stage_jpeg_progressive's region, read back by device_stage.progressive_records, holds the records, scans,
    tables and segments jpeg.pack_progressive builds from the same files (the pipeline's form of the same input)."""
    from clipmi import decode_worker, device_stage, jpeg
    rng = np.random.default_rng(12)
    blobs = [encode(smooth(rng, 40 + 9 * k, 60 - 5 * k), quality=75 + k, subsampling=k % 3, progressive=True) for k in range(4)]
    blobs.append(jpeg_progressive.writer_cases(rng, big=False)[1][0])
    cap = 1 << 16
    big = np.zeros(len(blobs) * cap, np.uint8)
    for k, b in enumerate(blobs):
        (tmp_path / f"{k}.jpg").write_bytes(b)
        w, h, used = decode_worker.stage_jpeg_progressive(str(tmp_path / f"{k}.jpg"), 224, big[k * cap:(k + 1) * cap])
        assert 0 < used <= cap
    with pytest.raises(jpeg_parse.Unsupported):
        decode_worker.stage_jpeg_progressive(_baseline(tmp_path), 224, big[:cap])
    assert decode_worker.stage_jpeg_progressive(str(tmp_path / "0.jpg"), 224, big[:256])[2] < 0          # does not fit: bytes wanted
    decode_worker.stage_jpeg_progressive(str(tmp_path / "0.jpg"), 224, big[:cap])
    recs, scans, tables, jobs, out_sz, blocks, nt = device_stage.progressive_records(big, len(blobs), cap, np.arange(len(blobs)),
                                                                                np.arange(len(blobs)), 224)
    items = [jpeg_parse.parse_progressive(b) for b in blobs]
    prec, pscans, ptables = jpeg.pack_progressive(items)[:3]
    for f in ("coef_off", "out_off", "width", "height", "ncomp", "hs", "vs", "first_scan", "n_scans", "quant"):
        assert np.array_equal(recs[f], prec[f]), f
    assert nt == len(ptables) and list(blocks) == [it.blocks() for it in items]
    for k, it in enumerate(items):
        for j, sc in enumerate(it.scans):
            r = scans[recs["first_scan"][k] + j]
            o, nb = int(r["stream_off"]), int(r["stream_bytes"])
            assert bytes(big[o:o + nb]) == sc.stream and not big[o + nb:o + nb + 16].any() and o % 16 == 0
            assert (r["ss"], r["se"], r["ah"], r["al"], r["ncomp"]) == (sc.ss, sc.se, sc.ah, sc.al, len(sc.comps))
            assert list(r["comp"][:len(sc.comps)]) == list(sc.comps)
            want = sc.dc if sc.ss == 0 else sc.ac
            for i, t in enumerate(want):
                assert (r["tbl"][i] == -1) if t is None else (bytes(tables[r["tbl"][i] * 288:(r["tbl"][i] + 1) * 288]) == t)


def _baseline(tmp_path):
    p = tmp_path / "baseline.jpg"
    p.write_bytes(encode(smooth(np.random.default_rng(1), 30, 30), quality=80))
    return str(p)


def test_parser_never_accepts_a_file_pillow_refuses():
    corpus = jpeg_progressive.malformed_corpus(np.random.default_rng(11))
    for fam, blob in corpus:
        try:
            jpeg_parse.parse_progressive(blob)
        except jpeg_parse.Unsupported:
            continue
        pillow(blob)                                     # accepted: Pillow decodes it without an error


def test_complete_script_equals_baseline_and_incomplete_script_smooths():
    """libjpeg applies block smoothing only while a low coefficient is incomplete: the same coefficients written with a
    complete script decode to the baseline file's pixels, and a script that stops early decodes differently from plain
    jpeg_idct_islow of what it holds (which is why parse_progressive refuses it)."""
    rng = np.random.default_rng(6)
    for (h, w), sub in [((224, 224), 2), ((37, 53), 1), ((300, 200), 0)]:
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(pillow(encode(a, quality=85, subsampling=sub, progressive=True)), pillow(encode(a, quality=85, subsampling=sub)))
    base = encode(smooth(rng, 64, 64)[..., 0], quality=85)
    full = jpeg_progressive.write(base, [((0,), 0, 0, 0, 1), ((0,), 1, 63, 0, 0), ((0,), 0, 0, 1, 0)])
    assert np.array_equal(pillow(full), pillow(base))
    part = jpeg_progressive.write(base, [((0,), 0, 0, 0, 1), ((0,), 1, 63, 0, 0)])           # DC stops at Al = 1
    _refused(part)
    assert not np.array_equal(pillow(part), pillow(base))


def test_restatement_equals_pillow_live():
    rng = np.random.default_rng(7)
    n = 0
    for (h, w) in [(5, 7), (8, 8), (17, 16), (37, 53), (64, 129)]:
        for sub in (0, 1, 2):
            for q in (95, 75, 30):
                for a in (smooth(rng, h, w), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)):
                    blob = encode(a, quality=q, subsampling=sub, progressive=True, optimize=bool(q == 75))
                    assert np.array_equal(jpeg_progressive.decode(blob), pillow(blob))
                    n += 1
    for q in (90, 40):
        blob = encode(smooth(rng, 29, 31)[..., 0], quality=q, progressive=True)
        assert np.array_equal(jpeg_progressive.decode(blob), pillow(blob))
    blob = encode(np.zeros((16, 16, 3), np.uint8), quality=50, progressive=True)
    assert np.array_equal(jpeg_progressive.decode(blob), pillow(blob))
    assert n == 90


def test_restatement_equals_the_committed_pillow_pixels():
    d = np.load(GOLDEN)
    assert int(d["n"]) >= 25
    for i in range(int(d["n"])):
        assert np.array_equal(jpeg_progressive.decode(d[f"file_{i}"].tobytes()), d[f"rgb_{i}"])


def test_writer_round_trips_to_the_baseline_pixels():
    """Pillow decodes every writer script to exactly the baseline file's pixels (the writer pinned without any decoder of
    ours), and the restatement agrees with Pillow on them; the 2 000 x 1 500 file holds EOB runs of the maximum length."""
    rng = np.random.default_rng(8)
    cases = jpeg_progressive.writer_cases(rng)
    assert len(cases) >= 20
    for blob, name in cases:
        p = jpeg_parse.parse_progressive(blob)
        assert len({s.dc[0] if s.dc else s.ac[0] for s in p.scans if (s.dc and s.dc[0]) or s.ac}) > 1, name
        if "2000x1500" not in name:
            assert np.array_equal(jpeg_progressive.decode(blob), pillow(blob)), name
    # the baseline files the cases came from: write them again from a fixed base and compare with it
    base = encode(smooth(rng, 37, 53), quality=77, subsampling=1)
    for name, script in jpeg_progressive.scripts(3).items():
        assert np.array_equal(pillow(jpeg_progressive.write(base, script)), pillow(base)), name
    base = encode(smooth(rng, 29, 11)[..., 0], quality=60)
    for name, script in jpeg_progressive.scripts(1).items():
        assert np.array_equal(pillow(jpeg_progressive.write(base, script)), pillow(base)), name
    y, x = np.mgrid[0:1500, 0:2000]
    big = encode((128 + 100 * np.sin(x / 97.0) * np.cos(y / 61.0)).astype(np.uint8), quality=60)
    assert np.array_equal(pillow(cases[-1][0]), pillow(big))
    ev = jpeg_progressive._encode_scan(jpeg_progressive.jpeg_oracle.decode_coefficients(jpeg_progressive.jpeg_oracle.parse(big))[0],
                                       jpeg_progressive._Geom(jpeg_progressive.jpeg_oracle.parse(big)), ((0,), 40, 63, 0, 0))
    assert ("h", 0, 14 << 4) in ev                       # an EOB14 symbol: a run of at least 16 384 blocks


def test_progressive_records_match_the_header(tmp_path):
    """The numpy records of jpeg.py equal the C compiler's view of clipmi_jpeg_scan / clipmi_jpeg_progressive_image."""
    from clipmi import jpeg
    src = tmp_path / "t.c"
    body = []
    for st, dt in (("clipmi_jpeg_scan", jpeg.SCAN), ("clipmi_jpeg_progressive_image", jpeg.PIMAGE)):
        body.append(f'printf("{st} sizeof %zu\\n", sizeof({st}));')
        body += [f'printf("{st} {f} %zu\\n", offsetof({st}, {f}));' for f in dt.names]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipmi.h"\nint main(){' + "\n".join(body) + "return 0;}")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = {tuple(l.split()[:2]): int(l.split()[2]) for l in subprocess.check_output([str(exe)], text=True).splitlines()}
    for st, dt in (("clipmi_jpeg_scan", jpeg.SCAN), ("clipmi_jpeg_progressive_image", jpeg.PIMAGE)):
        assert out[(st, "sizeof")] == dt.itemsize
        for f in dt.names:
            assert out[(st, f)] == dt.fields[f][1], (st, f)


def test_progressive_entry_validates_arguments_without_gpu():
    L = clipmi._lib.lib()
    assert L.clipmi_jpeg_progressive_workspace_bytes(-1, 10, 1) == -1
    assert L.clipmi_jpeg_progressive_workspace_bytes(2, 10, 3) > 10 * 192
    fake = C.c_void_p(256)
    rc = L.clipmi_jpeg_decode_progressive_rgb8(fake, fake, 1, fake, 0, fake, 1, 10, 10, 10, fake, fake, fake, 1 << 20, None)
    assert rc != 0 and "bad arguments" in clipmi._lib.last_error()
    rc = L.clipmi_jpeg_decode_progressive_rgb8(fake, fake, 1, fake, 1, fake, 1, 10, 10, 10, fake, fake, fake, 16, None)
    assert rc != 0 and "workspace" in clipmi._lib.last_error()
