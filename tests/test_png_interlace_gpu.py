"""Adam7-interlaced PNG files on the device (clipmi_png_decode_rgb8 / clipmi_png_decode_px8 with the record's interlace bit;
png.decode_files / png.transform_files(..., interlaced=True)) against Pillow itself. No tolerance: a file the device keeps (status
0) decodes to exactly Pillow's pixels in the file's own mode and transforms to exactly `decode_worker.load_uint8`'s bytes; a file
Pillow refuses never comes back. The hand-written files and the numpy restatement are checked against Pillow on the CPU in
test_png_interlace.py."""
import collections
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from clipmi import png, png_parse
import png_cases
import png_interlace_cases as A
import png_mode_cases as M
import ws_cases as W

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Palette images with Transparency")]
DEV = "cuda:0"


def test_device_decode_equals_pillow():
    """Every file of the list - every combination of empty passes, the band edges of the last and the first pass, pass rows on
    both sides of a wave of bytes, a ring that wraps, every colour type and depth at widths whose pass rows end inside a byte -
    comes back with status 0 and Pillow's bytes. One decode call per entry."""
    files = A.cases(np.random.default_rng(90))
    assert len(files) == 64 + 7 + 6 + 2 + 3 * len(A.KINDS)
    kinds = collections.Counter((b[25], b[24]) for _, b in files)
    assert set(kinds) == set(A.MODES), kinds
    got = png.decode_files([b for _, b in files], DEV, modes=True, interlaced=True)
    handed_back = [name for (name, _), g in zip(files, got) if g is None]
    assert not handed_back, handed_back
    wrong = [name for (name, b), g in zip(files, got) if not A.same(g, b)]
    assert not wrong, wrong
    # without the switch nothing of this comes back, whatever else is on
    assert all(g is None for g in png.decode_files([b for _, b in files[::5]], DEV, modes=True))


def test_interlaced_and_plain_records_in_one_batch():
    """Interlaced records between records that are not: the latter come back bit-equal to a batch without the interlaced
    neighbours, the former equal Pillow."""
    rng = np.random.default_rng(97)
    plain = [png_cases.write(png_cases.smooth(rng, 70, 37, 3), "cycle"), png_cases.write(png_cases.noise(rng, 9, 130, 1), "cycle1"),
             M.mode_file(rng, 6, 8, 65, 22, 1), M.mode_file(rng, 3, 4, 40, 41, 2, with_trns=True), M.mode_file(rng, 0, 2, 33, 33, 3),
             png_cases.write(png_cases.screenshot(rng, 129, 64, 3), 4)]
    laced = [A.lace_file(rng, 2, 8, 70, 37, 1), A.lace_file(rng, 0, 8, 9, 130, 2), A.lace_file(rng, 6, 8, 65, 22, 3),
             A.lace_file(rng, 3, 4, 40, 41, 4, with_trns=True), A.lace_file(rng, 0, 2, 33, 33, 5), A.lace_file(rng, 4, 8, 19, 13, 6)]
    mixed = [b for pair in zip(laced, plain) for b in pair]
    alone = png.decode_files(plain, DEV, modes=True, interlaced=True)
    got = png.decode_files(mixed, DEV, modes=True, interlaced=True)
    assert all(g is not None for g in alone) and all(g is not None for g in got)
    for k, (a, b) in enumerate(zip(alone, got[1::2])):
        if isinstance(a, tuple):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k
        else:
            assert a.shape == b.shape and np.array_equal(a, b), k
    for k, (g, b) in enumerate(zip(got, mixed)):
        assert A.same(g, b), k


@pytest.fixture(scope="module")
def transform_cases():
    rng = np.random.default_rng(98)
    return [(f"{name}_{h}x{w}", A.lace_file(rng, ctype, depth, h, w, k, with_trns=t))
            for k, (name, ctype, depth, t) in enumerate(A.KINDS) for (h, w) in ((70, 37), (300, 260))]


@pytest.mark.parametrize("n_px", [32, 224])
def test_transform_equals_load_uint8(transform_cases, n_px):
    """decode + transform on the device for one file per kind at two sizes (one scaled up, one down): Pillow's transform, bit for bit"""
    got = png.transform_files([b for _, b in transform_cases], n_px, DEV, interlaced=True)
    handed_back = [name for (name, _), g in zip(transform_cases, got) if g is None]
    assert not handed_back, handed_back
    wrong = []
    for (name, b), g in zip(transform_cases, got):
        ref = M.load_uint8_blob(b, n_px)
        if g.shape != ref.shape or not np.array_equal(g, ref):
            wrong.append((name, int((g != ref).sum()) if g.shape == ref.shape else g.shape))
    assert not wrong, wrong
    assert all(g is None for g in png.transform_files([b for _, b in transform_cases[::4]], n_px, DEV))      # (not without the switch)


def test_malformed_files_never_return_wrong_pixels():
    """Status 0 exactly where the CPU restatement accepts the file; wherever it is 0 Pillow decodes the file and the pixels are
    equal; every "harmless" file has status 0."""
    corpus = A.malformed_corpus(np.random.default_rng(92))
    got = png.decode_files([b for _, b in corpus], DEV, modes=True, interlaced=True)
    counts = collections.defaultdict(lambda: [0, 0])           # family -> [files, device pixels]
    for k, ((fam, b), g) in enumerate(zip(corpus, got)):
        p = png_parse.parse(b, modes=True, interlaced=True)
        ref = A.cpu_decode(p) if p.interlace else (png_cases.cpu_decode(p) if p.kind == "rgb" else M.cpu_decode(p))
        counts[fam][0] += 1
        assert (g is None) == (ref is None), f"{fam} (file {k}): the device {'reports' if g is None else 'keeps'} a file the restatement does not"
        if g is not None:
            counts[fam][1] += 1
            Image.open(io.BytesIO(b)).convert("RGB")           # Pillow decodes it
            assert A.same(g, b), f"{fam} (file {k}): status 0 with pixels that are not Pillow's"
    for fam, (n, ok) in sorted(counts.items()):
        print(f"{fam:20s} files {n:5d}  device pixels {ok:5d}")
    assert counts["harmless"] == [20, 20]
    for fam, n in (("filter_byte", 12), ("adler_wrong", 8), ("adler_missing", 4), ("extra_rows", 4), ("short_data", 4), ("wrong_order", 8),
                   ("truncated", 28)):
        assert counts[fam] == [n, 0], (fam, counts[fam])
    assert counts["bitflip"][0] == 48


# ---- workspace independence (tests/ws_cases.py), the interlaced form of both entries ---------------------------------------------
def _bad(ctype, depth, s, palette=None):
    """one interlaced file per status of the stream itself: invalid DEFLATE (1), ended early (2), a filter byte of 7 in the last
    pass (3), a wrong Adler-32 (4)"""
    pieces = A.pass_pieces(s, ctype, depth)
    raw = b"".join(r for _, r, _ in pieces)
    z = png_cases.deflate(raw)
    bad = bytearray(raw)
    bad[len(raw) - 2 * pieces[-1][2]] = 7
    h, w, ch = s.shape

    def f(zz):
        return png_cases.assemble(w, h, ch, zz, before=A.before_chunks(ctype, palette), depth=depth, ctype=ctype, lace=1)
    return [("block type 3", f(z[:2] + bytes([z[2] | 6]) + z[3:])), ("stream cut short", f(z[:len(z) // 2])),
            ("filter byte 7", f(png_cases.deflate(bytes(bad)))), ("Adler-32 + 1", f(z[:-4] + struct.pack(">I", (zlib.adler32(raw) + 1) & 0xffffffff)))]


def _rgb_batch():
    rng = np.random.default_rng(99)
    P = lambda b: png_parse.parse(b, interlaced=True)  # noqa: E731
    good = [("rgb", A.lace_file(rng, 2, 8, 130, 45, 1)), ("grey", A.lace_file(rng, 0, 8, 64, 90, 2)),
            ("rgb stored blocks", A.lace_file(rng, 2, 8, 37, 70, 0, level=0)), ("rgb 3 x 1", A.lace_file(rng, 2, 8, 1, 3, 0))]
    bad = _bad(2, 8, png_cases.smooth(rng, 40, 50, 3))
    out = []
    for k in range(4):
        out.append((good[k][0], P(good[k][1]), A.pillow_pixels(good[k][1])[1], good[k][1]))
        out.append((bad[k][0], P(bad[k][1]), None, None))
    plain = png_cases.write(png_cases.smooth(rng, 21, 22, 3), "cycle")         # and a record without the bit behind them
    out.append(("not interlaced", P(plain), A.pillow_pixels(plain)[1], plain))
    return out


def _px8_batch():
    rng = np.random.default_rng(100)
    P = lambda b: png_parse.parse(b, modes=True, interlaced=True)  # noqa: E731
    good = [("rgba", A.lace_file(rng, 6, 8, 70, 37, 0)), ("p8", A.lace_file(rng, 3, 8, 64, 90, 1)),
            ("p4 + tRNS", A.lace_file(rng, 3, 4, 40, 51, 2, with_trns=True)), ("g2", A.lace_file(rng, 0, 2, 33, 33, 3)),
            ("la", A.lace_file(rng, 4, 8, 19, 13, 4))]
    bad = _bad(6, 8, M.samples_for(rng, 6, 8, 40, 50, 1)[0])
    idx = rng.integers(0, 100, (30, 40, 1), dtype=np.uint8)
    idx[7, 9] = 200
    bad.append(("index beyond the palette", A.write(idx, 3, 8, palette=rng.integers(0, 256, (100, 3), dtype=np.uint8))))
    out = []
    for k in range(5):
        out.append((good[k][0], P(good[k][1]), A.pillow_pixels(good[k][1])[1], good[k][1]))
        out.append((bad[k][0], P(bad[k][1]), None, None))
    return out


@pytest.mark.parametrize("kind", ["png", "png_px8"])
def test_interlaced_decode_does_not_depend_on_its_workspace(clipmi, gpu, kind):
    """Both entries over interlaced records, one file per status between good ones: the same statuses and the same bytes whatever
    the workspace, the output and the status tensor held on entry (zeros, words of 1, random bytes, 0xFF), guard bands intact, the
    good files Pillow's pixels, each reported file alone in its block."""
    from test_ws_decode_gpu import Decode
    batch = _rgb_batch() if kind == "png" else _px8_batch()
    d = Decode(clipmi, gpu, kind, batch)
    assert all(int(r["reserved"][0]) & png.INTERLACE_BIT for r, (name, _, _, _) in zip(d.recs, batch) if name != "not interlaced")
    got = W.run_independent(d, d.outputs, d.ws_bytes, device=gpu, canon=d.canon)
    assert d.check(got) == ([1, 2, 3, 4] if kind == "png" else [1, 2, 3, 4, 5])
