"""PNG files of depth 16 and PNG files with metadata chunks on the device (clipmi_png_decode_px8 with colour type << 8 | 16 in the
record; png.decode_files / png.transform_files(..., chunks=True, deep=True)) against Pillow itself. No tolerance: a file the device
keeps decodes to exactly the pixels Pillow opens it as - every sample's high byte - and transforms to exactly
`decode_worker.load_uint8`'s bytes; a file Pillow refuses never comes back. The hand-written files are checked against Pillow on
the CPU in test_png_deep.py."""
import io
import os

import numpy as np
import pytest
from PIL import Image

from clipmi import png, png_parse
import png_cases
import png_deep_cases as D
import png_mode_cases as M
import ws_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ON = dict(modes=True, deep=True)


def _own_mode(blob):
    """what decode_files has to return, from Pillow: the file's own-mode pixels, 8-bit grey replicated"""
    a = np.asarray(Image.open(io.BytesIO(blob)))
    return np.repeat(a[..., None], 3, axis=2) if a.ndim == 2 else a


def _compare(files, got):
    handed_back = [name for (name, _), g in zip(files, got) if g is None]
    assert not handed_back, handed_back
    wrong = []
    for (name, b), g in zip(files, got):
        ref = _own_mode(b)
        if g.shape != ref.shape or not np.array_equal(g, ref):
            wrong.append((name, int((g != ref).sum()) if g.shape == ref.shape else (g.shape, ref.shape)))
    assert not wrong, wrong


def test_deep_decode_equals_pillow():
    """Widths on either side of the 4-unit step, heights on either side of a 64-row band, each filter on every row and the cycling
    modes, every zlib level, for colour types 2, 6 and 4 at depth 16 with low bytes that are noise: nothing handed back, every
    file Pillow's bytes. Without deep=True none of them comes back."""
    files = D.decode_cases(np.random.default_rng(320))
    assert len(files) == len(D.WIDTHS) * len(D.HEIGHTS) + 3 * (len(png_cases.MODES) + len(png_cases.LEVELS))
    assert {(b[24], b[25]) for _, b in files} == {(16, 2), (16, 6), (16, 4)}
    _compare(files, png.decode_files([b for _, b in files], DEV, **ON))
    assert all(g is None for g in png.decode_files([b for _, b in files], DEV, modes=True, interlaced=True, chunks=True))
    # colour type 2 needs no modes=True, the two others do
    few = files[:6]
    got = png.decode_files([b for _, b in few], DEV, deep=True)
    assert [g is not None for g in got] == [b[25] == 2 for _, b in few]


def test_adam7_deep_decode_equals_pillow():
    files = D.lace_cases(np.random.default_rng(321))
    assert len(files) == 64 + 3 and all(b[28] == 1 for _, b in files)
    _compare(files, png.decode_files([b for _, b in files], DEV, interlaced=True, **ON))
    assert all(g is None for g in png.decode_files([b for _, b in files], DEV, **ON))          # (not without interlaced=True)


def test_widest_rows():
    """65 rows of 49152 bytes - RGBA16 at 6144 pixels, RGB16 at 8192, LA16 at 12288: the band's last row fills the LDS row"""
    files = D.widest_cases(np.random.default_rng(322))
    assert [(b[25], int.from_bytes(b[16:20], "big"), int.from_bytes(b[20:24], "big")) for _, b in files] == [(2, 8192, 65), (6, 6144, 65), (4, 12288, 65)]
    _compare(files, png.decode_files([b for _, b in files], DEV, **ON))


@pytest.fixture(scope="module")
def transform_cases():
    rng = np.random.default_rng(323)
    return [(f"c{ctype}_{h}x{w}", D.deep_file(rng, ctype, h, w, k + j, ("cycle", 1, 2)[(k + j) % 3], lace=(k + j) % 4 == 3, level=(1, 6)[k % 2]))
            for j, ctype in enumerate(D.CTYPES) for k, (h, w) in enumerate(M.SIZES)]


@pytest.fixture(scope="module")
def transform_refs(transform_cases):
    return {n_px: [M.load_uint8_blob(b, n_px) for _, b in transform_cases] for n_px in (32, 224)}


@pytest.mark.parametrize("n_px", [32, 224])
def test_transform_equals_load_uint8(transform_cases, transform_refs, n_px):
    got = png.transform_files([b for _, b in transform_cases], n_px, DEV, interlaced=True, deep=True)
    handed_back = [name for (name, _), g in zip(transform_cases, got) if g is None]
    assert not handed_back, handed_back
    wrong = [(name, int((g != ref).sum())) for (name, _), g, ref in zip(transform_cases, got, transform_refs[n_px]) if not np.array_equal(g, ref)]
    assert not wrong, wrong
    assert all(g is None for g in png.transform_files([b for _, b in transform_cases[::5]], n_px, DEV, interlaced=True))


def test_the_committed_fixture():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_deep.npz"))
    n, n_px = int(d["n"]), int(d["n_px"])
    blobs = [d[f"file_{i}"].tobytes() for i in range(n)]
    got = png.decode_files(blobs, DEV, interlaced=True, chunks=True, **ON)
    out = png.transform_files(blobs, n_px, DEV, interlaced=True, chunks=True, deep=True)
    for i in range(n):
        px = d[f"px_{i}"]
        px = np.repeat(px[..., None], 3, axis=2) if px.ndim == 2 else px
        assert got[i] is not None and got[i].shape == px.shape and np.array_equal(got[i], px), i
        assert out[i] is not None and np.array_equal(out[i], d[f"out_{i}"]), i
    assert all(g is None for g in png.decode_files(blobs, DEV, modes=True, interlaced=True))


def test_corrupt_deep_files_never_return_pixels():
    """a cut stream, a flipped Adler-32, a filter byte 5 and a stream that inflates to the 8-bit file's scanlines: statuses 2, 4, 3,
    2 between good files, which keep Pillow's pixels; Pillow refuses each of the four"""
    rng = np.random.default_rng(324)
    for ctype in D.CTYPES:
        bad = D.corrupt_cases(rng, ctype)
        good = [D.deep_file(rng, ctype, 40, 50, k) for k in range(len(bad) + 1)]
        blobs = [b for pair in zip(good, [f for _, f, _ in bad]) for b in pair] + [good[-1]]
        for _, f, _ in bad:
            assert D.transform_ref(f, 32) is None
        items = [png_parse.parse(b, **ON) for b in blobs]
        _, _, status = png.decode_device(items, DEV)
        st = status.cpu().tolist()
        # (the cut stream: 2, or 1 where the zero bits behind its end happen to be read as an invalid code first)
        assert st[::2] == [0] * 5 and st[1] in (1, 2) and st[3::2] == [s for _, _, s in bad[1:]], (ctype, st)
        got = png.decode_files(blobs, DEV, **ON)
        assert [g is None for g in got] == [False, True] * len(bad) + [False]
        for g, b in zip(got[::2], blobs[::2]):
            assert np.array_equal(g, _own_mode(b))


def test_chunk_files_decode_to_the_chunk_free_pixels():
    """every chunk case the parser lets through, in front of and behind the image data: the pixels of the file without the chunk
    (host only: the device sees the same stream); a 16-bit RGB file with tRNS and a profile needs both switches"""
    rng = np.random.default_rng(325)
    base = D.base_image(rng, 37, 40)
    free = D.with_chunk(base, b"", "before")
    files = [(f"{name}_{where}", D.with_chunk(base, chunk, where)) for name, chunk in D.valid_chunks() + D.broken_zlib_chunks() + D.tolerated_shapes()
             for where in ("before", "after")]
    files += [(name, blob) for name, blob, _ in D.trns_cases(rng) if name.split("_")[1] in ("grey8", "rgb8") and name.split("_")[2] in ("2", "6")]
    got = png.decode_files([free] + [b for _, b in files], DEV, chunks=True)
    assert np.array_equal(got[0], _own_mode(free))
    _compare(files, got[1:])
    assert all(np.array_equal(g, got[0]) for g in got[1:1 + 2 * 30])
    marked = [png_parse.parse(b, chunks=True).chunks for _, b in files]
    off = png.decode_files([b for _, b in files], DEV)
    assert [g is None for g in off] == [bool(m) for m in marked] and sum(marked) > len(files) // 2
    s = D.samples16(rng, 2, 37, 40, 1)
    meta = D.C(b"iCCP", b"Display P3\0\0" + D.z(536)) + D.C(b"tRNS", b"\0\1\0\2\0\3")
    both = [D.write16(s, 2, before=meta), D.write16(s, 2, after=meta), D.write16(s, 2, lace=1, before=meta)]
    for kw, ok in ((dict(chunks=True, deep=True), [True, True, False]), (dict(chunks=True, deep=True, interlaced=True), [True] * 3),
                   (dict(deep=True, interlaced=True), [False] * 3), (dict(chunks=True, interlaced=True), [False] * 3)):
        got = png.decode_files(both, DEV, **kw)
        assert [g is not None for g in got] == ok, kw
        assert all(np.array_equal(g, D.high_bytes(s, 2)) for g in got if g is not None)
    for n_px in (32, 224):
        out = png.transform_files(both + [b for _, b in files[:8]], n_px, DEV, interlaced=True, chunks=True, deep=True)
        for g, b in zip(out, both + [b for _, b in files[:8]]):
            assert g is not None and np.array_equal(g, M.load_uint8_blob(b, n_px))


# ---- workspace independence (tests/ws_cases.py) for the records this adds -----------------------------------------------------------
def _deep_batch():
    rng = np.random.default_rng(326)
    P = lambda b: png_parse.parse(b, modes=True, interlaced=True, deep=True)  # noqa: E731
    good = [("rgb16", D.deep_file(rng, 2, 70, 37, 1)), ("rgba16", D.deep_file(rng, 6, 65, 22, 0)), ("la16 interlaced", D.deep_file(rng, 4, 19, 13, 2, lace=1)),
            ("rgb16 interlaced", D.deep_file(rng, 2, 33, 9, 1, lace=1)), ("rgba8", M.mode_file(rng, 6, 8, 21, 22, 1))]
    bad = D.corrupt_cases(rng, 6)
    out = []
    for k in range(4):
        out.append((good[k][0], P(good[k][1]), _own_mode(good[k][1]), good[k][1]))
        out.append((bad[k][0], P(bad[k][1]), None, None))
    out.append((good[4][0], P(good[4][1]), M.pillow_pixels(good[4][1])[1], good[4][1]))
    return out


def test_deep_decode_does_not_depend_on_its_workspace(clipmi, gpu):
    """clipmi_png_decode_px8 over 16-bit records, one file per status between good ones: the same statuses and the same bytes whatever
    the workspace, the output and the status tensor held on entry, guard bands intact, the good files Pillow's pixels"""
    from test_ws_decode_gpu import Decode
    batch = _deep_batch()
    d = Decode(clipmi, gpu, "png_px8", batch)
    assert [int(r["reserved"][0]) & 255 for r in d.recs] == [16] * 8 + [8]
    got = W.run_independent(d, d.outputs, d.ws_bytes, device=gpu, canon=d.canon)
    assert d.check(got) in ([2, 3, 4], [1, 2, 3, 4])            # (1: what the cut stream may give, see test_corrupt_deep_files_never_return_pixels)
