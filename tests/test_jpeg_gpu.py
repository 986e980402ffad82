"""csrc/jpeg.hip against Pillow itself (the reference's decoder, build-index.py:47) and the committed Pillow pixels. The rule:
every file the device returns pixels for (status 0) gives exactly Pillow's `convert("RGB")` bytes; a file Pillow refuses is
never returned; anything else is handed back (Unsupported on the host, status != 0 from the device) and Pillow decides.
Well-formed files are returned, not handed back."""
import collections
import io

import numpy as np
import pytest
import torch
from PIL import Image

import clipmi
from clipmi import jpeg, jpeg_parse
from oracle import jpeg_oracle
import jpeg_corpus
from test_jpeg import encode, golden_cases, smooth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def pillow(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def test_golden_files_decode_to_the_committed_pillow_pixels():
    cases = golden_cases()
    got = jpeg.decode_files([b for b, _ in cases], DEV)
    for (blob, rgb), g in zip(cases, got):
        assert g is not None and np.array_equal(g, rgb)


def test_device_decode_equals_pillow_live():
    """One batch with every supported sampling x three qualities x smooth / noise content, odd sizes, an image of several
    chunks of subsequences (1 100 x 1 500), grey and optimised-table files, a 2 x 2-block image."""
    rng = np.random.default_rng(21)
    blobs = []
    for (h, w) in [(224, 224), (37, 53), (8, 8), (17, 16), (100, 75), (64, 129), (5, 7), (480, 640), (1100, 1500)]:
        for sub in (0, 1, 2):
            for q in (95, 75, 30):
                blobs.append(encode(smooth(rng, h, w), quality=q, subsampling=sub))
                if h * w < 100000:
                    blobs.append(encode(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), quality=q, subsampling=sub))
    blobs.append(encode(smooth(rng, 300, 200)[..., 0], quality=85, optimize=True))
    blobs.append(encode(smooth(rng, 300, 200), quality=85, optimize=True))
    blobs.append(encode(np.zeros((16, 16, 3), np.uint8), quality=50))
    for (h, w) in [(64, 96), (37, 53), (480, 640), (224, 224)]:         # restart intervals: 1 MCU, a few, a row of MCUs, many rows
        for sub in (0, 1, 2):
            for kw in (dict(restart_marker_blocks=1), dict(restart_marker_blocks=7), dict(restart_marker_rows=1), dict(restart_marker_rows=3)):
                a = smooth(rng, h, w) if (h + sub) % 2 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                blobs.append(encode(a, quality=88, subsampling=sub, **kw))
                assert jpeg_parse.parse(blobs[-1]).ri > 0
    got = jpeg.decode_files(blobs, DEV)
    raw = jpeg.decode_files(blobs, DEV, keep_stuffing=True)          # the pipeline's form: byte stuffing removed on the device
    assert sum(jpeg_parse.parse(b, keep_stuffing=True).stuffed for b in blobs) >= 140          # (not the restart-interval files)
    for b, g, r in zip(blobs, got, raw):
        assert g is not None and r is not None
        ref = pillow(b)
        assert np.array_equal(g, ref) and np.array_equal(r, ref)


def test_noise_image_of_many_subsequences_converges():
    """A noise image has no end-of-block symbols: the subsequences do not re-synchronise and the decode degenerates to the
    serial chain, one subsequence per round, across several chunks of 256 - same pixels."""
    rng = np.random.default_rng(22)
    blob = encode(rng.integers(0, 256, (400, 600, 3), dtype=np.uint8), quality=98, subsampling=0)
    assert len(jpeg_parse.parse(blob).stream) > 3 * 256 * 128
    (g,) = jpeg.decode_files([blob], DEV)
    assert np.array_equal(g, pillow(blob))


def test_corrupt_entropy_data_is_reported_or_decoded_as_pillow_does():
    rng = np.random.default_rng(23)
    blob = encode(smooth(rng, 96, 128), quality=85)
    p = jpeg_parse.parse(blob)
    short = jpeg_parse.parse(blob)
    short.stream = p.stream[:len(p.stream) // 2]                 # the data ends early
    out, recs, status = jpeg.decode_device([p, short], DEV)
    assert status.cpu().tolist() == [0, 2]
    start = blob.index(b"\xff\xda") + 14
    n_checked = 0
    for k in range(24):
        bad = bytearray(blob)
        pos = start + int(rng.integers(0, len(blob) - start - 4))
        bad[pos] ^= 1 << int(rng.integers(0, 8))
        bad = bytes(bad)
        try:
            q = jpeg_parse.parse(bad)
        except jpeg_parse.Unsupported:
            continue
        (g,) = jpeg.decode_files([bad], DEV)
        if g is None:
            continue                                             # reported: the file goes to Pillow
        ref = jpeg_corpus.pillow(bad)
        assert ref is not None, "the device returned pixels for a file Pillow refuses"
        assert np.array_equal(g, ref)
        n_checked += 1
    assert n_checked >= 4


def _decode_with_status(blobs, keep_stuffing):
    """-> [(status, pixels)] per file: status None where the host parser refuses the file, pixels only for status 0"""
    items, where = [], []
    for k, b in enumerate(blobs):
        try:
            items.append(jpeg_parse.parse(b, keep_stuffing=keep_stuffing))
            where.append(k)
        except jpeg_parse.Unsupported:
            pass
    res = [(None, None)] * len(blobs)
    if not items:
        return res
    out, recs, status = jpeg.decode_device(items, DEV)
    st = status.cpu().numpy()
    host = out.cpu().numpy()
    for t, k in enumerate(where):
        px = None
        if st[t] == 0:
            r = recs[t]
            h, w, o = int(r["height"]), int(r["width"]), int(r["out_off"])
            px = host[o:o + h * w * 3].reshape(h, w, 3)
        res[k] = (int(st[t]), px)
    return res


def test_malformed_corpus_is_reported_or_decoded_as_pillow_does():
    """The seeded corpus of malformed files (tests/jpeg_corpus.py: header bytes replaced, entropy-coded data damaged, forged
    headers) through the device, plain and with the stuffing left to the device: status 0 only with Pillow's exact pixels,
    never for a file Pillow refuses. The counts by family and status are printed (pytest -s)."""
    files = jpeg_corpus.corpus()
    refs = {}
    counts = collections.Counter()
    wrong = []
    for ks in (False, True):
        for lo in range(0, len(files), 4096):
            chunk = files[lo:lo + 4096]
            for k, (st, px) in enumerate(_decode_with_status([b for _, _, b in chunk], ks)):
                fam, name, blob = chunk[k]
                kind = ":".join(fam.split(":")[:2])
                counts[(kind, ks, "refused" if st is None else st)] += 1
                if fam == "a:DQT:body" and st is not None:   # intact data, new steps: the device reports where the oracle does
                    try:
                        jpeg_oracle.decode(blob)
                        reported = False
                    except jpeg_oracle.Reported:
                        reported = True
                    if reported != (st == 4):
                        wrong.append((fam, name, ks, f"status {st}, oracle reported: {reported}"))
                if st != 0:
                    continue
                if lo + k not in refs:
                    refs[lo + k] = jpeg_corpus.pillow(blob)
                ref = refs[lo + k]
                if ref is None or not np.array_equal(px, ref):
                    diff = "Pillow refuses" if ref is None else int(np.abs(px.astype(int) - ref.astype(int)).max())
                    wrong.append((fam, name, ks, diff))
    print("\nfamily, keep_stuffing: files by status (refused = the host parser hands the file to Pillow)")
    for kind in sorted({c[0] for c in counts}):
        for ks in (False, True):
            row = {st: n for (k_, ks_, st), n in counts.items() if k_ == kind and ks_ == ks}
            print(f"  {kind:22s} {str(ks):5s} " + " ".join(f"{st}={row[st]}" for st in sorted(row, key=str)))
    print(f"status 0 with pixels other than Pillow's: {len(wrong)}", wrong[:20])
    assert not wrong
    assert sum(n for (k_, ks_, st), n in counts.items() if k_ == "a:DQT" and st == 4) > 0
    assert sum(n for (k_, ks_, st), n in counts.items() if st == 0) > 20000


def test_marker_inside_a_stuffed_segment_is_reported():
    """A segment handed over with its stuffing is searched for markers on the device: 0xFF followed by anything but 0x00."""
    rng = np.random.default_rng(26)
    blob = encode(smooth(rng, 120, 160), quality=85)
    p = jpeg_parse.parse(blob, keep_stuffing=True)
    assert p.stuffed == 1 and p.stream.count(b"\xff\x00") > 0
    q = jpeg_parse.parse(blob, keep_stuffing=True)
    k = len(q.stream) // 2
    while q.stream[k - 1] == 0xFF or q.stream[k] == 0xFF:
        k += 1
    q.stream = q.stream[:k] + b"\xff\xd3" + q.stream[k + 2:]
    r = jpeg_parse.parse(blob, keep_stuffing=True)
    r.stream = r.stream[:-1] + b"\xff"                                  # a 0xFF with nothing behind it
    out, recs, status = jpeg.decode_device([p, q, r], DEV)
    assert status.cpu().tolist() == [0, 3, 3]
    (g,) = jpeg.decode_files([blob], DEV, keep_stuffing=True)
    assert np.array_equal(g, pillow(blob))


def test_restart_interval_that_ends_early_is_reported():
    rng = np.random.default_rng(25)
    blob = encode(smooth(rng, 96, 128), quality=85, restart_marker_rows=1)
    p = jpeg_parse.parse(blob)
    q = jpeg_parse.parse(blob)
    cut = int(q.starts[2])
    q.stream = q.stream[:cut - 40] + q.stream[cut:]                 # the second interval loses its last 40 bytes
    q.starts = np.concatenate([q.starts[:2], q.starts[2:] - 40]).astype(np.uint32)
    out, recs, status = jpeg.decode_device([p, q], DEV)
    st = status.cpu().tolist()
    assert st[0] == 0 and st[1] != 0


def test_decoded_pixels_feed_the_resize_kernel():
    """The decoder's output is the layout clipmi_resize_crop_rgb8 takes: decode + resize on the device equals the host
    transform's pixels (decode_worker.load_uint8 = Pillow decode + Pillow resize + crop)."""
    import os
    import tempfile
    from clipmi import resize
    from clipmi.decode_worker import load_uint8
    rng = np.random.default_rng(24)
    blobs = [encode(smooth(rng, h, w), quality=90, subsampling=s) for (h, w, s) in [(300, 400, 2), (224, 224, 2), (250, 224, 1), (500, 333, 0)]]
    imgs = jpeg.decode_files(blobs, DEV)
    got = resize.resize_crop_device(imgs, 224, DEV).cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        for k, b in enumerate(blobs):
            path = os.path.join(d, f"{k}.jpg")
            with open(path, "wb") as f:
                f.write(b)
            assert np.array_equal(got[k], load_uint8(path, 224))
