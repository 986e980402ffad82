"""Progressive JPEG files on the device (csrc/jpeg.hip jpeg_progressive_kernel) against Pillow itself and the committed Pillow
pixels. The rule is the baseline decoder's: every file the device returns pixels for (status 0) gives exactly Pillow's
`convert("RGB")` bytes; a file Pillow refuses is never returned; anything else is handed back and Pillow decides."""
import collections
import io
import os

import numpy as np
import pytest
from PIL import Image, ImageFile

from clipmi import jpeg, jpeg_parse
import jpeg_progressive
from test_jpeg import smooth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_progressive_cases.npz")


@pytest.fixture(autouse=True)
def big_encode_buffer(monkeypatch):
    # Pillow's default encoder buffer is too small for progressive noise files of a few hundred pixels a side
    monkeypatch.setattr(ImageFile, "MAXBLOCK", 1 << 24)


def pillow(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def encode(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", progressive=True, **kw)
    return buf.getvalue()


def live_batch():
    rng = np.random.default_rng(31)
    blobs = []
    for (h, w) in [(5, 7), (8, 8), (17, 16), (37, 53), (13, 300), (300, 13), (100, 75), (64, 129), (224, 224), (480, 640)]:
        for sub in (0, 1, 2):
            for q in (95, 75, 30):
                blobs.append(encode(smooth(rng, h, w), quality=q, subsampling=sub))
                blobs.append(encode(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), quality=q, subsampling=sub))
    for q in (95, 75, 30):
        blobs.append(encode(np.full((1, 1, 3), 200, np.uint8), quality=q, subsampling=0))
        blobs.append(encode(smooth(rng, 37, 53)[..., 0], quality=q))
        blobs.append(encode(rng.integers(0, 256, (64, 96), dtype=np.uint8), quality=q))
    for sub in (0, 1, 2):
        blobs.append(encode(smooth(rng, 300, 200), quality=85, subsampling=sub, optimize=True))
        blobs.append(encode(smooth(rng, 1500, 2000), quality=85, subsampling=sub))
    blobs.append(encode(rng.integers(0, 256, (1500, 2000, 3), dtype=np.uint8), quality=90, subsampling=2))
    blobs.append(encode(np.zeros((16, 16, 3), np.uint8), quality=50))
    blobs.append(encode(smooth(rng, 300, 200)[..., 0], quality=85, optimize=True))
    blobs += [b for b, _ in jpeg_progressive.writer_cases(rng)]
    return blobs


def test_device_equals_pillow_live():
    blobs = live_batch()
    accepted = []
    for b in blobs:
        try:
            jpeg_parse.parse_progressive(b)
            accepted.append(b)
        except jpeg_parse.Unsupported:
            w, h = Image.open(io.BytesIO(b)).size
            assert (w + 1) // 2 <= 2, "only too-narrow subsampled files are refused here"
    assert len(accepted) >= 200
    got = jpeg.decode_progressive_files(accepted, DEV)
    for b, g in zip(accepted, got):
        assert g is not None
        assert np.array_equal(g, pillow(b))


def test_golden_files_decode_to_the_committed_pillow_pixels():
    d = np.load(GOLDEN)
    cases = [(d[f"file_{i}"].tobytes(), d[f"rgb_{i}"]) for i in range(int(d["n"]))]
    got = jpeg.decode_progressive_files([b for b, _ in cases], DEV)
    for (blob, rgb), g in zip(cases, got):
        assert g is not None and np.array_equal(g, rgb)


def test_batch_beside_baseline_layout():
    """A batch mixing samplings, grey and sizes: the records' offsets keep images apart, and a refused file in the middle of
    the list leaves the others' pixels in place."""
    rng = np.random.default_rng(5)
    blobs = [encode(smooth(rng, 40 + 7 * k, 30 + 5 * k), quality=80, subsampling=k % 3) for k in range(9)]
    b = io.BytesIO()
    Image.fromarray(smooth(rng, 20, 20)).save(b, format="JPEG", quality=80)           # baseline: not for this decoder
    blobs.insert(4, b.getvalue())
    got = jpeg.decode_progressive_files(blobs, DEV)
    assert got[4] is None
    for k, (blob, g) in enumerate(zip(blobs, got)):
        if k != 4:
            assert np.array_equal(g, pillow(blob))


def test_malformed_corpus_never_returns_wrong_pixels():
    """Seeded malformed files built here: bit flips and truncations inside individual scans, DHT mutations between scans,
    SOS parameter mutations, scans cut short before EOI, and writer files with EOB runs that overrun the scan and coefficient
    runs that overrun the band (every code valid). Every status-0 file equals Pillow; a file Pillow refuses never comes back
    with status 0."""
    corpus = jpeg_progressive.malformed_corpus(np.random.default_rng(77))
    blobs = [b for _, b in corpus]
    got = jpeg.decode_progressive_files(blobs, DEV)
    counts = collections.defaultdict(lambda: [0, 0, 0, 0])     # family -> [files, device pixels, handed back, Pillow refuses]
    for (fam, b), g in zip(corpus, got):
        c = counts[fam]
        c[0] += 1
        try:
            ref = pillow(b)
        except Exception:
            ref = None
        if ref is None:
            c[3] += 1
            assert g is None, f"{fam}: the device returned pixels for a file Pillow refuses"
        elif g is None:
            c[2] += 1
        else:
            c[1] += 1
            assert np.array_equal(g, ref), f"{fam}: status 0 with pixels that are not Pillow's"
    for fam, (n, ok, back, refused) in sorted(counts.items()):
        print(f"{fam:12s} files {n:5d}  device pixels {ok:5d}  handed back {back:5d}  Pillow refuses {refused:5d}")
    assert sum(c[1] for c in counts.values()) > 0 and sum(c[2] for c in counts.values()) > 0


def _progressive_pipeline_worker(tmp):
    """Own process, the product's start order (decode workers before the GPU). Progressive files of every sampling, grey and a
    photo-sized one beside baseline, PNG, CMYK and broken files, a progressive file whose data ends early (the device reports it,
    Pillow decides) and one with restart intervals (Pillow's)."""
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import torch
    import clipmi
    ImageFile.MAXBLOCK = 1 << 24
    rng = np.random.default_rng(41)
    paths, prog = [], []

    def put(name, img, **kw):
        p = os.path.join(tmp, name)
        img.save(p, **kw)
        paths.append(p)
        return p

    for i, (w, h, sub, q) in enumerate([(224, 224, 2, 95), (640, 480, 2, 85), (300, 500, 1, 90), (224, 300, 0, 75), (1600, 1200, 2, 80),
                                        (90, 70, 1, 60), (225, 223, 0, 92)]):
        a = smooth(rng, h, w) if i % 2 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        prog.append(put(f"p{i:02d}.jpg", Image.fromarray(a), quality=q, subsampling=sub, progressive=True))
    prog.append(put("p_grey.jpg", Image.fromarray(smooth(rng, 300, 260)[..., 0]), quality=85, progressive=True, optimize=True))
    put("p_rst.jpg", Image.fromarray(smooth(rng, 260, 300)), quality=85, progressive=True, restart_marker_blocks=5)
    for i in range(3):
        put(f"a{i}.jpg", Image.fromarray(smooth(rng, 240 + 30 * i, 320)), quality=85, subsampling=i)
    put("d.png", Image.fromarray(smooth(rng, 250, 350)))
    put("e_cmyk.jpg", Image.fromarray(smooth(rng, 240, 320)).convert("CMYK"), quality=85)
    cut = put("g_cut.jpg", Image.fromarray(smooth(rng, 320, 320)), quality=90, progressive=True)
    blob = open(cut, "rb").read()
    sos = [k for k in range(len(blob) - 1) if blob[k] == 0xFF and blob[k + 1] == 0xDA]
    open(cut, "wb").write(blob[:sos[-1] + (len(blob) - sos[-1]) // 2] + b"\xff\xd9")     # the last scan's data ends early
    bad = os.path.join(tmp, "h_broken.jpg")
    with open(bad, "wb") as f:
        f.write(b"broken")
    files = paths[:6] + [bad] + paths[6:]
    import warnings
    warnings.simplefilter("ignore")
    with clipmi.pipeline.DecodePool(3) as pool:
        assert not torch.cuda.is_initialized()
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        host = list(clipmi.pipeline.encode_files(model, files, batch=6, pool=pool, device_resize_mb=0, device_jpeg_kb=0))
        st_off, st_on, st_grp = {}, {}, {}
        off = list(clipmi.pipeline.encode_files(model, files, batch=6, pool=pool, device_resize_mb=0, device_jpeg_kb=2048, stats=st_off))
        on = list(clipmi.pipeline.encode_files(model, files, batch=6, pool=pool, device_resize_mb=0, device_jpeg_kb=2048, stats=st_on,
                                               device_progressive=True))
        grp = list(clipmi.pipeline.encode_files(model, files, batch=6, pool=pool, device_resize_mb=8, device_jpeg_kb=2048, stats=st_grp,
                                                device_progressive=True, jpeg_group_mb=1))
        os.environ["CLIPMI_DEVICE_PROGRESSIVE"] = "1"
        st_env = {}
        env = list(clipmi.pipeline.encode_files(model, files, batch=6, pool=pool, device_resize_mb=0, device_jpeg_kb=2048, stats=st_env))
        del os.environ["CLIPMI_DEVICE_PROGRESSIVE"]
    for other in (off, on, grp, env):
        assert [h[0] for h in host] == [d[0] for d in other] and [h[2] for h in host] == [d[2] for d in other]
        for h, d in zip(host, other):
            assert (h[1] is None and d[1] is None) or np.array_equal(h[1], d[1])
    failed = [p for h in host for p in h[2]]
    assert bad in failed
    assert st_off.get("jpeg_progressive_files", 0) == 0 and st_off["jpeg_files"] >= 3
    # The pipeline sizes its JPEG regions from the batches before (1.25 x the largest file held or turned away, at least 64 KB;
    # a file that does not fit goes to Pillow), and decode runs a batch ahead of that sizing: a file whose region needs at most
    # 64 KB always takes the device, a larger one may go to Pillow in a given call.
    from clipmi import decode_worker
    scratch = np.zeros(4 << 20, np.uint8)
    need = [decode_worker.stage_jpeg_progressive(p, 224, scratch)[2] for p in prog]
    sure = sum(1 for b in need if b <= 65536)
    assert sure >= 4
    for st in (st_on, st_grp, st_env):
        assert sure <= st["jpeg_progressive_files"] <= len(prog) + 1, st      # (+1: the cut file is staged, then reported)
        assert st["jpeg_files"] == st_off["jpeg_files"], st
    open(os.path.join(tmp, "ok"), "w").write("1")


def test_pipeline_progressive_on_device_gives_the_same_vectors(tmp_path):
    """encode_files(..., device_progressive=True) and CLIPMI_DEVICE_PROGRESSIVE=1 return the vectors and failed files of the
    all-Pillow path bit for bit, with the progressive files decoded on the device (stats["jpeg_progressive_files"])."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r}); " \
           f"import test_jpeg_progressive_gpu as t; t._progressive_pipeline_worker({str(tmp_path)!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "ok").read_text() == "1"
