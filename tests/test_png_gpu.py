"""PNG files on the device (csrc/png.hip) against Pillow itself and the committed Pillow pixels. PNG is lossless, so there is no
tolerance: every file the device returns pixels for (status 0) gives exactly Pillow's `convert("RGB")` bytes; a file Pillow
refuses is never returned; anything else is handed back and Pillow decides."""
import collections
import io
import os

import numpy as np
import pytest
from PIL import Image

from clipmi import png, png_parse
import png_cases
from test_png import pillow, pillow_saved, save

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_cases.npz")


def live_batch():
    rng = np.random.default_rng(1)
    files = png_cases.writer_cases(rng) + pillow_saved(rng)
    files.append(("pillow_noise_480x640", save(Image.fromarray(png_cases.noise(rng, 480, 640)))))
    files.append(("pillow_smooth_1500x2000", save(Image.fromarray(png_cases.smooth(rng, 1500, 2000)), compress_level=1)))
    # the widest row the device takes (png_parse.MAX_WIDTH), more than one band: the band's last row fills the kernel's LDS row
    files.append(("widest_rgb", png_cases.write(png_cases.screenshot(rng, 66, png_parse.MAX_WIDTH, 3), "cycle1", level=1)))
    files.append(("widest_grey", png_cases.write(png_cases.screenshot(rng, 65, png_parse.MAX_WIDTH - 1, 1), 4, level=1)))
    return files


def test_device_equals_pillow_live():
    """Every valid file of the writer and the bit-level writer, and files Pillow's own encoder saved: none may be handed back,
    and all equal Pillow."""
    files = live_batch()
    assert len(files) >= 200
    blobs = [b for _, b in files]
    for name, b in files:
        png_parse.parse(b)                                     # (the parser lets every one of them through)
    got = png.decode_files(blobs, DEV)
    handed_back = [name for (name, _), g in zip(files, got) if g is None]
    assert not handed_back, handed_back
    for (name, b), g in zip(files, got):
        assert np.array_equal(g, pillow(b)), name


def test_golden_files_decode_to_the_committed_pillow_pixels():
    d = np.load(GOLDEN)
    cases = [(d[f"file_{i}"].tobytes(), d[f"rgb_{i}"]) for i in range(int(d["n"]))]
    assert len(cases) >= 20
    got = png.decode_files([b for b, _ in cases], DEV)
    for i, ((blob, rgb), g) in enumerate(zip(cases, got)):
        assert g is not None and np.array_equal(g, rgb), i


def test_batch_layout():
    """Nine files of mixed size and channels with an RGBA file and a corrupt file in the middle: the two come back None, the
    records' offsets keep the others apart and their pixels are intact."""
    rng = np.random.default_rng(5)
    blobs = [png_cases.write(png_cases.smooth(rng, 40 + 17 * k, 30 + 11 * k, 1 if k % 3 == 0 else 3), "cycle", level=(1, 6, 9)[k % 3])
             for k in range(9)]
    blobs.insert(4, save(Image.fromarray(png_cases.noise(rng, 20, 20, 4), "RGBA")))
    z = bytearray(png_cases.deflate(png_cases.filter_rows(png_cases.smooth(rng, 50, 50), [4] * 50)))
    z[len(z) // 2] ^= 0x10
    blobs.insert(5, png_cases.assemble(50, 50, 3, bytes(z)))
    with pytest.raises(Exception):
        pillow(blobs[5])
    got = png.decode_files(blobs, DEV)
    assert got[4] is None and got[5] is None
    for k, (blob, g) in enumerate(zip(blobs, got)):
        if k not in (4, 5):
            assert g is not None and np.array_equal(g, pillow(blob)), k


def test_malformed_corpus_never_returns_wrong_pixels():
    """Seeded malformed files (png_cases.malformed_corpus): every status-0 file equals Pillow; a file Pillow refuses never comes
    back with status 0; the files of the "harmless" family, which Pillow accepts, all come back from the device with pixels
    (so that handing everything back does not pass); a wrong Adler-32 is always handed back; the files of the "behind_idat"
    family, intact streams with a chunk behind the image data that makes Pillow refuse the file, never come back."""
    corpus = png_cases.malformed_corpus(np.random.default_rng(77))
    blobs = [b for _, b in corpus]
    got = png.decode_files(blobs, DEV)
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
        print(f"{fam:20s} files {n:5d}  device pixels {ok:5d}  handed back {back:5d}  Pillow refuses {refused:5d}")
    assert counts["harmless"][0] >= 26 and counts["harmless"][1] == counts["harmless"][0]
    assert counts["adler_wrong"][0] >= 8 and counts["adler_wrong"][1] == 0
    assert counts["behind_idat"][0] >= 10 and counts["behind_idat"][3] == counts["behind_idat"][0]
    assert len(counts) >= 19
