"""Writes tests/golden/jpeg_progressive_cases.npz: small progressive JPEG files (Pillow's own scripts for every sampling the
device decoder takes, grey, odd sizes, optimised tables; writer scripts from tests/jpeg_progressive.py) and the pixels PILLOW
decodes them to - `Image.open(...).convert("RGB")`. Run from the repository root:
    python tests/golden/make_jpeg_progressive_golden.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image, ImageFile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_progressive  # noqa: E402
from test_jpeg import smooth  # noqa: E402


def files(rng):
    out = []
    for (h, w) in [(37, 53), (8, 8), (17, 16), (5, 7), (64, 129)]:
        for sub in (0, 1, 2):
            q = (95, 75, 30)[(h + sub) % 3]
            a = smooth(rng, h, w) if (h + w + sub) % 2 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            buf = io.BytesIO()
            Image.fromarray(a).save(buf, format="JPEG", quality=q, subsampling=sub, progressive=True)
            out.append(buf.getvalue())
    for a, kw in [(smooth(rng, 45, 61)[..., 0], dict(quality=85)), (smooth(rng, 45, 61), dict(quality=85, optimize=True)),
                  (np.full((1, 1, 3), 90, np.uint8), dict(quality=90, subsampling=0))]:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", progressive=True, **kw)
        out.append(buf.getvalue())
    out += [b for b, _ in jpeg_progressive.writer_cases(rng, big=False)[::2]]
    return out


def main():
    ImageFile.MAXBLOCK = 1 << 24
    blobs = files(np.random.default_rng(2026))
    arrays = {"n": np.array(len(blobs))}
    for i, b in enumerate(blobs):
        arrays[f"file_{i}"] = np.frombuffer(b, np.uint8)
        arrays[f"rgb_{i}"] = np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
    path = os.path.join(HERE, "jpeg_progressive_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(blobs)} files, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
