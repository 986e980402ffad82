"""Writes tests/golden/png_cases.npz: about twenty small PNG files (Pillow's own encoder at several levels, L and RGB; files
from the writer and the bit-level DEFLATE writer of tests/png_cases.py) and the pixels PILLOW decodes them to -
`Image.open(...).convert("RGB")`. Run from the repository root:
    python tests/golden/make_png_golden.py
"""
import io
import os
import sys
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import png_cases  # noqa: E402


def files(rng):
    out = []
    for k, (h, w, ch) in enumerate([(1, 1, 3), (5, 7, 1), (37, 53, 3), (64, 64, 1), (65, 63, 3), (13, 150, 3), (130, 13, 1)]):
        a = (png_cases.smooth, png_cases.noise)[k % 2](rng, h, w, ch)
        buf = io.BytesIO()
        Image.fromarray(a[..., 0] if ch == 1 else a).save(buf, format="PNG", **[{"compress_level": 0}, {"compress_level": 1}, {}, {"optimize": True}][k % 4])
        out.append(buf.getvalue())
    for mode in png_cases.MODES:
        out.append(png_cases.write(png_cases.smooth(rng, 66, 45, 3 if mode != 3 else 1), mode, level=9))
    out.append(png_cases.write(png_cases.screenshot(rng, 120, 160, 3), "cycle1", strategy=zlib.Z_FIXED, wbits=9))
    out.append(png_cases.write(png_cases.smooth(rng, 20, 21, 3), "cycle", flush_every=7, idat=7))
    out += [b for _, b in png_cases.bit_writer_cases(rng)]
    return out


def main():
    blobs = files(np.random.default_rng(2026))
    arrays = {"n": np.array(len(blobs))}
    for i, b in enumerate(blobs):
        arrays[f"file_{i}"] = np.frombuffer(b, np.uint8)
        arrays[f"rgb_{i}"] = np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
    path = os.path.join(HERE, "png_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(blobs)} files, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
