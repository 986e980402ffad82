"""Writes tests/golden/png_deep.npz: small PNG files of depth 16 (colour types 2, 6 and 4, plain and Adam7; the writer of
tests/png_deep_cases.py) and 8-bit files that carry metadata chunks, what PILLOW opens them as (its own-mode pixels: RGB or RGBA
of the samples' high bytes) and what the reference's transform makes of them at n_px = 32 (decode_worker.load_uint8). Run from
the repository root:
    python tests/golden/make_png_deep_golden.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import clipmi  # noqa: E402,F401
import png_deep_cases as D  # noqa: E402
import png_mode_cases as M  # noqa: E402

N_PX = 32


def files(rng):
    out = []
    sizes = [(37, 40), (40, 37), (33, 33), (1, 5), (32, 32), (40, 9)]
    k = 0
    for ctype in D.CTYPES:
        for lace in (0, 1):
            h, w = sizes[k % len(sizes)]
            out.append(D.deep_file(rng, ctype, h, w, k, D.png_cases.MODES[(5 + k) % 8], lace=lace, level=(1, 6, 9)[k % 3]))
            k += 1
    out.append(D.deep_file(rng, 2, 5, 1, 0, 4))
    out.append(D.deep_file(rng, 6, 36, 35, 1, 3, before=D.C(b"iCCP", b"p\0\0" + D.z(300))))
    img = D.png_cases.smooth(rng, 38, 40, 3)
    chunks = dict(D.valid_chunks())
    out.append(D.png_cases.write(img, "cycle", before=chunks["screenshot"]))
    out.append(D.png_cases.write(D.png_cases.smooth(rng, 33, 35, 1), "cycle1", before=chunks["zTXt"] + D.C(b"tRNS", b"\0\x80")))
    out.append(D.with_chunk((40, 38, D.png_cases.deflate(D.png_cases.filter_rows(img, [4] * 38))), chunks["iTXt_compressed"] + chunks["eXIf"], "after"))
    return out


def main():
    warnings.simplefilter("ignore")
    blobs = files(np.random.default_rng(2029))
    arrays = {"n": np.array(len(blobs)), "n_px": np.array(N_PX)}
    for i, b in enumerate(blobs):
        arrays[f"file_{i}"] = np.frombuffer(b, np.uint8)
        arrays[f"px_{i}"] = np.asarray(D.Image.open(D.io.BytesIO(b)))
        arrays[f"out_{i}"] = M.load_uint8_blob(b, N_PX)
    path = os.path.join(HERE, "png_deep.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(blobs)} files, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
