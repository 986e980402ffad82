"""Writes tests/golden/png_modes.npz: small PNG files of the modes `png_parse.parse(modes=True)` adds (RGBA, grey + alpha,
palette at depth 1/2/4/8 with and without tRNS, grey at depth 1/2/4; Pillow's own encoder and the writer of
tests/png_mode_cases.py), what PILLOW decodes them to (`convert("RGBA")` for files with alpha and low-depth grey files, the
indices and the palette for palette and 1-bit files) and what the reference's transform makes of them at n_px = 32
(decode_worker.load_uint8). Run from the repository root:
    python tests/golden/make_png_modes_golden.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import clipmi  # noqa: E402,F401
import png_mode_cases as M  # noqa: E402

N_PX = 32


def files(rng):
    out = []
    sizes = [(37, 70), (70, 37), (33, 33), (1, 5), (32, 32), (65, 40), (9, 100), (32, 77), (129, 17)]
    k = 0
    for name, ctype, depth, t in M.KINDS:
        for j in range(2):
            h, w = sizes[k % len(sizes)]
            out.append(M.mode_file(rng, ctype, depth, h, w, k, M.png_cases.MODES[k % 8], with_trns=t, level=(1, 6, 9, 0)[k % 4]))
            k += 1
    for what in ("RGBA", "LA", "P1", "P2", "P4", "P8", "P8t", "P4t", "1"):
        h, w = sizes[k % len(sizes)]
        out.append(M.pillow_mode_file(rng, what, h, w, k))
        k += 1
    return out


def main():
    warnings.simplefilter("ignore")
    blobs = files(np.random.default_rng(2027))
    arrays = {"n": np.array(len(blobs)), "n_px": np.array(N_PX)}
    for i, b in enumerate(blobs):
        kind, px = M.pillow_pixels(b)
        arrays[f"file_{i}"] = np.frombuffer(b, np.uint8)
        arrays[f"kind_{i}"] = np.array(kind)
        arrays[f"px_{i}"] = px
        if kind == "index":
            arrays[f"palette_{i}"] = M.pillow_palette(b)[0]
        arrays[f"out_{i}"] = M.load_uint8_blob(b, N_PX)
    path = os.path.join(HERE, "png_modes.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(blobs)} files, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
