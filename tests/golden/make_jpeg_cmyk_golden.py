"""Writes tests/golden/jpeg_cmyk_cases.npz: small four-component JPEG files - CMYK as stored, YCCK, without an Adobe marker, with
restart intervals, optimised tables, two quantisation tables and two Huffman table pairs, at component-0 sampling 1x1, 2x1 and 2x2
(tests/jpeg_cmyk.py writes them with Pillow's encoder and edits their headers) - with what PILLOW makes of them, run in this
container (Pillow 12.2.0, libjpeg-turbo): `np.asarray(Image.open(f))`, [H, W, 4] in mode CMYK, and the transform's bytes
`decode_worker.load_uint8(f, 32)`, [3, 32, 32]. Run from the repository root:
    python tests/golden/make_jpeg_cmyk_golden.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import jpeg_cmyk  # noqa: E402
from clipmi.decode_worker import load_uint8  # noqa: E402

N_PX = 32
# (form, Pillow's subsampling, H, W)
CASES = [("cmyk", 0, 1, 1), ("cmyk", 0, 8, 8), ("cmyk", 1, 17, 33), ("cmyk", 2, 45, 37), ("ycck", 0, 17, 33), ("ycck", 1, 45, 37),
         ("ycck", 2, 40, 33), ("no_adobe", 2, 17, 33), ("restart", 1, 45, 37), ("restart", 2, 40, 33), ("optimize", 2, 45, 37),
         ("two_quant", 1, 40, 33), ("two_huffman", 2, 45, 37)]


def main():
    rng = np.random.default_rng(89)
    d = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (form, sub, H, W) in enumerate(CASES):
            blob, _ = jpeg_cmyk.form_file(jpeg_cmyk.smooth4(rng, H, W), sub, form, quality=(90, 70, 45)[i % 3])
            path = os.path.join(tmp, f"{i}.jpg")
            with open(path, "wb") as f:
                f.write(blob)
            d[f"file_{i}"] = np.frombuffer(blob, np.uint8)
            d[f"cmyk_{i}"] = jpeg_cmyk.pillow4(blob)
            d[f"transform_{i}"] = load_uint8(path, N_PX)
            assert d[f"cmyk_{i}"].shape == (H, W, 4) and d[f"transform_{i}"].shape == (3, N_PX, N_PX)
    d["n"] = np.array(len(CASES))
    d["n_px"] = np.array(N_PX)
    d["names"] = np.array([f"{form} sub{sub} {H}x{W}" for form, sub, H, W in CASES])
    np.savez_compressed(os.path.join(HERE, "jpeg_cmyk_cases.npz"), **d)
    print(len(CASES), "cases")


if __name__ == "__main__":
    main()
