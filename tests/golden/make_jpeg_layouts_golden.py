"""Writes tests/golden/jpeg_layout_cases.npz: small forged JPEG files of the layouts jpeg_parse.parse(layouts=True) adds - luma
sampling 1x2, 4x1 and 1x4 and RGB-coded files, baseline (plain and with restart intervals) and progressive, a few per layout
(tests/jpeg_layouts.py forges them from Pillow files) - and the pixels PILLOW decodes them to, `Image.open(...).convert("RGB")`, run
in this container (Pillow 12.2.0, libjpeg-turbo). Run from the repository root:
    python tests/golden/make_jpeg_layouts_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import jpeg_layouts  # noqa: E402

# (form, layout, H, W, RGB-coded, noise)
CASES = [("baseline", "1x2", 9, 17, False, False), ("baseline", "1x2", 33, 47, False, False), ("baseline", "1x2", 1, 31, False, False),
         ("baseline", "1x2", 24, 40, False, True), ("baseline", "4x1", 13, 35, False, False), ("baseline", "4x1", 8, 63, False, False),
         ("baseline", "4x1", 16, 40, False, True), ("baseline", "1x4", 35, 13, False, False), ("baseline", "1x4", 63, 8, False, False),
         ("baseline", "1x4", 40, 16, False, True), ("baseline", "1x1", 40, 56, True, False), ("baseline", "2x2", 33, 47, True, False),
         ("baseline", "1x2", 33, 47, True, False), ("restart", "1x2", 33, 47, False, False), ("restart", "4x1", 13, 63, False, False),
         ("restart", "1x4", 63, 13, False, False), ("restart", "2x1", 20, 37, True, False),
         ("progressive", "1x2", 33, 47, False, False), ("progressive", "1x2", 100, 75, False, False),
         ("progressive", "4x1", 16, 96, False, False), ("progressive", "1x4", 96, 16, False, False),
         ("progressive", "1x1", 40, 56, True, False), ("progressive", "1x2", 9, 17, True, False)]


def main():
    rng = np.random.default_rng(73)
    d = {}
    for i, (form, layout, H, W, rgb, noise) in enumerate(CASES):
        kw = {"baseline": {}, "restart": dict(restart_marker_blocks=3), "progressive": dict(progressive=True)}[form]
        blob, _ = jpeg_layouts.forge(layout, H, W, rng, noise=noise, rgb=rgb, quality=(90, 70, 45)[i % 3], **kw)
        d[f"file_{i}"] = np.frombuffer(blob, np.uint8)
        d[f"rgb_{i}"] = jpeg_layouts.pillow(blob)
        assert d[f"rgb_{i}"].shape == (H, W, 3)
    d["n"] = np.array(len(CASES))
    d["names"] = np.array([f"{form} {layout}{' rgb' if rgb else ''}{' noise' if noise else ''} {H}x{W}" for form, layout, H, W, rgb, noise in CASES])
    np.savez_compressed(os.path.join(HERE, "jpeg_layout_cases.npz"), **d)
    print(len(CASES), "cases")


if __name__ == "__main__":
    main()
