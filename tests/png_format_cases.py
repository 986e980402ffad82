"""Every PNG format the device decodes, plain and Adam7, at the sizes where a step, a byte or a band ends: the list behind
test_png_formats.py and test_png_formats_gpu.py. No tests here.

The unfilter kernel walks every format through one pass loop (csrc/png.hip png_unfilter_passes); the per-feature tests each cover
their own formats at their own sizes. This list crosses all of them: the 14 (colour type, depth) pairs of the two decode entries,
each stored without interlace and with Adam7, at widths on both sides of the 4-unit step and of a byte at depths 1/2/4, and at
heights on both sides of the 64-row band (131 rows give the last Adam7 pass, 65 rows, a second band). The files come from the
writers of the per-feature case modules in their filter-cycling modes, so that all five filter types occur.
"""
import functools

import numpy as np

import png_cases
import png_deep_cases as D
import png_interlace_cases as A
import png_mode_cases as M

# (colour type, depth): clipmi_png_decode_rgb8's two, then clipmi_png_decode_px8's at depth <= 8 and at depth 16
FORMATS = [(0, 8), (2, 8), (6, 8), (4, 8), (3, 1), (3, 2), (3, 4), (3, 8), (0, 1), (0, 2), (0, 4), (2, 16), (6, 16), (4, 16)]
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 17, 33]
HEIGHTS = [1, 2, 9, 63, 64, 65, 131]
CYCLES = ("cycle", "cycle1", "cycle4")                         # png_cases.filters_for: every filter type in turn, from row 0, 1 or 4 on
ON = dict(modes=True, interlaced=True, deep=True)              # the parser's switches that let every file through


def one(rng, ctype, depth, lace, h, w, k):
    """a file of that format; k chooses the content and the filter cycle (the Adam7 writers cycle the filters of each pass
    themselves: png_interlace_cases.pass_filters)"""
    if depth == 16:
        return D.deep_file(rng, ctype, h, w, k, CYCLES[k % 3], lace=lace)
    if lace:
        return A.lace_file(rng, ctype, depth, h, w, k)
    if ctype in (0, 2) and depth == 8:
        return png_cases.write(A.samples_for(rng, ctype, depth, h, w, k)[0], CYCLES[k % 3])
    return M.mode_file(rng, ctype, depth, h, w, k, CYCLES[k % 3])


@functools.lru_cache(maxsize=None)
def cases(seed=330):
    """[(name, file)]: FORMATS x (plain, Adam7) x WIDTHS x HEIGHTS, all valid, all for the device with ON. Built once per process."""
    rng = np.random.default_rng(seed)
    out = []
    for ctype, depth in FORMATS:
        for lace in (0, 1):
            for w in WIDTHS:
                for h in HEIGHTS:
                    out.append((f"c{ctype}d{depth}{'_adam7' if lace else ''}_{h}x{w}", one(rng, ctype, depth, lace, h, w, len(out))))
    return out


def same(got, blob):
    """what png.decode_files returned for a file == Pillow's pixels in the file's own mode (and its palette)"""
    if blob[24] == 16:
        ref = D.pillow_pixels(blob)
        return got is not None and not isinstance(got, tuple) and got.shape == ref.shape and np.array_equal(got, ref)
    return A.same(got, blob)
