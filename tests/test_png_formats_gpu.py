"""Every PNG format the device decodes through the unfilter kernel's one pass walk (csrc/png.hip png_unfilter_passes), plain and
Adam7, at the sizes where a step, a byte or a band ends (tests/png_format_cases.py), against Pillow itself. No tolerance: every
file comes back with status 0 and exactly Pillow's pixels in the file's own mode. test_png_formats.py checks the list on the CPU."""
import numpy as np
import pytest

from clipmi import png
import png_format_cases as F

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Palette images with Transparency")]
DEV = "cuda:0"


def _equal(a, b):
    """two results of png.decode_files, bit for bit: arrays, or (indices, palette)"""
    if isinstance(a, tuple) or isinstance(b, tuple):
        return isinstance(a, tuple) and isinstance(b, tuple) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))
    return a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b)


def test_every_format_at_every_edge_equals_pillow():
    """The whole list in one call per decode entry: nothing handed back, every file Pillow's pixels. Then every seventh file alone:
    bit-equal to its result in the big batch, so a record's decode does not depend on its neighbours' formats."""
    files = F.cases()
    assert len(files) == 1960
    got = png.decode_files([b for _, b in files], DEV, **F.ON)
    handed_back = [name for (name, _), g in zip(files, got) if g is None]
    assert not handed_back, handed_back
    wrong = [name for (name, b), g in zip(files, got) if not F.same(g, b)]
    assert not wrong, wrong
    differs = []
    for (name, b), g in list(zip(files, got))[::7]:
        (alone,) = png.decode_files([b], DEV, **F.ON)
        if not _equal(alone, g):
            differs.append(name)
    assert not differs, differs
