"""The list of every PNG format x interlace x edge size (tests/png_format_cases.py) on the CPU: it is complete, the parser lets every
file through and Pillow opens every file. test_png_formats_gpu.py decodes it."""
import collections
import io
import zlib

import pytest
from PIL import Image

from clipmi import png_parse
import png_format_cases as F

pytestmark = pytest.mark.filterwarnings("ignore")


def test_the_list_is_complete():
    files = F.cases()
    assert len(F.FORMATS) == 14 and len(set(F.FORMATS)) == 14
    assert len(files) == 14 * 2 * len(F.WIDTHS) * len(F.HEIGHTS) == 1960 and len({name for name, _ in files}) == 1960
    per = collections.Counter((b[25], b[24], b[28]) for _, b in files)              # colour type, depth, interlace method of IHDR
    assert per == {(c, d, lace): 70 for c, d in F.FORMATS for lace in (0, 1)}, per
    sizes = collections.Counter((int.from_bytes(b[16:20], "big"), int.from_bytes(b[20:24], "big")) for _, b in files)
    assert sizes == {(w, h): 28 for w in F.WIDTHS for h in F.HEIGHTS}, sizes


def test_every_file_parses_for_its_entry():
    """no file of the list is refused with every switch on; 8-bit grey and RGB go to one decode entry, the other twelve formats to
    the other, and a record says what its file's header says"""
    px8 = 0
    filters = collections.defaultdict(set)                     # format -> the filter types of its files without interlace
    for name, b in F.cases():
        p = png_parse.parse(b, **F.ON)                         # (raises Unsupported for a file it does not let through)
        assert (p.ctype, p.depth, p.interlace) == (b[25], b[24], b[28]), name
        assert (p.width, p.height) == (int.from_bytes(b[16:20], "big"), int.from_bytes(b[20:24], "big")), name
        assert p.px8 == ((b[25], b[24]) not in ((0, 8), (2, 8))), name
        px8 += p.px8
        raw = zlib.decompressobj(-15).decompress(p.stream)
        assert len(raw) == p.raw_bytes(), name
        if not p.interlace:
            filters[(p.ctype, p.depth)] |= set(raw[::1 + p.row_bytes()])
    assert px8 == 12 * 140
    assert filters == {f: {0, 1, 2, 3, 4} for f in F.FORMATS}, filters


def test_pillow_opens_every_file():
    for name, b in F.cases():
        im = Image.open(io.BytesIO(b))
        im.load()
        assert im.size == (int.from_bytes(b[16:20], "big"), int.from_bytes(b[20:24], "big")), name
