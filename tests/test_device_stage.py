"""device_stage's format table without a GPU: every row's group builder, run on regions the workers' stagers wrote, has to call its
C entry with the arguments in the prototype's order - the two builders serve eight entry / switch combinations, and a swapped
positional pointer would only show on the device. The library is replaced by a stand-in that records its calls; the argument counts
come from the real ctypes prototypes. Beside it: the groups DeviceStage cuts a kind's files into cover them once, in order, and
their statuses lie back to back."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from clipmi import decode_worker as dw
from clipmi import device_stage as ds
import png_cases
import png_mode_cases as M
from test_jpeg import smooth

N_PX, CAP = 224, 256 << 10
ENTRY = {(dw.KIND_BASELINE, False): "clipmi_jpeg_decode_rgb8", (dw.KIND_BASELINE, True): "clipmi_jpeg_decode_transform_rgb8",
         (dw.KIND_PROGRESSIVE, False): "clipmi_jpeg_decode_progressive_rgb8",
         (dw.KIND_PROGRESSIVE, True): "clipmi_jpeg_decode_progressive_transform_rgb8",
         (dw.KIND_PNG, False): "clipmi_png_decode_rgb8", (dw.KIND_PNG, True): "clipmi_png_decode_rgb8",
         (dw.KIND_PNG_ALPHA, False): "clipmi_png_decode_px8", (dw.KIND_PNG_ALPHA, True): "clipmi_png_decode_px8",
         (dw.KIND_PNG_INDEX, False): "clipmi_png_decode_px8", (dw.KIND_PNG_INDEX, True): "clipmi_png_decode_px8"}
WORKSPACE = {"clipmi_jpeg_decode_rgb8": "clipmi_jpeg_workspace_bytes", "clipmi_jpeg_decode_transform_rgb8": "clipmi_jpeg_workspace_bytes",
             "clipmi_jpeg_decode_progressive_rgb8": "clipmi_jpeg_progressive_workspace_bytes",
             "clipmi_jpeg_decode_progressive_transform_rgb8": "clipmi_jpeg_progressive_workspace_bytes",
             "clipmi_png_decode_rgb8": "clipmi_png_workspace_bytes", "clipmi_png_decode_px8": "clipmi_png_px8_workspace_bytes"}


class Recorder:
    """Stands in for the library: every attribute is a callable that stores (name, arguments) and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _jpeg(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", **kw)
    return buf.getvalue()


@pytest.fixture(scope="module")
def regions():
    """{kind: (the segment of 5 regions, the 3 slots that hold a staged file of that kind)}, staged once with the workers' stagers"""
    rng = np.random.default_rng(29)
    blobs = {dw.KIND_BASELINE: [_jpeg(smooth(rng, 64, 96), quality=85, subsampling=2), _jpeg(smooth(rng, 260, 300), quality=80, subsampling=0),
                                _jpeg(smooth(rng, 230, 225)[..., 0], quality=80)],
             dw.KIND_PROGRESSIVE: [_jpeg(smooth(rng, 64, 96), quality=85, subsampling=2, progressive=True),
                                   _jpeg(smooth(rng, 260, 300), quality=75, subsampling=1, progressive=True),
                                   _jpeg(smooth(rng, 230, 225)[..., 0], quality=80, progressive=True)],
             dw.KIND_PNG: [png_cases.write(png_cases.smooth(rng, 64, 96, 3), "cycle"), png_cases.write(png_cases.smooth(rng, 260, 300, 1), "cycle"),
                           png_cases.write(png_cases.smooth(rng, 230, 225, 3), "cycle")],
             dw.KIND_PNG_ALPHA: [M.pillow_mode_file(rng, what, h, w, k) for k, (what, h, w) in enumerate((("RGBA", 64, 96), ("LA", 260, 300), ("RGBA", 230, 225)))],
             dw.KIND_PNG_INDEX: [M.pillow_mode_file(rng, what, h, w, k) for k, (what, h, w) in enumerate((("P8", 64, 96), ("P4", 260, 300), ("1", 230, 225)))]}
    out = {}
    for kind in dw.PARSED:
        big = np.full(5 * CAP, 0xAB, np.uint8)
        slots = [0, 2, 3]                                              # (slots 1 and 4 hold no file: rows and slots differ)
        for slot, blob in zip(slots, blobs[kind.kind]):
            assert 0 < kind.stager(None, N_PX, big[slot * CAP:(slot + 1) * CAP], data=blob)[2] <= CAP
            assert big[slot * CAP:slot * CAP + 4].view(np.int32)[0] == kind.kind
        out[kind.kind] = (big, np.array(slots))
    return out


@pytest.mark.parametrize("fused", [False, True])
def test_every_row_calls_its_entry_with_the_prototypes_arguments(clipmi, regions, fused):
    real = clipmi._lib.lib()
    table = ds.formats(fused)
    assert set(table) == {k.kind for k in dw.PARSED}
    base, sb, rgb, status, ws, stream = 1 << 40, 1 << 30, 5 << 20, 6 << 20, 7 << 20, 8 << 20       # distinct stand-in addresses
    tr = ds.Transform(max_rows=77, n_px=N_PX, out=9 << 20, scratch=10 << 20)
    comp = np.array([0, -1, 1, 2, -1])
    for kind, fmt in table.items():
        big, slots = regions[kind]
        L = Recorder()
        r = fmt.records(big, 5, CAP, slots, comp, N_PX)
        arrays, out_sz, ws_bytes, name, decode = fmt.group(L, r)
        small, offs = ds._pack16(arrays)
        assert name == ENTRY[(kind, fused)] and (fmt.entry is None) == ("transform" in name)
        assert [c[0] for c in L.calls] == [WORKSPACE[name]] and ws_bytes == 0
        assert len(L.calls[0][1]) == len(getattr(real, WORKSPACE[name]).argtypes)
        assert decode(base, sb, offs, rgb, status, ws, stream, tr) == 0
        (called, args), = L.calls[1:]
        assert called == name                                         # the row's named entry, once
        assert len(args) == len(getattr(real, name).argtypes), name
        n = len(slots)
        recs, jobs = r[0], arrays[-1]
        assert len(recs) == n and len(jobs) == n and len(out_sz) == n and offs[0] == 0
        assert args[:3] == (base, sb, n)                              # the segment, the records at the packed buffer's start, the files
        assert args[-4:] == (status, ws, ws_bytes, stream)
        if name.startswith("clipmi_png"):
            raw_sz = r[3]
            assert args[3:6] == (int(raw_sz.sum()), int(raw_sz.max()), rgb) and len(arrays) == 2
            continue
        blocks, nt = r[-2], r[-1]
        assert blocks.shape == (n,) and nt >= 1 and np.array_equal(jobs["out_index"], comp[slots])
        if "progressive" in name:
            scans, tables = arrays[1], arrays[2]
            assert args[3:7] == (sb + offs[1], len(scans), sb + offs[2], nt) and len(scans) == int(recs["n_scans"].sum())
            rest = args[7:-4]
        else:
            tables = arrays[1]
            assert args[3:5] == (sb + offs[1], nt)
            rest = args[5:-4]
        assert tables.size == nt * clipmi.jpeg.TABLE_BYTES and small[offs[-2]:offs[-2] + tables.size].tobytes() == tables.tobytes()
        assert small[offs[-1]:offs[-1] + jobs.nbytes].tobytes() == jobs.tobytes()
        assert rest[:2] == (int(blocks.sum()), int(blocks.max()))
        if fused:                                                     # jobs, max_rows, the coefficients' base (the segment), n_px, out, scratch
            assert rest[2:] == (sb + offs[-1], tr.max_rows, base, N_PX, tr.out, tr.scratch)
        else:                                                         # the largest image's pixels, the full-size rows
            assert rest[2:] == (int((recs["width"].astype(np.int64) * recs["height"]).max()), rgb)


def test_groups_cover_every_file_once_in_order_with_contiguous_statuses(clipmi, regions):
    for fused in (False, True):
        for kind, fmt in ds.formats(fused).items():
            big, slots = regions[kind]
            hd = ds._headers(big, 5, CAP, slots)
            need = ds.file_need(hd, fmt, N_PX)
            for budget, n_groups in ((int(need.max()), None), (1, 3), (1 << 40, 1)):
                groups = ds._groups(need, budget)
                assert n_groups is None or len(groups) == n_groups
                assert groups[0][0] == 0 and groups[-1][1] == len(slots) and all(lo < hi for lo, hi in groups)
                assert all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
                stage = ds.DeviceStage(None, torch.device("cpu"), None, N_PX, budget, ds.formats(fused))
                launch = stage._stage_kind(fmt, big, 5, CAP, slots, np.array([0, -1, 1, 2, -1]), 7)
                assert [c.n_files for c in launch.calls] == [hi - lo for lo, hi in groups]
                at = 4 * 7
                for c in launch.calls:                                # each group's statuses start where the one before ended
                    assert c.status_off == at
                    at += 4 * c.n_files
                assert at == 4 * (7 + len(slots))
                assert (launch.rgb is None) == (fmt.entry is None) and launch.fmt is fmt
