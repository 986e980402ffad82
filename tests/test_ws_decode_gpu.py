"""-m gpu: the decoders and the transforms give the same statuses and the same pixels whatever their workspace, their scratch rows,
their output and their STATUS tensor held on entry (tests/ws_cases.py: the table and the harness) - DeviceStage.run hands them a
status tensor of torch.empty where the wrappers the other tests call hand over zeros. Every batch puts one file per status the entry
can report between good files of mixed samplings: a reported file must leave its neighbours' pixels and everything outside its own
block alone. Statuses equal the wrapper's; pixels of status-0 files equal Pillow's. The header leaves a reported file's own block and
the padding between images unspecified: those bytes are blanked before the runs are compared.

Then DeviceStage._launch_kind's loop: two groups of one kind through ONE workspace, ONE buffer of decoded rows and ONE status tensor
(at different status offsets), the workspace sized for the larger group - in both orders."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_layouts as jl
import png_cases
import png_mode_cases as M
import ws_cases as W

pytestmark = pytest.mark.gpu

N_PX = 224
_cache = {}


def _pil(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


# ---- the batches ------------------------------------------------------------------------------------------------------------
def _baseline_batch(clipmi, second=False):
    """[(label, record, Pillow's pixels or None for a file built to be reported, the file)]: 4:2:0 with restart intervals, 4:4:4
    that keeps its byte stuffing, a forged 4:4:0 file (layouts=True), grey; between them a marker inside a stuffed segment (3),
    a segment cut in the middle (2), sixteen one-bits in a row (1: no Huffman code is all ones) and steps of 255 under noise (4).
    second: a smaller all-good batch of other samplings (4:2:2, 4:1:1 forged, RGB-coded)."""
    P = clipmi.jpeg_parse.parse
    rng = np.random.default_rng(501 + second)
    if second:
        files = [("4:2:2", jl.encode(jl.smooth(rng, 90, 150), quality=80, subsampling=1), {}),
                 ("4:1:1 forged", jl.forge("4x1", 64, 96, rng)[0], {}),
                 ("RGB-coded", jl.forge("1x1", 75, 61, rng, rgb=True)[0], {}),
                 ("4:2:0 stuffed", jl.encode(jl.smooth(rng, 50, 70), quality=90, subsampling=2), dict(keep_stuffing=True))]
        return [(name, P(b, layouts=True, **kw), _pil(b), b) for name, b, kw in files]
    a = jl.encode(jl.smooth(rng, 200, 320), quality=85, subsampling=2, restart_marker_rows=1)
    b = jl.encode(jl.smooth(rng, 123, 77), quality=85, subsampling=0)
    c = jl.forge("1x2", 120, 88, rng)[0]
    d = jl.encode(jl.smooth(rng, 65, 130)[..., 0], quality=80)
    n = jl.encode(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), quality=95, subsampling=0)
    pa, pb, pc, pd = P(a), P(b, keep_stuffing=True), P(c, layouts=True), P(d)
    assert pa.ri and pb.stuffed == 1 and pb.stream.count(b"\xff\x00") > 0 and clipmi.jpeg_parse.is_layout(pc) and pd.ncomp == 1
    s3 = P(b, keep_stuffing=True)
    k = len(s3.stream) // 2
    while s3.stream[k - 1] == 0xFF or s3.stream[k] == 0xFF:
        k += 1
    s3.stream = s3.stream[:k] + b"\xff\xd3" + s3.stream[k + 2:]
    s2 = P(jl.encode(jl.smooth(rng, 96, 128), quality=85, subsampling=2))
    s2.stream = s2.stream[:len(s2.stream) // 2]
    s1 = P(jl.encode(jl.smooth(rng, 80, 112), quality=85, subsampling=1))
    k = len(s1.stream) // 3
    s1.stream = s1.stream[:k] + b"\xff" * 16 + s1.stream[k + 16:]
    s4 = P(n)
    s4.quant = np.full_like(s4.quant, 255)
    return [("4:2:0 restart rows", pa, _pil(a), a), ("marker in a stuffed segment", s3, None, None), ("4:4:4 stuffed", pb, _pil(b), b),
            ("segment cut short", s2, None, None), ("4:4:0 forged", pc, _pil(c), c), ("sixteen one-bits", s1, None, None),
            ("grey", pd, _pil(d), d), ("steps of 255", s4, None, None)]


def _progressive_batch(clipmi, second=False):
    P = clipmi.jpeg_parse.parse_progressive
    rng = np.random.default_rng(511 + second)
    if second:
        files = [("4:2:2", jl.encode(jl.smooth(rng, 90, 150), quality=80, subsampling=1, progressive=True)),
                 ("grey", jl.encode(jl.smooth(rng, 50, 70)[..., 0], quality=90, progressive=True)),
                 ("RGB-coded", jl.forge("1x1", 75, 61, rng, rgb=True, progressive=True)[0])]
        return [(name, P(b, layouts=True), _pil(b), b) for name, b in files]
    a = jl.encode(jl.smooth(rng, 200, 320), quality=85, subsampling=2, progressive=True)
    b = jl.encode(jl.smooth(rng, 123, 77), quality=85, subsampling=0, progressive=True)
    c = jl.forge("1x2", 120, 88, rng, progressive=True)[0]
    d = jl.encode(jl.smooth(rng, 96, 128), quality=75, subsampling=1, progressive=True)
    n = jl.encode(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), quality=95, subsampling=0, progressive=True)
    s2 = P(d)
    s2.scans[1].stream = s2.scans[1].stream[:len(s2.scans[1].stream) // 2]
    s1 = P(b)
    big = max(range(len(s1.scans)), key=lambda i: len(s1.scans[i].stream))
    k = len(s1.scans[big].stream) // 3
    s1.scans[big].stream = s1.scans[big].stream[:k] + b"\xff" * 16 + s1.scans[big].stream[k + 16:]
    s4 = P(n)
    s4.quant = np.full_like(s4.quant, 255)
    return [("4:2:0", P(a), _pil(a), a), ("a scan cut short", s2, None, None), ("4:4:4", P(b), _pil(b), b),
            ("sixteen one-bits", s1, None, None), ("4:4:0 forged", P(c, layouts=True), _pil(c), c), ("steps of 255", s4, None, None),
            ("4:2:2", P(d), _pil(d), d)]


def _png_bad(rng, build):
    """one file per status of the stream itself: invalid DEFLATE (1), ended early (2), a filter byte of 7 (3), a wrong Adler-32 (4)"""
    import struct
    import zlib
    raw, w, h, ch = build(rng)
    z = png_cases.deflate(raw)
    bad = bytearray(raw)
    bad[(h // 2) * (len(raw) // h)] = 7
    return [("block type 3", (w, h, ch, z[:2] + bytes([z[2] | 6]) + z[3:])),      # BTYPE of the first block: the reserved value
            ("stream cut short", (w, h, ch, z[:len(z) // 2])), ("filter byte 7", (w, h, ch, png_cases.deflate(bytes(bad)))),
            ("Adler-32 + 1", (w, h, ch, z[:-4] + struct.pack(">I", (zlib.adler32(raw) + 1) & 0xffffffff)))]


def _png_rgb_batch(clipmi, second=False):
    P = clipmi.png_parse.parse
    rng = np.random.default_rng(521 + second)
    if second:
        files = [("rgb stored", png_cases.write(png_cases.noise(rng, 21, 22, 3), 0, level=0)), ("grey Paeth", png_cases.write(png_cases.smooth(rng, 65, 64, 1), 4)),
                 ("rgb Sub", png_cases.write(png_cases.screenshot(rng, 63, 100, 3), 1, level=1))]
        return [(name, P(b), _pil(b), b) for name, b in files]
    good = [("rgb every filter", png_cases.write(png_cases.smooth(rng, 300, 260, 3), "cycle", level=6)),
            ("grey", png_cases.write(png_cases.smooth(rng, 64, 90, 1), "cycle1", level=9)),
            ("rgb stored blocks", png_cases.write(png_cases.noise(rng, 37, 70, 3), "cycle4", level=0)),
            ("screenshot", png_cases.write(png_cases.screenshot(rng, 129, 300, 3), 4, level=9))]

    def build(rng):
        img = png_cases.smooth(rng, 40, 50, 3)
        return png_cases.filter_rows(img, png_cases.filters_for("cycle", 40)), 50, 40, 3
    bad = [(name, png_cases.assemble(*b)) for name, b in _png_bad(rng, build)]
    out = []
    for k in range(4):
        out.append((good[k][0], P(good[k][1]), _pil(good[k][1]), good[k][1]))
        out.append((bad[k][0], P(bad[k][1]), None, None))
    return out


def _png_px8_batch(clipmi, second=False):
    P = lambda b: clipmi.png_parse.parse(b, modes=True)  # noqa: E731
    rng = np.random.default_rng(531 + second)
    if second:
        files = [("la", M.mode_file(rng, 4, 8, 33, 47, 1)), ("p1", M.mode_file(rng, 3, 1, 50, 70, 2)), ("g4", M.mode_file(rng, 0, 4, 21, 22, 3))]
        return [(name, P(b), M.pillow_pixels(b)[1], b) for name, b in files]
    good = [("rgba", M.mode_file(rng, 6, 8, 70, 37, 0)), ("p8 of 77 entries", M.mode_file(rng, 3, 8, 64, 90, 1, entries=77)),
            ("p4 + tRNS", M.mode_file(rng, 3, 4, 40, 51, 2, with_trns=True)), ("g2", M.mode_file(rng, 0, 2, 33, 33, 3))]

    def build(rng):
        s, _ = M.samples_for(rng, 6, 8, 40, 50, 1)
        return M.scanlines(s, 6, 8, "cycle"), 50, 40, 4
    bad = [(name, png_cases.assemble(*b, ctype=6)) for name, b in _png_bad(rng, build)]
    idx = rng.integers(0, 256, (30, 40, 1), dtype=np.uint8)
    idx[7, 9] = 200
    bad.append(("index beyond the palette", M.write(idx, 3, 8, palette=rng.integers(0, 256, (100, 3), dtype=np.uint8))))
    out = []
    for k in range(5):
        if k < 4:
            out.append((good[k][0], P(good[k][1]), M.pillow_pixels(good[k][1])[1], good[k][1]))
        out.append((bad[k][0], P(bad[k][1]), None, None))
    return out


# ---- the calls --------------------------------------------------------------------------------------------------------------
class Decode:
    """One decode entry over a batch: call(ws, pixels, status) re-uploads the records and streams (the baseline entry rewrites
    both), then calls the entry. status_off / its own window of a shared status tensor: see run_after."""

    def __init__(self, clipmi, gpu, kind, batch, status_off=0):
        J, PN, lib = clipmi.jpeg, clipmi.png, clipmi._lib
        self.lib, self.L, self.gpu, self.kind, self.batch, self.status_off = lib, lib.lib(), gpu, kind, batch, status_off
        items = [it for _, it, _, _ in batch]
        self.n = n = len(items)
        if kind in ("baseline", "progressive"):
            packed = (J.pack if kind == "baseline" else J.pack_progressive)(items, layouts=True)
            *arrays, streams, self.out_bytes, blocks, max_blocks, max_pixels = packed
            self.recs = arrays[0]
            self.px = 3
            self.entry = "clipmi_jpeg_decode_rgb8" if kind == "baseline" else "clipmi_jpeg_decode_progressive_rgb8"
            self.ws_bytes = int(self.L.clipmi_jpeg_workspace_bytes(blocks, len(arrays[-1])) if kind == "baseline" else
                                self.L.clipmi_jpeg_progressive_workspace_bytes(n, blocks, len(arrays[-1])))
            self.dev, offs, self.host = lib.to_device16(arrays + [streams], gpu)
            base = self.dev.data_ptr()
            head = [base + offs[-1], base + offs[0], n]
            for a, o in zip(arrays[1:], offs[1:-1]):
                head += [base + o, len(a)]
            self.args = head + [blocks, max_blocks, max_pixels]
            self.wrapper = lambda: (J.decode_device if kind == "baseline" else J.decode_progressive_device)(items, gpu, layouts=True)
        else:
            self.recs, streams, self.out_bytes, total_raw, max_raw = PN.pack(items)
            self.entry = "clipmi_png_decode_rgb8" if kind == "png" else "clipmi_png_decode_px8"
            self.ws_bytes = int((self.L.clipmi_png_workspace_bytes if kind == "png" else self.L.clipmi_png_px8_workspace_bytes)(n, total_raw))
            self.dev, offs, self.host = lib.to_device16([self.recs, streams], gpu)
            base = self.dev.data_ptr()
            self.args = [base + offs[1], base, n, total_raw, max_raw]
            self.wrapper = lambda: PN.decode_device(items, gpu)
        self.sizes = [int(r["width"]) * int(r["height"]) * (PN.PX_BYTES[it.kind] if kind.startswith("png") else 3)
                      for r, it in zip(self.recs, items)]
        self.outputs = [("pixels", max(self.out_bytes, 16)), ("status", 4 * n)]

    def __call__(self, ws, pixels, status):
        self.dev.copy_(self.host, non_blocking=True)
        rc = getattr(self.L, self.entry)(*self.args, pixels.data_ptr(), status.data_ptr() + self.status_off, ws.data_ptr(), self.ws_bytes,
                                         self.lib.stream_ptr(self.gpu))
        self.lib.check(rc, self.entry)

    def canon(self, d):
        """blank what is unspecified: the padding between the images' rows and the rows of a reported file"""
        st = d["status"][self.status_off:self.status_off + 4 * self.n].view(np.int32)
        keep = np.zeros(d["pixels"].size, bool)
        for r, nb, s in zip(self.recs, self.sizes, st):
            if s == 0:
                keep[int(r["out_off"]):int(r["out_off"]) + nb] = True
        d["pixels"][~keep] = 0
        return d

    def check(self, got):
        """statuses: the wrapper's, 0 exactly for the files built to be good, every status the batch was built for; pixels: Pillow's"""
        st = got["status"].view(np.int32)
        _, _, wst = self.wrapper()
        assert st.tolist() == wst.cpu().tolist()[:self.n], (st.tolist(), wst.cpu().tolist())
        good = [ref is not None for _, _, ref, _ in self.batch]
        assert [s == 0 for s in st] == good, [(name, int(s)) for (name, _, _, _), s in zip(self.batch, st)]
        assert sum(good) >= (4 if len(good) > 4 else len(good))
        for (name, it, ref, _), r, nb, s in zip(self.batch, self.recs, self.sizes, st):
            if s == 0:
                px = got["pixels"][int(r["out_off"]):int(r["out_off"]) + nb]
                assert np.array_equal(px.reshape(ref.shape), ref), f"{self.kind}: '{name}' differs from Pillow"
        return sorted({int(s) for s in st if s})


BATCHES = {"baseline": (_baseline_batch, [1, 2, 3, 4]), "progressive": (_progressive_batch, [1, 2, 4]), "png": (_png_rgb_batch, [1, 2, 3, 4]),
           "png_px8": (_png_px8_batch, [1, 2, 3, 4, 5])}


def _batch(clipmi, kind, second=False):
    if (kind, second) not in _cache:
        _cache[kind, second] = BATCHES[kind][0](clipmi, second)
    return _cache[kind, second]


@pytest.mark.parametrize("kind", sorted(BATCHES))
def test_decode_entries(clipmi, gpu, kind):
    d = Decode(clipmi, gpu, kind, _batch(clipmi, kind))
    assert 5 <= d.n <= 9
    got = W.run_independent(d, d.outputs, d.ws_bytes, device=gpu, canon=d.canon)
    assert d.check(got) == BATCHES[kind][1]


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("kind", sorted(BATCHES))
def test_two_groups_share_workspace_rows_and_status_tensor(clipmi, gpu, kind, order):
    """_launch_kind: the batch with reported files, then a smaller all-good one with other samplings - through one workspace
    (sized for the larger), one buffer of decoded rows and one status tensor, the second group's statuses behind the first's"""
    first, second = Decode(clipmi, gpu, kind, _batch(clipmi, kind)), Decode(clipmi, gpu, kind, _batch(clipmi, kind, True))
    seq = [first, second] if order == "forward" else [second, first]
    last = seq[1]
    alone = W.run_independent(last, last.outputs, last.ws_bytes, device=gpu, canon=last.canon)
    last.check(alone)
    expect = {"pixels": last.canon({k: v.copy() for k, v in alone.items()})["pixels"], "status": (4 * seq[0].n, alone["status"])}
    last.status_off = 4 * seq[0].n                    # from here on the group's statuses lie behind the other group's
    outputs = [("pixels", max(first.outputs[0][1], second.outputs[0][1])), ("status", 4 * (first.n + second.n))]
    got = W.run_after([seq[0]], last, outputs, max(first.ws_bytes, second.ws_bytes), expect, device=gpu, canon=last.canon)
    # the earlier group's statuses are still its own: the later call wrote its window of the tensor only
    _, _, wst = seq[0].wrapper()
    assert got["status"][:4 * seq[0].n].view(np.int32).tolist() == wst.cpu().tolist()[:seq[0].n]


# ---- the transforms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["baseline", "progressive"])
def test_decode_transform_entries(clipmi, gpu, kind):
    """clipmi_jpeg_decode_transform_rgb8 / _progressive_transform_rgb8: the same batches straight to the transform's pixels; the
    scratch rows between the two resize passes are a third buffer of arbitrary contents"""
    J, lib, L = clipmi.jpeg, clipmi._lib, clipmi._lib.lib()
    batch = _batch(clipmi, kind)
    st = J.stage_transform([it for _, it, _, _ in batch], N_PX, gpu, layouts=True)
    (g,), (host,) = st.groups, st.keep
    n = g["n"]
    base, o = g["dev"].data_ptr(), g["offs"]
    head = (base + o[-1], base, n) + ((base + o[1], g["nscans"], base + o[2]) if g["progressive"] else (base + o[1],))
    head += (g["ntables"], g["total_blocks"], g["max_blocks"], base + o[-3], g["max_rows"], base + o[-2], N_PX)
    name = "clipmi_jpeg_decode_progressive_transform_rgb8" if g["progressive"] else "clipmi_jpeg_decode_transform_rgb8"
    block = 3 * N_PX * N_PX

    def call(ws, pixels, status, scratch):
        g["dev"].copy_(host, non_blocking=True)
        lib.check(getattr(L, name)(*head, pixels.data_ptr(), scratch.data_ptr(), status.data_ptr(), ws.data_ptr(), g["ws_bytes"],
                                   lib.stream_ptr(gpu)), name)

    def canon(d):
        d["scratch"][:] = 0
        for k, s in enumerate(d["status"].view(np.int32)):
            if s != 0:
                d["pixels"][k * block:(k + 1) * block] = 0
        return d
    got = W.run_independent(call, [("pixels", n * block), ("status", 4 * n), ("scratch", g["scratch"].numel())], g["ws_bytes"],
                            device=gpu, canon=canon)
    stt = got["status"].view(np.int32)
    wout, wst = J.run_transform(st, fused=True)
    assert stt.tolist() == wst.cpu().tolist()
    assert [s == 0 for s in stt] == [ref is not None for _, _, ref, _ in batch]
    assert sorted({int(s) for s in stt if s}) == BATCHES[kind][1] and (stt == 0).sum() >= 4
    for k, (label, _, ref, blob) in enumerate(batch):
        if stt[k] == 0:
            assert np.array_equal(got["pixels"][k * block:(k + 1) * block].reshape(3, N_PX, N_PX), M.load_uint8_blob(blob, N_PX)), label


SHAPES = [(300, 260), (224, 224), (225, 223), (37, 70), (70, 37), (224, 320)]


@pytest.mark.parametrize("px", [3, 4], ids=["rgb8", "rgba8"])
def test_resize_crop_entries(clipmi, gpu, px):
    """clipmi_resize_crop_rgb8 / _rgba8: the scratch rows between the passes ARE the workspace. Up- and downscaling, one side
    already n_px, neither"""
    lib, L = clipmi._lib, clipmi._lib.lib()
    rng = np.random.default_rng(541 + px)
    if px == 3:
        blobs = [png_cases.write(png_cases.smooth(rng, h, w, 3), "cycle") for h, w in SHAPES]
        imgs = [_pil(b) for b in blobs]
    else:
        blobs = [M.mode_file(rng, 6, 8, h, w, k) for k, (h, w) in enumerate(SHAPES)]
        imgs = [M.pillow_pixels(b)[1] for b in blobs]
    jobs, coef, raw_bytes, scratch_bytes, max_rows = clipmi.resize.pack_jobs([a.shape[:2] for a in imgs], N_PX, px=px)
    assert {(int(j["need_h"]), int(j["need_v"])) for j in jobs} >= {(0, 0), (1, 1)}
    src = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in imgs])).to(gpu)
    small = torch.from_numpy(np.concatenate([jobs.view(np.uint8).reshape(-1), coef.view(np.uint8)])).to(gpu)
    name = "clipmi_resize_crop_rgb8" if px == 3 else "clipmi_resize_crop_rgba8"
    n, block = len(imgs), 3 * N_PX * N_PX

    def call(ws, pixels):
        lib.check(getattr(L, name)(src.data_ptr(), small.data_ptr(), n, max_rows, small.data_ptr() + jobs.nbytes, N_PX, pixels.data_ptr(),
                                   ws.data_ptr(), lib.stream_ptr(gpu)), name)
    got = W.run_independent(call, [("pixels", n * block)], scratch_bytes, device=gpu)
    for k, b in enumerate(blobs):
        assert np.array_equal(got["pixels"][k * block:(k + 1) * block].reshape(3, N_PX, N_PX), M.load_uint8_blob(b, N_PX)), SHAPES[k]


def test_nearest_crop_p8(clipmi, gpu):
    """clipmi_nearest_crop_p8 takes no scratch rows: the output alone is prefilled"""
    from clipmi.decode_worker import nearest_plan
    from clipmi.resize import NEAREST_JOB
    lib, L = clipmi._lib, clipmi._lib.lib()
    rng = np.random.default_rng(551)
    blobs = [M.mode_file(rng, 3, (8, 4, 2, 1, 8, 4)[k], h, w, k) for k, (h, w) in enumerate(SHAPES)]
    idx = [M.pillow_pixels(b)[1] for b in blobs]
    n, block = len(idx), 3 * N_PX * N_PX
    jobs = np.zeros(n, dtype=NEAREST_JOB)
    tabs = np.zeros(n * (768 + 8 * N_PX), np.uint8)
    soff = 0
    for k, a in enumerate(idx):
        h, w = a.shape
        plan = nearest_plan(w, h, N_PX)
        o = k * (768 + 8 * N_PX)
        tabs[o:o + 768] = M.pillow_palette(blobs[k])[0].reshape(-1)
        tabs[o + 768:o + 768 + 8 * N_PX].view(np.int32)[:] = np.concatenate([plan["hcoef"], plan["vcoef"]])
        j = jobs[k]
        j["src_off"], j["w"], j["h"], j["out_index"] = soff, w, h, k
        j["pal_off"], j["col_off"], j["row_off"] = o, (o + 768) // 4, (o + 768) // 4 + N_PX
        soff += (h * w + 15) // 16 * 16
    flat = np.zeros(soff, np.uint8)
    for j, a in zip(jobs, idx):
        flat[int(j["src_off"]):int(j["src_off"]) + a.size] = a.reshape(-1)
    src = torch.from_numpy(flat).to(gpu)
    small = torch.from_numpy(np.concatenate([jobs.view(np.uint8).reshape(-1), tabs])).to(gpu)

    def call(ws, pixels):
        lib.check(L.clipmi_nearest_crop_p8(src.data_ptr(), small.data_ptr(), n, small.data_ptr() + jobs.nbytes, N_PX, pixels.data_ptr(),
                                           lib.stream_ptr(gpu)), "clipmi_nearest_crop_p8")
    got = W.run_independent(call, [("pixels", n * block)], 0, device=gpu)
    for k, b in enumerate(blobs):
        assert np.array_equal(got["pixels"][k * block:(k + 1) * block].reshape(3, N_PX, N_PX), M.load_uint8_blob(b, N_PX)), SHAPES[k]
