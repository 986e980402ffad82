"""pipeline.encode_files with baseline JPEG, progressive JPEG and PNG files decoded on the device in the SAME batches, each format
with files the device reports: every status has to reach the file it belongs to. The three formats share one status tensor
(baseline files, then progressive ones, then PNG files), so a wrong offset would hand one file's "corrupt" verdict to another -
a good file would be decoded again by Pillow (harmless) while the corrupt one keeps the device's pixels or stays among the good
files (wrong vectors, wrong failed list). Runs in a child process with the product's start order (decode workers before the GPU).

Per format: three good files; one file the parser lets through, the device reports and Pillow refuses too (it must join the
failed files and its row leave the batch); one the device reports and Pillow decodes (Pillow's pixels must replace exactly its
row). Progressive has no file of the first kind: jpeg_parse.parse_progressive lets nothing through that Pillow refuses
(test_jpeg_progressive.py::test_parser_never_accepts_a_file_pillow_refuses holds it to that over the malformed corpus, and none of
that corpus' files qualifies), while the baseline parser, which leaves the byte stuffing to the device, cannot see a marker inside
the scan, and the PNG parser does not inflate the stream. Beside them an RGB BMP (full size in its region, resized on the
device) and an RGBA PNG (Pillow's).

The second test runs the same worker under a poisoning allocator: every CUDA tensor torch.empty returns during the device runs - the
status tensor DeviceStage.run allocates, the workspaces, the decoded and the scratch rows, the batch tensor - starts as 0xFF bytes. A
decoder that wrote a status only where it found an error, or read a workspace it had not written, would change the result."""
import io
import os
import re

import numpy as np
import pytest
from PIL import Image, ImageFile

import jpeg_corpus
import jpeg_progressive
import png_cases
from test_jpeg import smooth

pytestmark = pytest.mark.gpu


def _pillow_takes(blob):
    try:
        Image.open(io.BytesIO(blob)).convert("RGB")
        return True
    except Exception:
        return False


def reported_baseline():
    """(a file Pillow refuses, a file Pillow decodes) out of jpeg_corpus' damaged scans: the parser lets both through with their
    stuffing kept, and the device finds a marker inside the segment (status 3, test_jpeg_gpu.py)."""
    from clipmi import jpeg_parse
    picked = {}
    for fam, name, blob in jpeg_corpus.entropy_damage(jpeg_corpus.base_files()):
        try:
            p = jpeg_parse.parse(blob, keep_stuffing=True)
        except jpeg_parse.Unsupported:
            continue
        if p.stuffed == 1 and re.search(rb"\xff[^\x00]", p.stream) is not None:
            picked.setdefault(_pillow_takes(blob), blob)
    return picked[False], picked[True]


def reported_progressive():
    """A file out of jpeg_progressive's malformed corpus whose scan data ends early: the parser lets it through, the CPU
    restatement of the device decoder reports it (Corrupt), Pillow decodes what is there."""
    from clipmi import jpeg_parse
    for fam, blob in jpeg_progressive.malformed_corpus(np.random.default_rng(77)):
        if fam != "short_scan":
            continue
        try:
            p = jpeg_parse.parse_progressive(blob)
            jpeg_progressive.decode(p)
        except jpeg_parse.Unsupported:
            continue
        except jpeg_progressive.Corrupt:
            if _pillow_takes(blob):
                return blob
    raise AssertionError("no such file in the corpus")


def reported_png(rng):
    """(the cut stream test_png_pipeline_gpu.py builds: Pillow refuses it too; a stream without its Adler-32, which Pillow does
    not look at and the device reports: png_cases.malformed_corpus' adler_missing family)"""
    from clipmi import png_parse
    a = png_cases.screenshot(rng, 240, 320, 3)
    z = png_cases.deflate(png_cases.filter_rows(a, png_cases.filters_for("cycle", 240)))
    cut, no_adler = png_cases.assemble(320, 240, 3, z[:len(z) * 2 // 3]), png_cases.assemble(320, 240, 3, z[:-4])
    for blob in (cut, no_adler):
        assert png_cases.cpu_decode(png_parse.parse(blob)) is None           # the device's rule on the CPU: reported
    assert not _pillow_takes(cut) and _pillow_takes(no_adler)
    return cut, no_adler


class _PoisonedEmpty:
    """While active, every CUDA tensor torch.empty returns holds 0xFF bytes (and the device has finished writing them)"""

    def __enter__(self):
        import torch
        self.torch, self.empty, self.count = torch, torch.empty, 0

        def empty(*a, **kw):
            t = self.empty(*a, **kw)
            if t.is_cuda and t.numel():
                t.view(-1).view(torch.uint8).fill_(0xFF)
                torch.cuda.synchronize(t.device)
                self.count += 1
            return t
        torch.empty = empty
        return self

    def __exit__(self, *exc):
        self.torch.empty = self.empty


def _mixed_worker(tmp, poison=False):
    import contextlib
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import torch
    import clipmi
    from clipmi import decode_worker
    ImageFile.MAXBLOCK = 1 << 24
    rng = np.random.default_rng(47)

    def put(name, blob):
        p = os.path.join(tmp, name)
        with open(p, "wb") as f:
            f.write(blob)
        return p

    def put_img(name, img, **kw):
        p = os.path.join(tmp, name)
        img.save(p, **kw)
        return p

    base = [put_img("base0.jpg", Image.fromarray(smooth(rng, 240, 320)), quality=85, subsampling=2),
            put_img("base1.jpg", Image.fromarray(smooth(rng, 300, 200)), quality=80, subsampling=1, restart_marker_rows=1),
            put_img("base2.jpg", Image.fromarray(smooth(rng, 225, 223)[..., 0]), quality=80, optimize=True)]
    prog = [put_img("prog0.jpg", Image.fromarray(smooth(rng, 224, 300)), quality=75, subsampling=0, progressive=True),
            put_img("prog1.jpg", Image.fromarray(smooth(rng, 260, 230)), quality=85, subsampling=1, progressive=True),
            put_img("prog2.jpg", Image.fromarray(smooth(rng, 300, 260)[..., 0]), quality=85, progressive=True, optimize=True)]
    pngs = [put_img("png0.png", Image.fromarray(png_cases.screenshot(rng, 480, 640, 3))),
            put("png1.png", png_cases.write(png_cases.screenshot(rng, 300, 260, 1), "cycle", level=6)),
            put("png2.png", png_cases.write(png_cases.smooth(rng, 90, 70, 3), "cycle", level=9))]
    bmp = put_img("full.bmp", Image.fromarray(smooth(rng, 250, 350)))
    rgba = put_img("rgba.png", Image.fromarray(smooth(rng, 230, 240)).convert("RGBA"))
    b_refused, b_decoded = reported_baseline()
    base_refused, base_decoded = put("base_refused.jpg", b_refused), put("base_decoded.jpg", b_decoded)
    prog_decoded = put("prog_decoded.jpg", reported_progressive())
    p_cut, p_no_adler = reported_png(rng)
    png_refused, png_decoded = put("png_refused.png", p_cut), put("png_decoded.png", p_no_adler)
    # formats alternate within each batch of 8, and both batches hold reported files of more than one format
    files = [base[0], prog[0], pngs[0], bmp, base_refused, prog_decoded, png_refused, base[1],
             pngs[1], prog[1], rgba, png_decoded, base_decoded, prog[2], base[2], pngs[2]]
    assert Image.open(bmp).mode == "RGB" and all(max(Image.open(p).size) <= 640 for p in files)
    scratch = np.zeros(4 << 20, np.uint8)
    for stager, group in ((decode_worker.stage_jpeg, base + [base_refused, base_decoded]),
                          (decode_worker.stage_jpeg_progressive, prog + [prog_decoded]),
                          (decode_worker.stage_png, pngs + [png_refused, png_decoded])):
        for p in group:
            assert 0 < stager(p, 224, scratch)[2] <= 65536, p       # fits the smallest region size the pipeline uses, in every run
    import warnings
    warnings.simplefilter("ignore")
    with clipmi.pipeline.DecodePool(3) as pool:
        assert not torch.cuda.is_initialized()
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        host = list(clipmi.pipeline.encode_files(model, files, batch=8, pool=pool, device_resize_mb=0, device_jpeg_kb=0))
        kw = dict(batch=8, pool=pool, device_resize_mb=8, device_jpeg_kb=2048, device_progressive=True, device_png=True)
        st_on, st_grp = {}, {}
        with (_PoisonedEmpty() if poison else contextlib.nullcontext()) as poisoned:
            on = list(clipmi.pipeline.encode_files(model, files, stats=st_on, **kw))
            grp = list(clipmi.pipeline.encode_files(model, files, stats=st_grp, jpeg_group_mb=1, **kw))
        assert not poison or (poisoned.count >= 8 and torch.empty is poisoned.empty), "the device runs allocate through torch.empty"
    assert [p for h in host for p in h[2]] == [base_refused, png_refused]
    assert [len(h[0]) for h in host] == [6, 8]
    for other, st in ((on, st_on), (grp, st_grp)):
        assert [h[0] for h in host] == [d[0] for d in other] and [h[2] for h in host] == [d[2] for d in other]
        for h, d in zip(host, other):
            assert np.array_equal(h[1], d[1])
        # staged for the device: every file of the format, reported or not; png_files counts what the device decoded and kept
        assert st["jpeg_files"] == len(base) + 2 and st["jpeg_progressive_files"] == len(prog) + 1 and st["png_files"] == len(pngs), st
    open(os.path.join(tmp, "ok"), "w").write("1")


def _run_worker(tmp_path, poison):
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r}); " \
           f"import test_mixed_formats_pipeline_gpu as t; t._mixed_worker({str(tmp_path)!r}, poison={poison!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "ok").read_text() == "1"


def test_statuses_reach_their_files_when_three_formats_share_a_batch(tmp_path):
    _run_worker(tmp_path, poison=False)


def test_the_same_under_an_allocator_that_poisons_every_device_tensor(tmp_path):
    """The same vectors, failed lists and counters as the host path, with and without jpeg_group_mb=1, when nothing the device path
    allocates starts out as zeros"""
    _run_worker(tmp_path, poison=True)
