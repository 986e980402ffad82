"""Four-component JPEG files on the device (csrc/jpeg.hip clipmi_jpeg_decode_cmyk8, csrc/resize.hip clipmi_resize_crop_cmyk8), bit
for bit against Pillow live and the committed pixels: the decode in every form (segments sliced, unstuffed, with restart
intervals), the transform, a damaged file among good ones, a record the kernels do not take, and
pipeline.encode_files(device_jpeg_cmyk=True). tests/jpeg_cmyk.py writes the files."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import jpeg_cmyk as jc
from clipmi import jpeg, jpeg_parse
from clipmi.decode_worker import load_uint8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_cmyk_cases.npz")


def decoded(out, recs, status):
    st, host = status.cpu().numpy(), out.cpu().numpy()
    pix = [host[int(r["out_off"]):int(r["out_off"]) + int(r["height"]) * int(r["width"]) * 4].reshape(int(r["height"]), int(r["width"]), 4)
           for r in recs]
    return pix, [int(s) for s in st[:len(recs)]]


def device(items):
    return decoded(*jpeg.decode_device(items, DEV, cmyk=True))


def pillow_or_none(blob):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            return jc.pillow4(blob)
        except Exception:
            return None


SIZES = [(5, 5), (8, 8), (16, 16), (17, 17), (45, 37), (130, 67)]          # (H, W), cycled across the batch; and 1x1 for 1x1 sampling


def live_batch(form):
    """One batch: every sampling x {CMYK, YCCK, no Adobe} at sizes cycled from SIZES (1x1 for 1x1 sampling too), the optimize,
    two_quant and two_huffman files at qualities 30 and 95, and a 160x120 noise file of more than 16 KiB of entropy-coded data"""
    rng = np.random.default_rng(61)
    kw = dict(restart_marker_blocks=3) if form == "restart" else {}
    files, k = [], 0
    for sub in (0, 1, 2):
        for colour in ("cmyk", "ycck", "no_adobe"):
            for H, W in [SIZES[k % len(SIZES)], SIZES[(k + 1) % len(SIZES)]] + ([(1, 1)] if sub == 0 else []):
                b = jc.cmyk_file(jc.smooth4(rng, H, W), subsampling=sub, quality=(92, 75, 50)[k % 3], **kw)
                files.append((f"{colour} sub{sub} {H}x{W}", jc.as_ycck(b) if colour == "ycck" else jc.without_adobe(b) if colour == "no_adobe" else b))
            k += 1
    assert {n.split()[-1] for n, _ in files} >= {f"{h}x{w}" for h, w in SIZES} | {"1x1"}
    for q in (30, 95):
        for j, form2 in enumerate(("optimize", "two_quant", "two_huffman")):
            H, W = SIZES[3 + (j + q) % 3]
            a = jc.smooth4(rng, H, W)
            if form2 == "two_quant":
                b = jc.two_quant(a, subsampling=j, quality=q, **kw)
            else:
                b = jc.cmyk_file(a, subsampling=j, quality=q, optimize=True, **kw)
                b = jc.two_huffman(b) if form2 == "two_huffman" else b
            files.append((f"{form2} q{q} sub{j} {H}x{W}", b))
    noise = jc.cmyk_file(rng.integers(0, 256, (120, 160, 4), dtype=np.uint8), subsampling=2, quality=95, **kw)
    files.append(("noise sub2 120x160", noise))
    return files


@pytest.mark.parametrize("form", ["sliced", "unstuffed", "restart"])
def test_device_equals_pillow_live(form):
    files = live_batch(form)
    items = [jpeg_parse.parse(b, keep_stuffing=form == "sliced", cmyk=True) for _, b in files]
    assert all(it.ncomp == 4 for it in items) and {(it.hs, it.vs) for it in items} == {(1, 1), (2, 1), (2, 2)}
    assert {it.transform for it in items} == {jc.CMYK, jc.YCCK}
    # the Huffman kernel crosses a chunk of 128 subsequences (16 KiB) with four components - where the file has no restart intervals
    assert len(items[-1].stream) > 16384
    if form == "sliced":
        assert all(it.stuffed == 1 for it in items)
    if form == "restart":
        assert all(it.ri == 3 for it in items)
    pix, st = device(items)
    bad = [(n, s) for (n, _), s in zip(files, st) if s]
    assert not bad, f"non-zero status for well-formed files: {bad}"
    wrong = [n for (n, b), g in zip(files, pix) if not np.array_equal(g, jc.pillow4(b))]
    assert not wrong, f"status 0 with pixels that are not Pillow's: {wrong}"


def test_component_0_at_the_layouts_samplings():
    """Component 0 sampled 1x2, 4x1 or 1x4 (forged by relabelling, as tests/jpeg_layouts.py does): taken with layouts=True as well"""
    rng = np.random.default_rng(62)
    blobs = []
    for luma, (H, W), (h, w), sub in ((0x12, (40, 24), (24, 40), 1), (0x41, (13, 35), (26, 18), 2), (0x14, (35, 13), (18, 26), 2)):
        for ycck in (False, True):
            b = jc.relabel(jc.cmyk_file(jc.smooth4(rng, h, w), subsampling=sub), luma=luma, width=W, height=H)
            blobs.append(jc.as_ycck(b) if ycck else b)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        refs = [jc.pillow4(b) for b in blobs]
    pix, st = decoded(*jpeg.decode_device([jpeg_parse.parse(b, keep_stuffing=True, cmyk=True, layouts=True) for b in blobs], DEV,
                                          cmyk=True, layouts=True))
    assert st == [0] * len(blobs)
    for k, (g, r) in enumerate(zip(pix, refs)):
        assert np.array_equal(g, r), k


def test_the_golden_files_decode_to_the_committed_pixels():
    d = np.load(GOLDEN)
    n, n_px = int(d["n"]), int(d["n_px"])
    blobs = [d[f"file_{i}"].tobytes() for i in range(n)]
    for ks in (True, False):
        pix, st = device([jpeg_parse.parse(b, keep_stuffing=ks, cmyk=True) for b in blobs])
        assert not any(st), st
        for i, g in enumerate(pix):
            assert np.array_equal(g, d[f"cmyk_{i}"]), str(d["names"][i])
    for fused in (True, False):
        out, status = jpeg.transform_files(blobs, n_px, DEV, fused=fused, cmyk=True)
        assert not status.cpu().numpy().any()
        out = out.cpu().numpy()
        for i in range(n):
            assert np.array_equal(out[i], d[f"transform_{i}"]), (fused, str(d["names"][i]))


def pillow_transform(tmp_path, blobs, n_px):
    out = []
    for k, b in enumerate(blobs):
        path = str(tmp_path / f"{n_px}_{k}.jpg")
        with open(path, "wb") as f:
            f.write(b)
        out.append(load_uint8(path, n_px))
    return np.stack(out)


# (H, W): both axes resampled | portrait | neither axis | one axis | odd sizes; and a small one at n_px = 32
TRANSFORM_SIZES = [((300, 400), 224), ((400, 300), 224), ((224, 224), 224), ((250, 224), 224), ((225, 226), 224), ((40, 33), 32)]


@pytest.mark.parametrize("n_px", [224, 32])
def test_transform_equals_pillows(tmp_path, n_px):
    rng = np.random.default_rng(63)
    files = []
    for (H, W), npx in TRANSFORM_SIZES:
        if npx != n_px:
            continue
        files.append((f"cmyk 2x2 {H}x{W}", jc.cmyk_file(jc.smooth4(rng, H, W), subsampling=2, quality=90)))
        files.append((f"ycck 1x1 {H}x{W}", jc.as_ycck(jc.cmyk_file(jc.smooth4(rng, H, W), subsampling=0, quality=90))))
        files.append((f"cmyk 2x1 {H}x{W}", jc.cmyk_file(jc.smooth4(rng, H, W), subsampling=1, quality=90)))
    files.append(("ordinary 4:2:0", jc.encode(jc.smooth(rng, 300, 260), quality=85, subsampling=2)))
    files.append(("grey", jc.encode(jc.smooth(rng, 230, 260)[..., 0], quality=85)))
    blobs = [b for _, b in files]
    with pytest.raises(jpeg_parse.Unsupported):              # the switch is opt-in on this path too
        jpeg.transform_files(blobs, n_px, DEV)
    with pytest.raises(jpeg_parse.Unsupported):
        jpeg.transform_files(blobs, n_px, DEV, layouts=True)
    ref = pillow_transform(tmp_path, blobs, n_px)
    staged = jpeg.stage_transform(blobs, n_px, DEV, keep_stuffing=True, cmyk=True)
    assert sorted(g["px"] for g in staged.groups) == [3, 4]
    for fused in (True, False):
        for out, status in (jpeg.run_transform(staged, fused), jpeg.transform_files(blobs, n_px, DEV, fused=fused, cmyk=True)):
            assert not status.cpu().numpy().any()
            out = out.cpu().numpy()
            for k, (label, _) in enumerate(files):
                assert np.array_equal(out[k], ref[k]), f"fused={fused}: {label} != Pillow's transform"


def cut(blob, frac):
    """The file with its entropy-coded data ended early and EOI appended again (as test_jpeg_layouts_gpu.cut)"""
    start = blob.index(b"\xff\xda")
    return blob[:start + int((len(blob) - start) * frac)] + b"\xff\xd9"


def test_a_file_whose_data_ends_early_among_good_ones():
    rng = np.random.default_rng(64)
    good = [jc.cmyk_file(jc.smooth4(rng, 120, 90), subsampling=2), jc.as_ycck(jc.cmyk_file(jc.smooth4(rng, 64, 130), subsampling=0)),
            jc.cmyk_file(jc.smooth4(rng, 130, 64), subsampling=1)]
    short = [cut(jc.cmyk_file(jc.smooth4(rng, 296, 328), subsampling=2), 0.5), cut(jc.as_ycck(jc.cmyk_file(jc.smooth4(rng, 296, 328), subsampling=1)), 0.9)]
    batch = [good[0], short[0], good[1], short[1], good[2]]
    where_good = [0, 2, 4]
    for ks in (True, False):
        pix, st = device([jpeg_parse.parse(b, keep_stuffing=ks, cmyk=True) for b in batch])
        for k, b in enumerate(batch):
            ref = pillow_or_none(b)
            if k in where_good:
                assert st[k] == 0 and np.array_equal(pix[k], ref), k
            else:
                assert st[k] != 0 or (ref is not None and np.array_equal(pix[k], ref)), k
        assert any(st), "a segment cut in half must be noticed"


def test_a_record_the_kernels_do_not_take_is_reported_not_decoded():
    """Sampling factors outside the set, a three-component record's transform, or ncomp = 3 in a record handed to the new entry:
    status 1 for that file, its neighbours Pillow's"""
    rng = np.random.default_rng(65)
    blobs = [jc.cmyk_file(jc.smooth4(rng, 40, 30), subsampling=2), jc.cmyk_file(jc.smooth4(rng, 33, 47), subsampling=2),
             jc.as_ycck(jc.cmyk_file(jc.smooth4(rng, 16, 40), subsampling=1)), jc.cmyk_file(jc.smooth4(rng, 24, 40), subsampling=0),
             jc.cmyk_file(jc.smooth4(rng, 21, 22), subsampling=0), jc.cmyk_file(jc.smooth4(rng, 30, 31), subsampling=1)]
    for ks in (True, False):
        items = [jpeg_parse.parse(b, keep_stuffing=ks, cmyk=True) for b in blobs]
        items[1].hs, items[1].vs = 4, 2                     # (pack sizes the record's buffers by these factors too: a consistent record)
        items[3].transform = 0
        recs, tables, streams, out_bytes, total, most, pixels = jpeg.pack(items, cmyk=True)
        recs["ncomp"][4] = 3                                # the record keeps its buffers; the kernels must not read it as either kind
        L = jpeg._lib.lib()
        dev, offs, _ = jpeg._lib.to_device16([recs, tables, streams], DEV)
        out = torch.zeros(out_bytes, dtype=torch.uint8, device=DEV)
        status = torch.full((len(items),), -1, dtype=torch.int32, device=DEV)
        ws_bytes = int(L.clipmi_jpeg_workspace_bytes(total, len(tables)))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        base = dev.data_ptr()
        jpeg._lib.check(L.clipmi_jpeg_decode_cmyk8(base + offs[2], base, len(items), base + offs[1], len(tables), total, most, pixels,
                                                   out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes, jpeg._lib.stream_ptr(torch.device(DEV))),
                        "clipmi_jpeg_decode_cmyk8")
        pix, st = decoded(out, recs, status)
        assert st == [0, 1, 0, 1, 1, 0]
        for k in (0, 2, 5):
            assert np.array_equal(pix[k], jc.pillow4(blobs[k])), k
        for k in (1, 3, 4):                                 # nothing of a refused record is decoded
            assert not pix[k].any(), k
        # the refused records come back emptied, as the baseline entry's
        back = dev[:recs.nbytes].cpu().numpy().view(jpeg.IMAGE4)
        for k in (1, 3, 4):
            r = back[k]
            assert (r["width"], r["height"], r["ncomp"], r["hs"], r["vs"], r["stream_bytes"], r["reserved"], r["stuffed"]) == (0, 0, 1, 1, 1, 0, 0, 0)


def test_the_fused_entries_refuse_four_components(tmp_path):
    """ncomp = 4 in a record of clipmi_jpeg_decode_transform_rgb8: status 1, the neighbour Pillow's"""
    rng = np.random.default_rng(67)
    blobs = [jc.encode(jc.smooth(rng, 33, 47), quality=85, subsampling=2), jc.encode(jc.smooth(rng, 40, 56), quality=85, subsampling=2)]
    staged = jpeg.stage_transform(blobs, 32, DEV)
    (g,) = staged.groups
    at = jpeg.IMAGE.itemsize + jpeg.IMAGE.fields["ncomp"][1]           # the second record's ncomp
    g["dev"][at:at + 4] = torch.tensor([4, 0, 0, 0], dtype=torch.uint8, device=DEV)
    out, status = jpeg.run_transform(staged, fused=True)
    assert status.cpu().tolist() == [0, 1]
    assert np.array_equal(out[0].cpu().numpy(), pillow_transform(tmp_path, blobs[:1], 32)[0])


def _cmyk_pipeline_worker(tmp):
    """Own process, the product's start order (decode workers first, GPU second): a directory of four-component files beside ordinary
    baseline and progressive files, a PNG, a progressive CMYK file and a broken one."""
    sys.path.insert(0, ROOT)
    import clipmi
    from PIL import Image
    rng = np.random.default_rng(66)
    paths = []

    def put(name, data):
        p = os.path.join(tmp, name)
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
        return p

    n_four = 0
    for k, (H, W, sub, ycck) in enumerate([(225, 226, 2, False), (300, 400, 0, True), (250, 330, 1, False), (301, 451, 2, True),
                                           (240, 320, 2, False)]):
        kw = dict(restart_marker_blocks=5) if k == 2 else {}
        b = jc.cmyk_file(jc.smooth4(rng, H, W), subsampling=sub, quality=90, **kw)
        put(f"a{k:02d}.jpg", jc.as_ycck(b) if ycck else b)
        n_four += 1
    put("c_cut.jpg", cut(jc.cmyk_file(jc.smooth4(rng, 296, 328), subsampling=2, quality=90), 0.66))     # parses; the device reports it
    n_four += 1
    for k, sub in enumerate((0, 1, 2)):
        put(f"d{k}.jpg", jc.encode(jc.smooth(rng, 240 + 30 * k, 350 - 20 * k), quality=88, subsampling=sub))
    put("e_prog.jpg", jc.encode(jc.smooth(rng, 300, 260), quality=88, subsampling=2, progressive=True))
    put("f_grey.jpg", jc.encode(jc.smooth(rng, 230, 260)[..., 0], quality=85))
    Image.fromarray(jc.smooth(rng, 250, 350)).save(os.path.join(tmp, "g.png"))
    paths.append(os.path.join(tmp, "g.png"))
    put("h_prog_cmyk.jpg", jc.cmyk_file(jc.smooth4(rng, 240, 320), subsampling=2, progressive=True))
    bad = put("i_broken.jpg", b"broken")
    warnings.simplefilter("ignore")
    runs, stats = {}, {}
    with clipmi.pipeline.DecodePool(3) as pool:                     # before anything initialises the GPU
        assert not torch.cuda.is_initialized()
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        # (the switch, then layouts + progressive on the device + the fused entries beside it)
        for key in ((False, False), (True, False), (False, True), (True, True)):
            stats[key] = {}
            pool.jpeg_cap_hint = 1 << 20                            # every run starts with regions all the files fit
            runs[key] = list(clipmi.pipeline.encode_files(
                model, paths, batch=16, pool=pool, device_resize_mb=0, device_jpeg_kb=4096, device_progressive=key[1], jpeg_fused=key[1],
                device_jpeg_layouts=key[1], device_jpeg_cmyk=key[0], stats=stats[key]))
    off = runs[False, False]
    for key, other in runs.items():
        assert [h[0] for h in off] == [d[0] for d in other] and [h[2] for h in off] == [d[2] for d in other], key
        for h, d in zip(off, other):
            assert torch.equal(torch.from_numpy(h[1]), torch.from_numpy(d[1])), key
    failed = [p for h in off for p in h[2]]
    assert bad in failed and len(failed) in (1, 2)                  # the cut file: whatever Pillow decides, every path agrees
    counts = {key: {k: v for k, v in s.items() if k.endswith("_files")} for key, s in stats.items()}
    assert [counts[key]["jpeg_cmyk_files"] for key in runs] == [0, n_four, 0, n_four], counts
    for extra in (False, True):                                     # every other count is unchanged by the switch
        a, b = dict(counts[False, extra]), dict(counts[True, extra])
        a.pop("jpeg_cmyk_files"), b.pop("jpeg_cmyk_files")
        assert a == b, counts
    assert counts[True, False]["jpeg_files"] == 4 and counts[True, True]["jpeg_progressive_files"] == 1, counts
    with open(os.path.join(tmp, "ok"), "w") as f:
        f.write("1")


def test_pipeline_with_the_switch_on_gives_the_same_vectors(tmp_path):
    """encode_files(device_jpeg_cmyk=True) yields the vectors and the failed files of the switch off, plain and beside
    device_jpeg_layouts + device_progressive + jpeg_fused, and counts the files it added under jpeg_cmyk_files"""
    code = f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); " \
           f"import test_jpeg_cmyk_gpu as t; t._cmyk_pipeline_worker({str(tmp_path)!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "ok").read_text() == "1"
