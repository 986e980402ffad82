"""The device JPEG decoder (csrc/jpeg.hip) on the layouts jpeg_parse.parse(layouts=True) adds - luma sampling 1x2, 4x1, 1x4 and
RGB-coded files (tests/jpeg_layouts.py forges them) - bit for bit against Pillow live and the committed pixels: the plain decode in
every form (segments sliced, unstuffed, with restart intervals, progressive), the transform entries fused and unfused, a damaged
file among good ones, and pipeline.encode_files(device_jpeg_layouts=True)."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import jpeg_layouts as jl
from clipmi import jpeg, jpeg_parse
from clipmi.decode_worker import load_uint8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_layout_cases.npz")


def ordinary(rng, progressive=False):
    """A 4:2:0, a 4:2:2 and a grey Pillow file: between the forged ones, so that the records' offsets have to keep images apart"""
    kw = dict(progressive=True) if progressive else {}
    return [jl.encode(jl.smooth(rng, 45, 61), quality=88, subsampling=2, **kw), jl.encode(jl.smooth(rng, 24, 50), quality=80, subsampling=1, **kw),
            jl.encode(jl.smooth(rng, 30, 26)[..., 0], quality=85, **kw)]


def decoded(out, recs, status):
    st, host = status.cpu().numpy(), out.cpu().numpy()
    pix = [host[int(r["out_off"]):int(r["out_off"]) + int(r["height"]) * int(r["width"]) * 3].reshape(int(r["height"]), int(r["width"]), 3)
           for r in recs]
    return pix, [int(s) for s in st[:len(recs)]]


def device(blobs, progressive=False, keep_stuffing=False):
    """-> (pixels, status) of every file; every file must pass its parser with layouts=True"""
    if progressive:
        return decoded(*jpeg.decode_progressive_device([jpeg_parse.parse_progressive(b, layouts=True) for b in blobs], DEV, layouts=True))
    return decoded(*jpeg.decode_device([jpeg_parse.parse(b, keep_stuffing=keep_stuffing, layouts=True) for b in blobs], DEV, layouts=True))


@pytest.mark.parametrize("form", ["sliced", "unstuffed", "restart", "progressive"])
def test_device_equals_pillow_live(form):
    fx = jl.fixtures({"sliced": "baseline", "unstuffed": "baseline"}.get(form, form))
    assert len(fx) == len(jl.PROGRESSIVE_SPECS if form == "progressive" else jl.SPECS)
    rng = np.random.default_rng(5)
    plain = ordinary(rng, form == "progressive")
    blobs, names = [], []
    for k, f in enumerate(fx):                             # an ordinary file after every seventh forged one
        blobs.append(f.blob)
        names.append(f.name)
        if k % 7 == 3:
            blobs.append(plain[(k // 7) % 3])
            names.append(f"ordinary {(k // 7) % 3}")
    assert len(blobs) >= len(fx) + 3
    if form == "sliced":
        assert sum(jpeg_parse.parse(b, keep_stuffing=True, layouts=True).stuffed for b in blobs) == len(blobs)
    if form == "restart":
        assert all(jpeg_parse.parse(f.blob, layouts=True).ri == 3 for f in fx)
    pix, st = device(blobs, form == "progressive", keep_stuffing=form == "sliced")
    bad = [(n, s) for n, s in zip(names, st) if s]
    assert not bad, f"non-zero status for well-formed files: {bad}"
    wrong = [n for n, b, g in zip(names, blobs, pix) if not np.array_equal(g, jl.pillow(b))]
    assert not wrong, f"status 0 with pixels that are not Pillow's: {wrong}"


def test_the_golden_files_decode_to_the_committed_pixels():
    d = np.load(GOLDEN)
    n = int(d["n"])
    blobs = [d[f"file_{i}"].tobytes() for i in range(n)]
    prog = [str(name).startswith("progressive") for name in d["names"]]
    assert 3 <= sum(prog) < n
    for progressive in (False, True):
        idx = [i for i in range(n) if prog[i] == progressive]
        pix, st = device([blobs[i] for i in idx], progressive, keep_stuffing=True)
        assert not any(st), st
        for i, g in zip(idx, pix):
            assert np.array_equal(g, d[f"rgb_{i}"]), str(d["names"][i])


# (H, W): both axes resampled, bands cross the 8-row boundary at odd r0 | the same, portrait | neither axis | one axis | more than
# JF_SPAN source columns, several chunks | odd sizes: the dh - 1 / last-column edges
TRANSFORM_SIZES = [(300, 400), (400, 300), (224, 224), (250, 224), (239, 1100), (225, 226)]


def pillow_transform(tmp_path, blobs, n_px):
    out = []
    for k, b in enumerate(blobs):
        path = str(tmp_path / f"{k}.jpg")
        with open(path, "wb") as f:
            f.write(b)
        out.append(load_uint8(path, n_px))
    return np.stack(out)


def test_fused_equals_unfused_equals_pillows_transform(tmp_path):
    rng = np.random.default_rng(47)
    files = []
    for H, W in TRANSFORM_SIZES:
        for layout, rgb in (("1x2", False), ("4x1", False), ("1x4", False), ("1x1", True), ("1x2", True), ("4x1", True)):
            files.append((f"{layout}{' rgb' if rgb else ''} {H}x{W}", jl.forge(layout, H, W, rng, rgb=rgb, quality=90)[0]))
        files.append((f"1x2 progressive {H}x{W}", jl.forge("1x2", H, W, rng, quality=90, progressive=True)[0]))
        files.append((f"2x2 rgb progressive {H}x{W}", jl.forge("2x2", H, W, rng, rgb=True, quality=90, progressive=True)[0]))
    files.append(("4x1 progressive 112x512", jl.forge("4x1", 112, 512, rng, quality=90, progressive=True)[0]))
    files.append(("1x4 progressive 512x112", jl.forge("1x4", 512, 112, rng, quality=90, progressive=True)[0]))
    files.append(("ordinary 4:2:0", jl.encode(jl.smooth(rng, 300, 260), quality=85, subsampling=2)))
    blobs = [b for _, b in files]
    with pytest.raises(jpeg_parse.Unsupported):              # the switch is opt-in on this path too
        jpeg.stage_transform(blobs[:1], 224, DEV)
    ref = pillow_transform(tmp_path, blobs, 224)
    st = jpeg.stage_transform(blobs, 224, DEV, keep_stuffing=True, layouts=True)
    assert sorted(g["progressive"] for g in st.groups) == [False, True]
    out, status = jpeg.run_transform(st, fused=True)
    plain, plain_status = jpeg.run_transform(st, fused=False)
    assert not status.cpu().numpy().any() and not plain_status.cpu().numpy().any()
    out, plain = out.cpu().numpy(), plain.cpu().numpy()
    for k, (label, _) in enumerate(files):
        assert np.array_equal(plain[k], ref[k]), f"unfused != Pillow: {label}"
        assert np.array_equal(out[k], plain[k]), f"fused != unfused: {label}"


def cut(blob, frac):
    """The file with its entropy-coded data ended early and EOI appended again"""
    start = blob.index(b"\xff\xda")
    return blob[:start + int((len(blob) - start) * frac)] + b"\xff\xd9"


def pillow_or_none(blob):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            return jl.pillow(blob)
        except Exception:
            return None


def test_a_file_whose_data_ends_early_among_good_ones(tmp_path):
    rng = np.random.default_rng(29)
    good = [jl.forge("1x2", 120, 90, rng)[0], jl.forge("4x1", 64, 130, rng, rgb=True)[0], jl.forge("1x4", 130, 64, rng)[0]]
    short = [cut(jl.forge(layout, 296, 328, rng, rgb=rgb)[0], frac) for layout, rgb, frac in
             (("1x2", False, 0.5), ("4x1", False, 0.66), ("1x4", True, 0.3), ("1x2", True, 0.9))]
    batch = [good[0], short[0], short[1], good[1], short[2], short[3], good[2]]
    where_good = [0, 3, 6]
    for ks in (True, False):
        pix, st = device(batch, keep_stuffing=ks)
        for k, b in enumerate(batch):
            ref = pillow_or_none(b)
            if k in where_good:
                assert st[k] == 0 and np.array_equal(pix[k], ref), k
            else:
                assert st[k] != 0 or (ref is not None and np.array_equal(pix[k], ref)), k
        assert any(st), "a segment cut in half must be noticed"
    ref = pillow_transform(tmp_path, good, 64)
    staged = jpeg.stage_transform(batch, 64, DEV, keep_stuffing=True, layouts=True)
    for fused in (True, False):
        out, status = jpeg.run_transform(staged, fused)
        out, status = out.cpu().numpy(), status.cpu().numpy()
        assert [int(status[k]) for k in where_good] == [0, 0, 0] and status.any()
        for j, k in enumerate(where_good):
            assert np.array_equal(out[k], ref[j]), (fused, k)


def test_a_record_the_kernels_do_not_take_is_reported_not_decoded():
    """Sampling factors or a colour transform outside the kernels' set: status 1 for that file, its neighbours Pillow's"""
    rng = np.random.default_rng(31)
    blobs = [jl.forge("1x2", 40, 30, rng)[0], jl.encode(jl.smooth(rng, 33, 47), quality=85, subsampling=2),
             jl.forge("4x1", 16, 40, rng)[0], jl.encode(jl.smooth(rng, 24, 40), quality=85, subsampling=0)]

    def spoil(items):
        items[1].hs, items[1].vs = 4, 2                     # (pack sizes the record's buffers by these factors too: a consistent record
        #                                                     of a sampling the kernels do not take - nothing of it may be decoded)
        items[3].transform = 2
        return items

    got = [decoded(*jpeg.decode_device(spoil([jpeg_parse.parse(b, keep_stuffing=ks, layouts=True) for b in blobs]), DEV, layouts=True))
           for ks in (True, False)]
    pblobs = [jl.forge(layout, 32, 48, rng, progressive=True)[0] for layout in ("1x2", "2x2", "1x2", "1x1")]
    got.append(decoded(*jpeg.decode_progressive_device(spoil([jpeg_parse.parse_progressive(b, layouts=True) for b in pblobs]), DEV, layouts=True)))
    for (pix, st), files in zip(got, (blobs, blobs, pblobs)):
        assert st == [0, 1, 0, 1]
        assert np.array_equal(pix[0], jl.pillow(files[0])) and np.array_equal(pix[2], jl.pillow(files[2]))


def _layouts_pipeline_worker(tmp):
    """Own process, the product's start order (decode workers first, GPU second): a directory of files of the new layouts, baseline
    and progressive, beside ordinary baseline and progressive files, a PNG, a CMYK JPEG, a file of a new layout whose data ends
    early and a broken one."""
    sys.path.insert(0, ROOT)
    import clipmi
    from PIL import Image
    rng = np.random.default_rng(53)
    paths = []

    def put(name, data):
        p = os.path.join(tmp, name)
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
        return p

    n_base = n_prog = 0
    for k, (layout, H, W, rgb) in enumerate([("1x2", 300, 400, False), ("1x2", 225, 226, False), ("4x1", 250, 330, False), ("4x1", 231, 1001, False),
                                             ("1x4", 400, 300, False), ("1x4", 227, 250, False), ("1x1", 260, 240, True), ("2x2", 301, 451, True),
                                             ("1x2", 240, 320, True), ("4x1", 224, 224, True)]):
        put(f"a{k:02d}.jpg", jl.forge(layout, H, W, rng, rgb=rgb, quality=90, **(dict(restart_marker_blocks=5) if k % 4 == 1 else {}))[0])
        n_base += 1
    for k, (layout, H, W, rgb) in enumerate([("1x2", 300, 400, False), ("1x2", 251, 333, True), ("4x1", 128, 512, False), ("1x4", 512, 128, False),
                                             ("2x1", 240, 300, True)]):
        put(f"b{k:02d}.jpg", jl.forge(layout, H, W, rng, rgb=rgb, quality=90, progressive=True)[0])
        n_prog += 1
    put("c_cut.jpg", cut(jl.forge("1x2", 320, 320, rng, quality=90)[0], 0.66))     # parses, but the data ends early: the device reports it
    n_base += 1
    for k, sub in enumerate((0, 1, 2)):
        put(f"d{k}.jpg", jl.encode(jl.smooth(rng, 240 + 30 * k, 350 - 20 * k), quality=88, subsampling=sub))
    put("e_prog.jpg", jl.encode(jl.smooth(rng, 300, 260), quality=88, subsampling=2, progressive=True))
    put("f_grey.jpg", jl.encode(jl.smooth(rng, 230, 260)[..., 0], quality=85))
    Image.fromarray(jl.smooth(rng, 250, 350)).save(os.path.join(tmp, "g.png"))
    paths.append(os.path.join(tmp, "g.png"))
    Image.fromarray(jl.smooth(rng, 240, 320)).convert("CMYK").save(os.path.join(tmp, "h_cmyk.jpg"), quality=85)
    paths.append(os.path.join(tmp, "h_cmyk.jpg"))
    bad = put("i_broken.jpg", b"broken")
    warnings.simplefilter("ignore")
    runs, stats = {}, {}
    with clipmi.pipeline.DecodePool(3) as pool:                     # before anything initialises the GPU
        assert not torch.cuda.is_initialized()
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        # (layouts, progressive on the device and the fused entries)
        for key in ((False, False), (True, False), (False, True), (True, True)):
            stats[key] = {}
            pool.jpeg_cap_hint = 1 << 20                            # every run starts with regions all the files fit
            runs[key] = list(clipmi.pipeline.encode_files(
                model, paths, batch=16, pool=pool, device_resize_mb=0, device_jpeg_kb=4096, device_progressive=key[1], jpeg_fused=key[1],
                device_jpeg_layouts=key[0], stats=stats[key]))
    off = runs[False, False]
    for key, other in runs.items():
        assert [h[0] for h in off] == [d[0] for d in other] and [h[2] for h in off] == [d[2] for d in other], key
        for h, d in zip(off, other):
            assert torch.equal(torch.from_numpy(h[1]), torch.from_numpy(d[1])), key
    failed = [p for h in off for p in h[2]]
    assert bad in failed and len(failed) in (1, 2)                  # the cut file: whatever Pillow decides, every path agrees
    counts = {key: {k: v for k, v in s.items() if k.endswith("_files")} for key, s in stats.items()}
    assert [counts[key]["jpeg_layout_files"] for key in runs] == [0, n_base, 0, n_base + n_prog], counts
    assert counts[True, False]["jpeg_files"] == counts[False, False]["jpeg_files"] + n_base, counts
    assert counts[True, True]["jpeg_progressive_files"] == counts[False, True]["jpeg_progressive_files"] + n_prog == 1 + n_prog, counts
    with open(os.path.join(tmp, "ok"), "w") as f:
        f.write("1")


def test_pipeline_with_the_switch_on_gives_the_same_vectors(tmp_path):
    """encode_files(device_jpeg_layouts=True) yields the vectors and the failed files of the switch off, plain and with
    device_progressive + jpeg_fused, and counts the files it added under jpeg_layout_files"""
    code = f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); " \
           f"import test_jpeg_layouts_gpu as t; t._layouts_pipeline_worker({str(tmp_path)!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "ok").read_text() == "1"
