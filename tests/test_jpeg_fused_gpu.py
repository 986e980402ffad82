"""jpeg_color_resize_h_kernel (csrc/jpeg.hip) through jpeg.transform_files and pipeline.encode_files(jpeg_fused=True): the
transform's pixels straight from the decoder's sample planes equal, byte for byte, the unfused path's (decode entry, full-size RGB
rows, clipmi_resize_crop_rgb8) and Pillow's own (decode_worker.load_uint8: Image.open + bicubic resize + centre crop)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from clipmi import jpeg, jpeg_parse
from clipmi.decode_worker import load_uint8
from test_jpeg import encode, smooth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w): both axes resampled | neither | crop only, top > 0 | portrait | odd sizes: the dw-1 / dh-1 edges of fancy upsampling |
# panorama: most columns discarded, the window starts at an odd column | upscaling | smaller than an MCU row / column | width 3:
# the parsers take it at 4:4:4 only (at 2x sampling jpeg_parse refuses (w + 1) // 2 <= 2: "too narrow for fancy upsampling", so
# those files are Pillow's on every path) | width 5: the narrowest file the parsers do take with 2x sampling
SIZES = [(300, 400), (224, 224), (250, 224), (500, 333), (301, 451), (225, 1800), (100, 75), (17, 16), (9, 3), (9, 5)]
NARROW = (9, 3)
PHOTO = (1500, 2000)              # about 27 taps per output, several column chunks


def make_files(rng):
    """-> [(label, file contents)]: the photo and SIZES at every sampling, and each at 4:2:0 (NARROW: 4:4:4) as a progressive file
    too; a grey and an optimised-table file"""
    photo = smooth(rng, *PHOTO)
    files = [("photo", encode(photo, quality=90, subsampling=2)),
             ("photo progressive", encode(photo, quality=90, subsampling=2, progressive=True))]
    for (h, w) in SIZES:
        a = smooth(rng, h, w)
        for sub in (0, 1, 2):
            files.append((f"{h}x{w} sub{sub}", encode(a, quality=90, subsampling=sub)))
        files.append((f"{h}x{w} progressive", encode(a, quality=90, subsampling=0 if (h, w) == NARROW else 2, progressive=True)))
    files.append(("grey", encode(smooth(rng, 300, 260)[..., 0], quality=85)))
    files.append(("optimised", encode(smooth(rng, 260, 300), quality=85, optimize=True)))
    return files


def device_kind(blob):
    """"baseline", "progressive" or None (a file the host parsers leave to Pillow)"""
    for kind, parser in (("baseline", jpeg_parse.parse), ("progressive", jpeg_parse.parse_progressive)):
        try:
            parser(blob)
            return kind
        except jpeg_parse.Unsupported:
            pass
    return None


def pillow_transform(tmp_path, blobs, n_px):
    out = []
    for k, b in enumerate(blobs):
        path = str(tmp_path / f"{k}.jpg")
        with open(path, "wb") as f:
            f.write(b)
        out.append(load_uint8(path, n_px))
    return np.stack(out)


def both(blobs, n_px):
    """-> (fused pixels, fused status, unfused pixels, unfused status) as numpy arrays"""
    st = jpeg.stage_transform(blobs, n_px, DEV)
    res = []
    for fused in (True, False):
        out, status = jpeg.run_transform(st, fused)
        res += [out.cpu().numpy(), status.cpu().numpy()]
    return res


def test_fused_equals_unfused_equals_pillow(tmp_path):
    files = make_files(np.random.default_rng(41))
    kinds = [device_kind(b) for _, b in files]
    refused = [label for (label, _), k in zip(files, kinds) if k is None]
    assert refused == ["9x3 sub1", "9x3 sub2"]                # not the device's on any path: transform_files says so
    with pytest.raises(jpeg_parse.Unsupported):
        jpeg.transform_files([b for (label, b) in files if label == "9x3 sub2"], 224, DEV)
    files = [f for f, k in zip(files, kinds) if k is not None]
    kinds = [k for k in kinds if k is not None]
    assert kinds.count("progressive") == len(SIZES) + 1 and kinds.count("baseline") == 3 * len(SIZES) - 2 + 3    # both entries run
    blobs = [b for _, b in files]
    ref = pillow_transform(tmp_path, blobs, 224)
    out, status = jpeg.transform_files(blobs, 224, DEV, fused=True)
    plain, plain_status = jpeg.transform_files(blobs, 224, DEV, fused=False)
    assert out.shape == (len(blobs), 3, 224, 224) and out.dtype == torch.uint8 and status.dtype == torch.int32
    assert not status.cpu().numpy().any() and not plain_status.cpu().numpy().any()
    out, plain = out.cpu().numpy(), plain.cpu().numpy()
    for k, (label, _) in enumerate(files):
        assert np.array_equal(plain[k], ref[k]), f"unfused != Pillow: {label}"
        assert np.array_equal(out[k], plain[k]), f"fused != unfused: {label}"
        assert np.array_equal(out[k], ref[k]), f"fused != Pillow: {label}"


def test_a_damaged_file_among_good_ones(tmp_path):
    """Bit-flipped files (test_jpeg_gpu's test_corrupt_entropy_data...'s kind) and one whose data ends early, between two good
    files: the fused path reports each as the unfused one does, returns the unfused pixels where both decode it, and the
    neighbours' pixels are Pillow's."""
    rng = np.random.default_rng(23)
    blob = encode(smooth(rng, 296, 328), quality=85)
    start = blob.index(b"\xff\xda") + 14
    damaged = []
    for _ in range(24):
        bad = bytearray(blob)
        pos = start + int(rng.integers(0, len(blob) - start - 4))
        bad[pos] ^= 1 << int(rng.integers(0, 8))
        try:
            jpeg_parse.parse(bytes(bad))
        except jpeg_parse.Unsupported:
            continue
        damaged.append(bytes(bad))
    assert len(damaged) >= 4
    short = jpeg_parse.parse(blob)
    short.stream = short.stream[:len(short.stream) // 2]
    good = [encode(smooth(rng, 300, 400), quality=90, subsampling=2), encode(smooth(rng, 240, 230), quality=90, subsampling=1)]
    batch = [good[0]] + damaged + [short] + [good[1]]
    out, status, plain, plain_status = both(batch, 224)
    assert np.array_equal(status, plain_status)
    assert status[0] == 0 and status[-1] == 0 and status[-2] == 2
    ref = pillow_transform(tmp_path, good, 224)
    assert np.array_equal(out[0], ref[0]) and np.array_equal(out[-1], ref[1])
    for k in range(len(batch)):
        if status[k] == 0:
            assert np.array_equal(out[k], plain[k])


def test_vit_l_size(tmp_path):
    """n_px = 336: coefficient blocks and chunking that are not the 224 ones"""
    rng = np.random.default_rng(43)
    blobs = [encode(smooth(rng, 400, 600), quality=90, subsampling=2), encode(smooth(rng, 700, 336), quality=90, subsampling=2)]
    ref = pillow_transform(tmp_path, blobs, 336)
    out, status, plain, plain_status = both(blobs, 336)
    assert not status.any() and not plain_status.any()
    assert np.array_equal(plain, ref) and np.array_equal(out, plain)


def test_outputs_whose_taps_exceed_a_chunk_are_computed_tap_by_tap(tmp_path):
    """n_px = 8 over sides of 1100 and more: an output has 553 - 603 taps (resize.pack_jobs' hk), more source columns than a chunk
    of jpeg_color_resize_h_kernel stages (JF_SPAN = 512), so every output is summed tap by tap from the planes in memory - the
    pixel function jpeg_color_kernel runs, called by the fused kernel. The odd sizes put the dw-1 / dh-1 edges of fancy upsampling
    under those taps; the 600 x 4000 panorama has 303 taps, few outputs per chunk under the coefficient limit (JF_COEF)."""
    rng = np.random.default_rng(45)
    files = []
    for (h, w) in [(1100, 1200), (1101, 1203), (1203, 1101)]:
        a = smooth(rng, h, w)
        for sub in (0, 1, 2):
            files.append((f"{h}x{w} sub{sub}", encode(a, quality=90, subsampling=sub)))
            files.append((f"{h}x{w} sub{sub} progressive", encode(a, quality=90, subsampling=sub, progressive=True)))
    files.append(("600x4000 sub2", encode(smooth(rng, 600, 4000), quality=90, subsampling=2)))
    kinds = [device_kind(b) for _, b in files]
    assert kinds == ["baseline", "progressive"] * 9 + ["baseline"]
    blobs = [b for _, b in files]
    ref = pillow_transform(tmp_path, blobs, 8)
    out, status = jpeg.transform_files(blobs, 8, DEV, fused=True)
    plain, plain_status = jpeg.transform_files(blobs, 8, DEV, fused=False)
    assert not status.cpu().numpy().any() and not plain_status.cpu().numpy().any()
    out, plain = out.cpu().numpy(), plain.cpu().numpy()
    for k, (label, _) in enumerate(files):
        assert np.array_equal(plain[k], ref[k]), f"unfused != Pillow: {label}"
        assert np.array_equal(out[k], plain[k]), f"fused != unfused: {label}"
        assert np.array_equal(out[k], ref[k]), f"fused != Pillow: {label}"


def _fused_pipeline_worker(tmp):
    """Own process, the product's start order (decode workers first, GPU second): a directory of baseline and progressive files of
    the sizes above beside a PNG and a CMYK JPEG (Pillow's), a file whose data ends early and a broken one."""
    sys.path.insert(0, ROOT)
    import clipmi
    from PIL import Image
    rng = np.random.default_rng(44)
    paths = []

    def put(name, data):
        p = os.path.join(tmp, name)
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
        return p

    for k, (label, b) in enumerate(make_files(rng)):
        put(f"a{k:02d}.jpg", b)
    Image.fromarray(smooth(rng, 250, 350)).save(os.path.join(tmp, "d.png"))
    paths.append(os.path.join(tmp, "d.png"))
    Image.fromarray(smooth(rng, 240, 320)).convert("CMYK").save(os.path.join(tmp, "e_cmyk.jpg"), quality=85)
    paths.append(os.path.join(tmp, "e_cmyk.jpg"))
    blob = encode(smooth(rng, 320, 320), quality=90)
    put("g_cut.jpg", blob[:len(blob) * 2 // 3] + b"\xff\xd9")               # parses, but the data ends early: the device reports it
    bad = put("h_broken.jpg", b"broken")
    assert 40 <= len(paths) <= 50
    import warnings
    warnings.simplefilter("ignore")
    runs, stats = {}, {}
    with clipmi.pipeline.DecodePool(3) as pool:                     # before anything initialises the GPU
        assert not torch.cuda.is_initialized()
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        for fused in (False, True):
            for group_mb in (32768, 8):                             # one group per kind; several (the photo: a group of its own)
                stats[fused, group_mb] = {}
                pool.jpeg_cap_hint = 4 << 20                        # every run starts with regions the photos (first batch) fit
                runs[fused, group_mb] = list(clipmi.pipeline.encode_files(
                    model, paths, batch=16, pool=pool, device_resize_mb=0, device_jpeg_kb=4096, device_progressive=True,
                    jpeg_group_mb=group_mb, jpeg_fused=fused, stats=stats[fused, group_mb]))
    plain = runs[False, 32768]
    for key, other in runs.items():
        assert [h[0] for h in plain] == [d[0] for d in other] and [h[2] for h in plain] == [d[2] for d in other], key
        for h, d in zip(plain, other):
            assert torch.equal(torch.from_numpy(h[1]), torch.from_numpy(d[1])), key
    failed = [p for h in plain for p in h[2]]
    assert bad in failed and len(failed) in (1, 2)                  # the cut file: whatever Pillow decides, both paths agree
    counts = {key: {k: v for k, v in s.items() if k.endswith("_files")} for key, s in stats.items()}
    assert all(c == counts[False, 32768] for c in counts.values()), counts
    assert counts[True, 32768]["jpeg_files"] >= 3 * len(SIZES) - 2 + 3 and counts[True, 32768]["jpeg_progressive_files"] == len(SIZES) + 1
    with open(os.path.join(tmp, "ok"), "w") as f:
        f.write("1")


def test_pipeline_with_the_fused_entries_gives_the_same_vectors(tmp_path):
    """encode_files(jpeg_fused=True) yields the vectors, the failed files and the device-decoded counts of jpeg_fused=False"""
    code = f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); " \
           f"import test_jpeg_fused_gpu as t; t._fused_pipeline_worker({str(tmp_path)!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "ok").read_text() == "1"
