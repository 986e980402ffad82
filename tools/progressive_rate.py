"""Progressive JPEG decode rate: the device path (host parse_progressive + clipmi_jpeg_decode_progressive_rgb8, pixels in HBM)
against Pillow's `Image.open(f).convert("RGB")` in 16 worker processes, on the same box, for one set of files:
  small  870 progressive 224 x 224 files, quality 85, photo-like content (smooth gradients + noise, 4:2:0)
  big    435 progressive 2 000 x 1 500 files, quality 85, photo-like content (4:2:0)
Prints one JSON line. Decode only: the files are in memory, no resize or encode. usage: python tools/progressive_rate.py small|big
With f2v: files -> vectors instead, build-index.py's loop (pipeline.encode_files, ViT-B/32, 16 decode workers) on the same files
written to a temporary directory, with device_progressive off (Pillow in the workers) and on.
usage: python tools/progressive_rate.py f2v small|big"""
import io
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np
from PIL import Image, ImageFile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def photo(seed, h, w):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    f = rng.uniform(20, 90, 6)
    a = np.stack([128 + 90 * np.sin(x / f[0] + y / f[1]), 128 + 70 * np.cos(x / f[2] - y / f[3]), 128 + 60 * np.sin((x + y) / f[4])], -1)
    a += rng.normal(0, 6, (h, w, 3)).astype(np.float32)
    ImageFile.MAXBLOCK = 1 << 24
    buf = io.BytesIO()
    Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=85, progressive=True)
    return buf.getvalue()


def _pillow(b):
    return np.asarray(Image.open(io.BytesIO(b)).convert("RGB")).shape


def sets(which):
    n, (h, w), distinct = (870, (224, 224), 870) if which == "small" else (435, (1500, 2000), 29)
    with mp.get_context("spawn").Pool(16) as pool:          # (fresh processes: nothing here has touched the GPU either way)
        files = pool.starmap(photo, [(s, h, w) for s in range(distinct)])
    return n, (h, w), [files[k % distinct] for k in range(n)], distinct


def files_to_vectors(which):
    import shutil
    import tempfile
    import clipmi
    pool = clipmi.pipeline.DecodePool(16)                    # before the GPU is touched
    n, (h, w), blobs, _ = sets(which)
    d = tempfile.mkdtemp(prefix="clipmi_prog_")
    try:
        paths = []
        for k, b in enumerate(blobs):
            paths.append(os.path.join(d, f"p{k:05d}.jpg"))
            with open(paths[-1], "wb") as f:
                f.write(b)
        paths *= 3 if which == "small" else 2
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        res = dict(set="f2v_" + which, files=len(paths), size=[w, h], batch=n)
        for on in (False, True):
            for _ in clipmi.pipeline.encode_files(model, paths[:n], batch=n, pool=pool, device_progressive=on):
                pass
            st = {}
            t0 = time.perf_counter()
            got = sum(len(ok) for ok, _, _ in clipmi.pipeline.encode_files(model, paths, batch=n, pool=pool, device_progressive=on,
                                                                            stats=st))
            dt = time.perf_counter() - t0
            key = "device" if on else "pillow"
            res[key + "_images_per_s"] = round(got / dt)
            res[key + "_progressive_on_device"] = st.get("jpeg_progressive_files", 0)
            res[key + "_stage_s"] = {k: round(v, 2) for k, v in st.items() if k.endswith("_s")}
        print(json.dumps(res), flush=True)
    finally:
        pool.close()
        shutil.rmtree(d, ignore_errors=True)


def main():
    if sys.argv[1:2] == ["f2v"]:
        return files_to_vectors(sys.argv[2] if len(sys.argv) > 2 else "small")
    which = sys.argv[1] if len(sys.argv) > 1 else "small"
    n, (h, w), blobs, distinct = sets(which)                 # (the Pillow processes are spawned: this one will open the GPU)
    import torch
    import clipmi
    dev = torch.device("cuda:0")
    got = clipmi.jpeg.decode_progressive_files(blobs[:distinct], dev)             # warm-up and a parity spot check
    for k in range(0, distinct, max(1, distinct // 8)):
        assert got[k] is not None and np.array_equal(got[k], np.asarray(Image.open(io.BytesIO(blobs[k])).convert("RGB")))
    dev_ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        items = [clipmi.jpeg.parse_progressive(b) for b in blobs]
        t1 = time.perf_counter()
        out, recs, status = clipmi.jpeg.decode_progressive_device(items, dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert int((status != 0).sum()) == 0
        dev_ms.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
        del out
    with mp.get_context("spawn").Pool(16) as pool:
        pool.map(_pillow, blobs[:32])
        t0 = time.perf_counter()
        pool.map(_pillow, blobs, chunksize=4)
        pil_s = time.perf_counter() - t0
    best = min(dev_ms, key=lambda t: t[0] + t[1])
    print(json.dumps(dict(set=which, files=n, size=[w, h], mean_file_kb=round(sum(map(len, blobs)) / n / 1024, 1),
                          device_parse_ms=round(best[0], 1), device_decode_ms=round(best[1], 1),
                          device_images_per_s=round(n / ((best[0] + best[1]) / 1e3)),
                          pillow16_images_per_s=round(n / pil_s))), flush=True)


if __name__ == "__main__":
    main()
