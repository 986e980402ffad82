"""Adam7-interlaced RGB PNG files -> vectors with `device_png_interlaced` on and off: build-index.py's loop (pipeline.encode_files,
ViT-B/32 with random weights, 16 decode workers, `device_png` on in both settings) on one box, in one process, the two settings in
turn for `--rounds` rounds (default 5) behind one warm-up pass each. Off, the files are Pillow's in the 16 workers; on, the device
inflates them and reconstructs the seven passes (csrc/png.hip). Every round's time is printed, with the fastest and the median per
setting (other people's work shares the host: the spread says how far a difference can be trusted). The timed window ends when
every batch's vectors are on the host, so the device has finished. The vectors of the two settings are compared, bit for bit.

Pillow's encoder writes no interlaced files, so the corpora come from a writer of their own: the picture's seven sub-images,
filter Sub on every pass row, one zlib stream at level 6. Two pictures (png_timing.py's "smooth", photo-like, and "screen",
screenshot-like) at 224 x 224 ("small") and 2 000 x 1 500 ("big").
Prints one JSON line per set and a table. usage: python tools/png_interlaced_ab.py [--rounds N] [--sets smooth:small,...]"""
import json
import multiprocessing as mp
import os
import statistics
import struct
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = {"small": (224, 224, 435, 87), "big": (1500, 2000, 58, 12)}          # h, w, files per batch, distinct files
PASSES = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def pixels(kind, seed, h, w):
    rng = np.random.default_rng(seed)
    if kind == "smooth":
        y, x = np.mgrid[0:h, 0:w].astype(np.float32)
        f = rng.uniform(20, 90, 6)
        a = np.stack([128 + 90 * np.sin(x / f[0] + y / f[1]), 128 + 70 * np.cos(x / f[2] - y / f[3]), 128 + 60 * np.sin((x + y) / f[4])], -1)
        return np.clip(a + rng.normal(0, 3, (h, w, 3)), 0, 255).astype(np.uint8)
    a = np.full((h, w, 3), 245, np.uint8)
    for _ in range(max(1, h * w // 4000)):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        a[y0:y0 + int(rng.integers(1, 60)), x0:x0 + int(rng.integers(1, 200))] = rng.integers(0, 256, 3, dtype=np.uint8)
    for y0 in range(4, h - 8, 14):
        xs = rng.integers(0, 2, w // 3 + 1).repeat(3)[:w].astype(bool)
        a[y0:y0 + 7:2, xs] = 30
    return a


def chunk(cid, body):
    return struct.pack(">I", len(body)) + cid + body + struct.pack(">I", zlib.crc32(cid + body))


def adam7_file(a):
    """uint8 [h][w][3] -> an interlaced RGB PNG file, filter Sub on every row of every pass"""
    h, w, _ = a.shape
    rows = []
    for x0, y0, dx, dy in PASSES:
        sub = a[y0::dy, x0::dx]
        if sub.size:
            d = sub.astype(np.int16)
            d[:, 1:] -= sub[:, :-1]
            body = (d & 255).astype(np.uint8).reshape(sub.shape[0], -1)
            rows.append(np.hstack([np.ones((sub.shape[0], 1), np.uint8), body]).tobytes())
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 1)) +
            chunk(b"IDAT", zlib.compress(b"".join(rows), 6)) + chunk(b"IEND", b""))


def picture(kind, seed, h, w):
    return adam7_file(pixels(kind, seed, h, w))


def main():
    import shutil
    import tempfile
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    sets = (sys.argv[sys.argv.index("--sets") + 1].split(",") if "--sets" in sys.argv else
            [f"{k}:{s}" for s in ("small", "big") for k in ("smooth", "screen")])
    import clipmi
    pool = clipmi.pipeline.DecodePool(16)                    # before the GPU is touched
    d = tempfile.mkdtemp(prefix="clipmi_png_lace_")
    rows = []
    try:
        with mp.get_context("spawn").Pool(16) as gen:        # (fresh processes: nothing here has touched the GPU)
            corpora = {s: gen.starmap(picture, [(s.split(":")[0], k, *SIZES[s.split(":")[1]][:2]) for k in range(SIZES[s.split(":")[1]][3])])
                       for s in sets}
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        for s in sets:
            h, w, n, distinct = SIZES[s.split(":")[1]]
            blobs = corpora[s]
            assert clipmi.png_parse.parse(blobs[0], interlaced=True).interlace == 1
            paths = []
            for k in range(2 * n):
                paths.append(os.path.join(d, f"{s.replace(':', '_')}_{k:05d}.png"))
                with open(paths[-1], "wb") as f:
                    f.write(blobs[k % distinct])
            kw = dict(batch=n, pool=pool, device_jpeg_kb=16384, device_png=True)
            times, kept, stage, vectors = {False: [], True: []}, {}, {}, {}
            for _ in range(2):                               # warm-up: region sizes (they grow with the files), workspaces, pinned segments
                for on in (False, True):
                    for _ in clipmi.pipeline.encode_files(model, paths, device_png_interlaced=on, **kw):
                        pass
            for _ in range(rounds):
                for on in (False, True):
                    st = {}
                    t0 = time.perf_counter()
                    out = list(clipmi.pipeline.encode_files(model, paths, stats=st, device_png_interlaced=on, **kw))
                    dt = time.perf_counter() - t0             # (every batch's vectors were copied to the host: the device is done)
                    assert sum(len(ok) for ok, _, _ in out) == len(paths)
                    if not times[on] or dt < min(times[on]):
                        kept[on] = st.get("png_interlaced_files", 0)
                        stage[on] = {k: round(v, 2) for k, v in st.items() if k.endswith("_s")}
                    times[on].append(dt)
                    vectors[on] = np.concatenate([v for _, v, _ in out])
            assert np.array_equal(vectors[False], vectors[True]), "the two settings give different vectors"
            rate = lambda t: round(len(paths) / t, 1)  # noqa: E731
            row = dict(set=s, files=len(paths), size=[w, h], mean_file_kb=round(sum(map(len, blobs)) / distinct / 1024, 1), rounds=rounds,
                       pillow_images_per_s=rate(min(times[False])), device_images_per_s=rate(min(times[True])),
                       pillow_median_images_per_s=rate(statistics.median(times[False])),
                       device_median_images_per_s=rate(statistics.median(times[True])),
                       pillow_round_s=[round(t, 3) for t in times[False]], device_round_s=[round(t, 3) for t in times[True]],
                       device_interlaced_files=kept[True], pillow_interlaced_files=kept[False], same_vectors=True,
                       pillow_stage_s=stage[False], device_stage_s=stage[True])
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        pool.close()
        shutil.rmtree(d, ignore_errors=True)
    print(f"{'set':14s} {'files':>6s} {'KB/file':>8s} {'Pillow img/s':>13s} {'(median)':>9s} {'device img/s':>13s} {'(median)':>9s} {'on device':>10s}")
    for r in rows:
        print(f"{r['set']:14s} {r['files']:6d} {r['mean_file_kb']:8.1f} {r['pillow_images_per_s']:13.1f} {r['pillow_median_images_per_s']:9.1f} "
              f"{r['device_images_per_s']:13.1f} {r['device_median_images_per_s']:9.1f} {r['device_interlaced_files']:10d}")


if __name__ == "__main__":
    main()
