"""PNG files with metadata chunks, and 16-bit RGB PNG files -> vectors with `device_png_chunks` / `device_png_deep` on and off:
build-index.py's loop (pipeline.encode_files, ViT-B/32 with random weights, 16 decode workers, `device_png` on in both settings) on
one box, in one process, the two settings in turn for `--rounds` rounds (default 5) behind two warm-up passes each. Off, the files
are Pillow's in the 16 workers; on, the workers check the chunks (png_parse.parse(chunks=True): a bounded inflate of the profile and
the text) or hand over the 16-bit stream, and the device inflates and reconstructs it (csrc/png.hip). Every round's time is printed,
with the fastest and the median per setting (other people's work shares the host: the spread says how far a difference can be
trusted). The timed window ends when every batch's vectors are on the host, so the device has finished. The vectors of the two
settings are compared, bit for bit.

Three sets of 224 x 224 files, filter Sub on every row, one zlib stream at level 6:
  screen_meta  a screenshot-like 8-bit RGB picture that carries what a macOS screenshot carries: iCCP (a 3 KB profile), eXIf, iTXt
               (XMP), pHYs and iDOT - the switch is device_png_chunks
  photo16      a photo-like 16-bit RGB picture whose low bytes are noise (a scan, a camera-raw export) - device_png_deep
  render16     a screenshot-like 16-bit RGB picture whose low bytes repeat the high bytes (8-bit content exported at depth 16)
Prints one JSON line per set and a table. usage: python tools/png_chunks_deep_ab.py [--rounds N] [--sets screen_meta,...]"""
import json
import multiprocessing as mp
import os
import statistics
import struct
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from png_interlaced_ab import chunk, pixels  # noqa: E402

H = W = 224
N, DISTINCT = 435, 87                                        # files per batch, distinct files
SETS = {"screen_meta": ("device_png_chunks", "png_chunk_files"), "photo16": ("device_png_deep", "png_deep_files"),
        "render16": ("device_png_deep", "png_deep_files")}


def sub_rows(b):
    """uint8 [h][w][unit] -> the scanlines with filter Sub on every row"""
    d = b.astype(np.int16)
    d[:, 1:] -= b[:, :-1]
    return np.hstack([np.ones((b.shape[0], 1), np.uint8), (d & 255).astype(np.uint8).reshape(b.shape[0], -1)]).tobytes()


def picture(name, seed):
    rng = np.random.default_rng(1000 + seed)
    if name == "screen_meta":
        a = pixels("screen", seed, H, W)
        profile = rng.integers(0, 256, 3144, dtype=np.uint8).tobytes()[:1500] * 2          # compresses about as a display profile does
        xmp = b"XML:com.adobe.xmp\0\0\0\0\0<x:xmpmeta xmlns:x='adobe:ns:meta/'><rdf:RDF><exif:PixelXDimension>448</exif:PixelXDimension></rdf:RDF></x:xmpmeta>"
        before = (chunk(b"iCCP", b"Display P3\0\0" + zlib.compress(profile)) + chunk(b"eXIf", b"MM\0*\0\0\0\x08\0\x01\x01\x12\0\x03\0\0\0\x01\0\x01\0\0\0\0\0\0") +
                  chunk(b"pHYs", struct.pack(">IIB", 5669, 5669, 1)) + chunk(b"iTXt", xmp) + chunk(b"iDOT", struct.pack(">7I", 2, 0, 112, 40, 112, 112, 9000)))
        return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + before +
                chunk(b"IDAT", zlib.compress(sub_rows(a), 6)) + chunk(b"IEND", b""))
    a = pixels("smooth" if name == "photo16" else "screen", seed, H, W)
    low = rng.integers(0, 256, a.shape, dtype=np.uint8) if name == "photo16" else a
    b = np.stack([a, low], axis=3).reshape(H, W, 6)            # each sample's high byte first
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 16, 2, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(sub_rows(b), 6)) + chunk(b"IEND", b""))


def main():
    import shutil
    import tempfile
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    sets = sys.argv[sys.argv.index("--sets") + 1].split(",") if "--sets" in sys.argv else list(SETS)
    import clipmi
    pool = clipmi.pipeline.DecodePool(16)                    # before the GPU is touched
    d = tempfile.mkdtemp(prefix="clipmi_png_cd_")
    rows = []
    try:
        with mp.get_context("spawn").Pool(16) as gen:        # (fresh processes: nothing here has touched the GPU)
            corpora = {s: gen.starmap(picture, [(s, k) for k in range(DISTINCT)]) for s in sets}
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        for s in sets:
            switch, stat = SETS[s]
            blobs = corpora[s]
            p = clipmi.png_parse.parse(blobs[0], chunks=True, deep=True)
            assert (p.chunks, p.depth) == ((1, 8) if s == "screen_meta" else (0, 16))
            paths = []
            for k in range(2 * N):
                paths.append(os.path.join(d, f"{s}_{k:05d}.png"))
                with open(paths[-1], "wb") as f:
                    f.write(blobs[k % DISTINCT])
            kw = dict(batch=N, pool=pool, device_jpeg_kb=16384, device_png=True)
            times, kept, stage, vectors = {False: [], True: []}, {}, {}, {}
            for _ in range(2):                               # warm-up: region sizes (they grow with the files), workspaces, pinned segments
                for on in (False, True):
                    for _ in clipmi.pipeline.encode_files(model, paths, **{switch: on}, **kw):
                        pass
            for _ in range(rounds):
                for on in (False, True):
                    st = {}
                    t0 = time.perf_counter()
                    out = list(clipmi.pipeline.encode_files(model, paths, stats=st, **{switch: on}, **kw))
                    dt = time.perf_counter() - t0             # (every batch's vectors were copied to the host: the device is done)
                    assert sum(len(ok) for ok, _, _ in out) == len(paths)
                    if not times[on] or dt < min(times[on]):
                        kept[on] = st.get(stat, 0)
                        stage[on] = {k: round(v, 2) for k, v in st.items() if k.endswith("_s")}
                    times[on].append(dt)
                    vectors[on] = np.concatenate([v for _, v, _ in out])
            assert np.array_equal(vectors[False], vectors[True]), "the two settings give different vectors"
            rate = lambda t: round(len(paths) / t, 1)  # noqa: E731
            row = dict(set=s, switch=switch, files=len(paths), size=[W, H], mean_file_kb=round(sum(map(len, blobs)) / DISTINCT / 1024, 1), rounds=rounds,
                       pillow_images_per_s=rate(min(times[False])), device_images_per_s=rate(min(times[True])),
                       pillow_median_images_per_s=rate(statistics.median(times[False])),
                       device_median_images_per_s=rate(statistics.median(times[True])),
                       pillow_round_s=[round(t, 3) for t in times[False]], device_round_s=[round(t, 3) for t in times[True]],
                       device_files=kept[True], pillow_files=kept[False], same_vectors=True,
                       pillow_stage_s=stage[False], device_stage_s=stage[True])
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        pool.close()
        shutil.rmtree(d, ignore_errors=True)
    print(f"{'set':14s} {'files':>6s} {'KB/file':>8s} {'Pillow img/s':>13s} {'(median)':>9s} {'device img/s':>13s} {'(median)':>9s} {'on device':>10s}")
    for r in rows:
        print(f"{r['set']:14s} {r['files']:6d} {r['mean_file_kb']:8.1f} {r['pillow_images_per_s']:13.1f} {r['pillow_median_images_per_s']:9.1f} "
              f"{r['device_images_per_s']:13.1f} {r['device_median_images_per_s']:9.1f} {r['device_files']:10d}")


if __name__ == "__main__":
    main()
