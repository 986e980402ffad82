"""PNG files -> vectors with the PNG decode on the device off and on: build-index.py's loop (pipeline.encode_files, ViT-B/32,
16 decode workers) on one box, in one process, the two settings in turn for `--rounds` rounds (default 3), the fastest run of
each reported (other people's work shares the host, so the minimum is the figure that says most about the code). Corpora, at
224 x 224 ("small") and 2 000 x 1 500 ("big"), written by Pillow's encoder at its default level:
  noise    incompressible pixels: zlib stores the first block and writes later ones as Huffman blocks of literals at about 8 bits
           each (its choice per block; the block kinds were not counted), so the file is as large as its scanlines
  smooth   photo-like: low-frequency waves plus a little noise, literals and short matches
  screen   screenshot-like: flat areas, text-like edges, long matches
and, for the alpha, palette and low-depth files `device_png_modes` adds, variants of smooth and screen (`--sets modes` runs the
eight of them): `<kind>_rgba` with an alpha plane (smooth: a slow wave; screen: opaque but for a few transparent boxes) and
`<kind>_p4`, quantised to a 16-colour palette and saved at 4 bits. For these the two settings are `device_png` on with
`device_png_modes` off (Pillow decodes them in the workers) and on.
Prints one JSON line per set and a table. usage: python tools/png_timing.py [--rounds N] [--sets noise:small,screen:big,...]
Under `rocprofv3 --kernel-trace --stats -- python tools/png_timing.py --rounds 1 --sets ...` the three png_* kernels' own
times are in the statistics file."""
import io
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = {"small": (224, 224, 435, 87), "big": (1500, 2000, 58, 12)}          # h, w, files per batch, distinct files


def picture(kind, seed, h, w):
    rng = np.random.default_rng(seed)
    kind, _, variant = kind.partition("_")
    if kind == "noise":
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == "smooth":
        y, x = np.mgrid[0:h, 0:w].astype(np.float32)
        f = rng.uniform(20, 90, 6)
        a = np.stack([128 + 90 * np.sin(x / f[0] + y / f[1]), 128 + 70 * np.cos(x / f[2] - y / f[3]), 128 + 60 * np.sin((x + y) / f[4])], -1)
        a = np.clip(a + rng.normal(0, 3, (h, w, 3)), 0, 255).astype(np.uint8)
    else:
        a = np.full((h, w, 3), 245, np.uint8)
        for _ in range(max(1, h * w // 4000)):
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            a[y0:y0 + int(rng.integers(1, 60)), x0:x0 + int(rng.integers(1, 200))] = rng.integers(0, 256, 3, dtype=np.uint8)
        for y0 in range(4, h - 8, 14):
            xs = rng.integers(0, 2, w // 3 + 1).repeat(3)[:w].astype(bool)
            a[y0:y0 + 7:2, xs] = 30
    buf = io.BytesIO()
    img = Image.fromarray(a)
    kw = {}
    if variant == "rgba":
        if kind == "smooth":
            y, x = np.mgrid[0:h, 0:w].astype(np.float32)
            alpha = np.clip(160 + 110 * np.sin(x / 70 + y / 110), 0, 255).astype(np.uint8)
        else:
            alpha = np.full((h, w), 255, np.uint8)
            for _ in range(max(1, h * w // 20000)):
                y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
                alpha[y0:y0 + int(rng.integers(1, 60)), x0:x0 + int(rng.integers(1, 200))] = 0
        img.putalpha(Image.fromarray(alpha))
    elif variant == "p4":
        img, kw = img.quantize(16), {"bits": 4}
    img.save(buf, format="PNG", **kw)
    return buf.getvalue()


def main():
    import shutil
    import tempfile
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3
    sets = (sys.argv[sys.argv.index("--sets") + 1].split(",") if "--sets" in sys.argv else
            [f"{k}:{s}" for s in ("small", "big") for k in ("noise", "smooth", "screen")])
    if sets == ["modes"]:
        sets = [f"{k}_{v}:{s}" for s in ("small", "big") for k in ("screen", "smooth") for v in ("rgba", "p4")]
    import clipmi
    pool = clipmi.pipeline.DecodePool(16)                    # before the GPU is touched
    d = tempfile.mkdtemp(prefix="clipmi_png_")
    rows = []
    try:
        with mp.get_context("spawn").Pool(16) as gen:        # (fresh processes: nothing here has touched the GPU)
            corpora = {s: gen.starmap(picture, [(s.split(":")[0], k, *SIZES[s.split(":")[1]][:2]) for k in range(SIZES[s.split(":")[1]][3])])
                       for s in sets}
        model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
        for s in sets:
            h, w, n, distinct = SIZES[s.split(":")[1]]
            blobs = corpora[s]
            paths = []
            for k in range(2 * n):
                paths.append(os.path.join(d, f"{s.replace(':', '_')}_{k:05d}.png"))
                with open(paths[-1], "wb") as f:
                    f.write(blobs[k % distinct])
            kw = dict(batch=n, pool=pool, device_jpeg_kb=16384)
            modes = "_" in s                                 # a variant for device_png_modes: that flag is what goes off and on
            flags = (lambda on: dict(device_png=True, device_png_modes=on)) if modes else (lambda on: dict(device_png=on))
            best, kept, stage = {False: 1e9, True: 1e9}, {}, {}
            for on in (False, True):                         # warm-up: region sizes, workspaces, page-locked segments
                for _ in clipmi.pipeline.encode_files(model, paths, **flags(on), **kw):
                    pass
            for _ in range(rounds):
                for on in (False, True):
                    st = {}
                    t0 = time.perf_counter()
                    got = sum(len(ok) for ok, _, _ in clipmi.pipeline.encode_files(model, paths, stats=st, **flags(on), **kw))
                    dt = time.perf_counter() - t0             # (every batch's vectors were copied to the host: the device is done)
                    assert got == len(paths)
                    if dt < best[on]:
                        best[on], kept[on] = dt, st.get("png_mode_files" if modes else "png_files", 0)
                        stage[on] = {k: round(v, 2) for k, v in st.items() if k.endswith("_s")}
            row = dict(set=s, files=len(paths), size=[w, h], mean_file_kb=round(sum(map(len, blobs)) / distinct / 1024, 1), rounds=rounds,
                       pillow_images_per_s=round(len(paths) / best[False], 1), device_images_per_s=round(len(paths) / best[True], 1),
                       device_png_files=kept[True], pillow_stage_s=stage[False], device_stage_s=stage[True])
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        pool.close()
        shutil.rmtree(d, ignore_errors=True)
    print(f"{'set':18s} {'files':>6s} {'KB/file':>8s} {'Pillow img/s':>13s} {'device img/s':>13s} {'on device':>10s}")
    for r in rows:
        print(f"{r['set']:18s} {r['files']:6d} {r['mean_file_kb']:8.1f} {r['pillow_images_per_s']:13.1f} {r['device_images_per_s']:13.1f} "
              f"{r['device_png_files']:10d}")


if __name__ == "__main__":
    main()
