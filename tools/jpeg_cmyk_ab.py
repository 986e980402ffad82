"""Files to vectors over a directory of four-component JPEG files (CMYK as Pillow's encoder writes them: Adobe transform 0, component
0 sampled 2x2 by default) with the device decode of such files on (encode_files(device_jpeg_cmyk=True)) against off, where Pillow
decodes them in the worker processes - the path every such file took before the switch existed. One process on one GPU, the decode
workers started first, both forms alternating: two warm-up runs of each, then `--reps` repetitions; the vectors of the two forms
are compared bit for bit. The pictures are tests/jpeg_cmyk.py's smooth4: a photo's statistics in four bands.

  python tools/jpeg_cmyk_ab.py [--files 435] [--height 1500] [--width 2000] [--subsampling 2] [--ycck] [--reps 5] [--workers 16] [--out FILE]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def one_file(args):
    import jpeg_cmyk
    seed, h, w, sub, ycck = args
    b = jpeg_cmyk.cmyk_file(jpeg_cmyk.smooth4(np.random.default_rng(seed), h, w), subsampling=sub, quality=90)
    return jpeg_cmyk.as_ycck(b) if ycck else b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=435)
    ap.add_argument("--height", type=int, default=1500)
    ap.add_argument("--width", type=int, default=2000)
    ap.add_argument("--subsampling", type=int, default=2, choices=(0, 1, 2))
    ap.add_argument("--ycck", action="store_true", help="the files' Adobe transform set to 2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import multiprocessing as mp
    with mp.get_context("fork").Pool(min(a.workers, len(os.sched_getaffinity(0)))) as procs:        # before the GPU is touched
        blobs = procs.map(one_file, [(9000 + k, a.height, a.width, a.subsampling, a.ycck) for k in range(a.files)], chunksize=4)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for k, b in enumerate(blobs):
            paths.append(os.path.join(tmp, f"{k:04d}.jpg"))
            with open(paths[-1], "wb") as f:
                f.write(b)
        import clipmi
        with clipmi.pipeline.DecodePool(a.workers) as pool:                                         # before the GPU is touched, too
            import torch
            if not torch.cuda.is_available():
                sys.exit("tools/jpeg_cmyk_ab.py measures on a GPU: none found")
            model = clipmi.CLIP(clipmi.weights.random_state_dict("ViT-B/32", seed=0), device="cuda:0")
            say(f"# tools/jpeg_cmyk_ab.py --files {a.files} --subsampling {a.subsampling}{' --ycck' if a.ycck else ''} --reps {a.reps} "
                f"--workers {a.workers}: {torch.cuda.get_device_name(0)}, ViT-B/32, batch {a.files}")
            say(f"{a.files} {'YCCK' if a.ycck else 'CMYK'} files of {a.width} x {a.height}, quality 90, {sum(map(len, blobs)) / a.files / 1024:.0f} KB each")

            def run(on):
                stats = {}
                pool.jpeg_cap_hint = (max(map(len, blobs)) * 5 // 4 + 65535) // 65536 * 65536       # regions every file fits, from the first batch
                t0 = time.perf_counter()
                res = list(clipmi.pipeline.encode_files(model, paths, batch=a.files, pool=pool, device_resize_mb=0, device_jpeg_cmyk=on,
                                                        stats=stats))
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert sum(len(r[0]) for r in res) == a.files and stats.get("jpeg_cmyk_files", 0) == (a.files if on else 0), stats
                return dt, np.concatenate([r[1] for r in res]), stats

            for _ in range(2):
                for on in (False, True):
                    run(on)
            secs, feats, last = {False: [], True: []}, {}, {}
            for _ in range(a.reps):
                for on in (False, True):                       # alternating
                    dt, feats[on], last[on] = run(on)
                    secs[on].append(dt)
            same = np.array_equal(feats[False].view(np.uint32), feats[True].view(np.uint32))
            med = {}
            for on in (False, True):
                v = sorted(secs[on])
                med[on] = v[len(v) // 2]
                st = last[on]
                say(f"  switch {'on  (device)' if on else 'off (Pillow)'}: median {med[on] * 1e3:8.1f} ms, min {v[0] * 1e3:8.1f}, max {v[-1] * 1e3:8.1f}"
                    f"  -> {a.files / med[on]:8.1f} files/s; stages busy decode {st['decode_s'] * 1e3:.0f} copy {st['copy_s'] * 1e3:.0f} "
                    f"encode {st['encode_s'] * 1e3:.0f} ms")
            say(f"  on / off = {med[False] / med[True]:.2f} x the files/s (medians); vectors bit-equal: {same}")
            assert same
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
