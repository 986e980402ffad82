"""The fused JPEG transform (clipmi_jpeg_decode_transform_rgb8: colour conversion + horizontal pass straight from the sample
planes) against the unfused one (clipmi_jpeg_decode_rgb8 + clipmi_resize_crop_rgb8), in one process on one GPU:
435 photo-like baseline files of 2 000 x 1 500 and 870 files of 224 x 224 (the bench's shape), quality 90, 4:2:0, tools/jpeg_probe.py's
generator. Both forms go through jpeg.transform_files' two halves: the files are parsed, packed and copied once
(jpeg.stage_transform), and jpeg.run_transform is timed with device events - two warm-up runs of each form, then `--reps`
alternating repetitions; the outputs of the two forms are compared byte for byte. One whole transform_files call of each form
(parse and copy included) is timed by the host clock as well.

  python tools/jpeg_fused_ab.py [--form both|fused|unfused] [--photos 435] [--small 870] [--reps 5] [--cache DIR] [--out FILE]

--form fused / unfused runs one form only (a kernel trace of its own per form); --cache keeps the generated files between runs."""
import argparse
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def smooth(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 100 * np.sin(xx / 9.0 + yy / 17.0), 127 + 100 * np.cos(xx / 13.0 - yy / 7.0), (xx * 3 + yy * 2) % 256], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def one_file(args):
    from PIL import Image
    seed, h, w = args
    buf = io.BytesIO()
    Image.fromarray(smooth(np.random.default_rng(seed), h, w)).save(buf, format="JPEG", quality=90, subsampling=2)
    return buf.getvalue()


def files(n, h, w, cache, workers=16):
    """n seeded files of h x w, generated on `workers` processes (started before the GPU is touched) or read from the cache"""
    path = os.path.join(cache, f"jpeg_fused_ab_{n}_{h}x{w}.npz") if cache else None
    if path and os.path.exists(path):
        z = np.load(path)
        return [z[f"f{k}"].tobytes() for k in range(n)]
    import multiprocessing as mp
    with mp.get_context("fork").Pool(min(workers, len(os.sched_getaffinity(0)))) as pool:
        blobs = pool.map(one_file, [(1000 * h + k, h, w) for k in range(n)], chunksize=4)
    if path:
        os.makedirs(cache, exist_ok=True)
        np.savez(path, **{f"f{k}": np.frombuffer(b, np.uint8) for k, b in enumerate(blobs)})
    return blobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", default="both", choices=("both", "fused", "unfused"))
    ap.add_argument("--photos", type=int, default=435)
    ap.add_argument("--small", type=int, default=870)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cache", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sets = [("photos", a.photos, 1500, 2000), ("small", a.small, 224, 224)]
    blobs = {name: files(n, h, w, a.cache) for name, n, h, w in sets if n}
    import torch
    from clipmi import jpeg
    if not torch.cuda.is_available():
        sys.exit("tools/jpeg_fused_ab.py measures on a GPU: none found")
    dev = torch.device("cuda:0")
    forms = {"both": (False, True), "fused": (True,), "unfused": (False,)}[a.form]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/jpeg_fused_ab.py --form {a.form} --reps {a.reps}: {torch.cuda.get_device_name(0)}, n_px 224, quality 90, 4:2:0")
    for name, n, h, w in sets:
        if not n:
            continue
        items = [jpeg.parse(b) for b in blobs[name]]
        st = jpeg.stage_transform(items, 224, dev)
        torch.cuda.synchronize()
        outs = {}
        for _ in range(2):                                   # warm-up: code objects, the allocator's blocks
            for fused in forms:
                outs[fused] = jpeg.run_transform(st, fused)
        torch.cuda.synchronize()
        ms = {f: [] for f in forms}
        for _ in range(a.reps):
            for fused in forms:                              # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                outs[fused] = jpeg.run_transform(st, fused)
                e1.record()
                e1.synchronize()
                ms[fused].append(e0.elapsed_time(e1))
        for fused in forms:
            assert not outs[fused][1].any().item(), "a file was reported"
        whole = {}
        for fused in forms:                                  # the whole call, parse and copy included: host clock, once
            t0 = time.perf_counter()
            jpeg.transform_files(blobs[name], 224, dev, fused=fused)
            torch.cuda.synchronize()
            whole[fused] = (time.perf_counter() - t0) * 1e3
        kb = sum(len(b) for b in blobs[name]) / n / 1024
        say(f"{name}: {n} files of {w} x {h}, {kb:.0f} KB each")
        for fused in forms:
            v = sorted(ms[fused])
            say(f"  {'fused  ' if fused else 'unfused'} device stage per batch: median {v[len(v) // 2]:8.2f} ms, min {v[0]:8.2f}, max {v[-1]:8.2f}"
                f"  ({n / v[len(v) // 2]:.1f} k images/s); whole call incl. parse and copy {whole[fused]:8.1f} ms")
        if len(forms) == 2:
            same = torch.equal(outs[True][0], outs[False][0])
            med = {f: sorted(ms[f])[len(ms[f]) // 2] for f in forms}
            say(f"  fused / unfused = {med[True] / med[False]:.3f} (medians); outputs equal: {same}")
            assert same
        del st, outs
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
