"""The host tables of the transform (decode_worker.coeffs_window, resize_plan, nearest_plan) against Pillow itself, densely, on
hard-edged data; and the condition on the saturating corpus that tests/test_transform_saturating_gpu.py rests on. No GPU.

`int(n_px * h / w)`, `round((w - n_px) / 2.0)` (half to even) and `trunc(center +- support + 0.5)` are where a table leaves
Pillow by one tap at one size in a thousand: the sweeps below visit every size, not thirty.

The four classes of a plan. resize_plan resamples both axes or neither: `nw != w` whenever anything is resized (the shorter side
becomes n_px and was not n_px), and then `nh = int(n_px * h / w)` differs from h as well - for w > n_px it is below h, for
w < n_px it is at least h (1 + 1 / w) >= h + 1, h being the longer side. test_the_planner_resamples_both_axes_or_neither pins
that over the grids; jobs that resample one axis only exist as hand-made jobs (tests/test_transform_exact_gpu.py)."""
import io

import numpy as np
import pytest
from PIL import Image

import transform_cases as T
from clipmi import decode_worker as dw

LENGTHS = list(range(1, 1500)) + [2000, 3000, 4000, 4096, 6000, 8191, 12288]


def long_side(length, n_px):
    """The length-dependent output of the sweep: the long side load_uint8 arrives at for an image of sides `length` and a
    shorter side of 3/8 .. 7/8 of it (the eighths in turn with the length), so n_px x 1.14 .. 2.67 and every rounding of
    int(n_px * h / w) that goes with them"""
    short = max(1, length * (3 + length % 5) // 8)
    return int(n_px * length / short)


def test_coefficient_tables_equal_pillows_on_every_length():
    """coeffs_window over a whole axis, for every source length and three output lengths per n_px, reproduces Image.resize(BICUBIC)
    of a 1-row image of random 0 / 255 byte for byte (0 differences over about 9 000 pairs), and the sweep clips on both sides."""
    rng = np.random.default_rng(5)
    pairs = wrong = below = above = 0
    first_wrong = None
    for length in LENGTHS:
        row = (rng.integers(0, 2, (1, length)) * 255).astype(np.uint8)
        im = Image.fromarray(row, "L")
        for n_px in (224, 336):
            for out in sorted({n_px, int(1.5 * n_px), long_side(length, n_px)}):
                if out == length:
                    continue
                got, q = T.resample_ref(row, *dw.coeffs_window(length, out, 0, out), axis=1)
                ref = np.asarray(im.resize((out, 1), Image.BICUBIC))
                pairs += 1
                below += int((q < 0).sum())
                above += int((q > 255).sum())
                if got.shape != ref.shape or not np.array_equal(got, ref):
                    wrong += 1
                    first_wrong = first_wrong or (length, out)
    print(f"{pairs} (source, output) pairs, {wrong} differ from Pillow {Image.__version__}; sums below 0: {below}, above 255: {above}")
    assert pairs >= 8900
    assert wrong == 0, f"{wrong} pairs differ, the first: {first_wrong}"
    assert below > 1000 and above > 1000


def save_png(a, mode=None, palette=None):
    im = Image.fromarray(a, mode)
    if palette is not None:
        im.putpalette(np.asarray(palette, np.uint8).reshape(-1).tolist())
    buf = io.BytesIO()
    im.save(buf, format="PNG", compress_level=0)
    buf.seek(0)
    return buf


def fine_grid():
    return [(w, h, 8) for w in range(1, 65) for h in range(1, 65)]


def coarse_grid():
    """1 .. 700 in steps of 7 on both axes at n_px 32, thinned to the pairs whose grid indices add up to a multiple of 10 (1 000 of
    10 000 pairs: the full grid takes minutes); the step never lands on n_px, so the sides 31, 32 and 33 are paired with every
    side of the grid, both ways round - the crop-only class and its two neighbours"""
    sides = list(range(1, 701, 7))
    grid = [(w, h, 32) for i, w in enumerate(sides) for j, h in enumerate(sides) if (i + j) % 10 == 0]
    for s in (31, 32, 33):
        grid += [(s, t, 32) for t in sides] + [(t, s, 32) for t in sides]
    return grid


def plan_class(plan):
    return (plan["need_h"], plan["need_v"])


@pytest.mark.parametrize("grid", [fine_grid, coarse_grid])
def test_whole_plans_equal_load_uint8(grid):
    """transform_ref over resize_plan == load_uint8 of the same pixels, for every size of the grid: the resized sizes, the
    half-to-even crop offsets, need_h / need_v and the window all have to be Pillow's. As such too: every tap inside the image,
    r0 / nrows exactly the rows the window reads."""
    rng = np.random.default_rng(6)
    wrong, off, classes = [], [], set()
    cases = grid()
    for k, (w, h, n_px) in enumerate(cases):
        a = T.hard(rng, h, w, k)
        plan = dw.resize_plan(w, h, n_px)
        classes.add(plan_class(plan))
        why = T.window_in_bounds(plan, w, h, n_px)
        if why:
            off.append((w, h, why))
            continue
        ref = dw.load_uint8(save_png(a), n_px)
        if not np.array_equal(T.transform_ref(a, plan, n_px, "rgb"), ref):
            wrong.append((w, h))
    print(f"{len(cases)} sizes, classes (need_h, need_v) seen: {sorted(classes)}, {len(wrong)} differ")
    assert not off, off[:5]
    assert not wrong, f"{len(wrong)} sizes differ from load_uint8, the first: {wrong[:5]}"
    assert classes == {(0, 0), (1, 1)}


def test_the_planner_resamples_both_axes_or_neither():
    """(this module's docstring) every size up to 700 x 700 at n_px 8, 32 and 224: need_h == need_v, and nothing is resampled
    exactly when the shorter side is n_px"""
    for n_px in (8, 32, 224):
        side = np.arange(1, 701)
        for w in side:
            h = side
            short_w = w <= h
            nh = np.where(short_w, (n_px * h / w).astype(np.int64), n_px)
            nw = np.where(short_w, n_px, (n_px * w / h).astype(np.int64))
            keep = np.where(short_w, w == n_px, h == n_px)
            assert ((nw != w) == (nh != h))[~keep].all() and (nw != w)[~keep].all()
        for w, h in ((n_px, n_px), (n_px, 3 * n_px), (5 * n_px, n_px), (n_px + 1, n_px), (n_px - 1, n_px), (n_px, n_px - 1)):
            p = dw.resize_plan(w, h, n_px)
            assert plan_class(p) == ((0, 0) if min(w, h) == n_px else (1, 1)), (w, h)


def test_nearest_plans_equal_load_uint8():
    """nearest_plan on the fine grid against load_uint8 of a mode-P file whose index encodes its coordinate (x + 16 y mod 256: a
    step in either direction changes the index) under a palette that is one-to-one"""
    palette = np.stack([np.arange(256), 255 - np.arange(256), np.arange(256) * 7 % 256], axis=1).astype(np.uint8)
    wrong, off = [], []
    for (w, h, n_px) in fine_grid():
        yy, xx = np.mgrid[0:h, 0:w]
        idx = ((xx + 16 * yy) % 256).astype(np.uint8)
        plan = dw.nearest_plan(w, h, n_px)
        cols, rows = plan["hcoef"], plan["vcoef"]
        if not (cols.min() >= 0 and cols.max() < w and rows.min() >= 0 and rows.max() < h and
                (plan["r0"], plan["nrows"]) == (int(rows.min()), int(rows.max()) - int(rows.min()) + 1)):
            off.append((w, h))
            continue
        if not np.array_equal(T.transform_ref((idx, palette), plan, n_px, "index"), dw.load_uint8(save_png(idx, "P", palette), n_px)):
            wrong.append((w, h))
    assert not off, off[:5]
    assert not wrong, f"{len(wrong)} sizes differ from load_uint8, the first: {wrong[:5]}"


# ---- the saturating corpus: a condition on the inputs of tests/test_transform_saturating_gpu.py, so that it cannot pass vacuously
@pytest.mark.parametrize("which", ["corpus", "big_corpus"])
def test_every_corpus_file_clips_in_both_passes_and_both_directions(which):
    """Per file, from the CPU restatement of its decoder (oracle.jpeg_oracle, jpeg_progressive.decode, jpeg_layouts' and
    jpeg_cmyk's restatements, png_cases / png_mode_cases / png_interlace_cases cpu_decode): the unclipped sums below 0 and above
    255 of the horizontal and of the vertical pass are all counted above zero; a file with alpha sends colours above their alpha
    into the un-premultiply; and the restated transform is load_uint8's, so the counts are those of the bytes the GPU test compares."""
    files, n_px = (T.corpus(), T.N_PX) if which == "corpus" else (T.big_corpus(), T.BIG_N_PX)
    assert {f.path for f in files} == ({"jpeg", "layouts", "cmyk", "png", "interlaced"} if which == "corpus" else {"jpeg"})
    for f in files:
        stats = {}
        ref = T.file_ref(f, n_px, stats)
        print(f"{f.name:40s} { {k: v for k, v in stats.items() if k not in ('hq', 'vq')} }")
        for key in ("h_below", "h_above", "v_below", "v_above"):
            assert stats[key] > 0, (f.name, key, stats)
        if f.kind == "rgba":
            assert stats["over_alpha"] > 0, (f.name, stats)
        assert np.array_equal(ref, T.load_uint8_blob(f.blob, n_px)), f.name
    if which == "corpus":
        wide = [f for f in files if T._size(f) == T.WIDE[::-1]]
        ht = T.tables_of(dw.resize_plan(*T.WIDE[::-1], n_px), n_px)[0]
        assert len(wide) == 1 and int((ht[0] + ht[1]).max() - ht[0].min()) > 512           # (the window spans more than JF_SPAN columns)
    else:
        assert all(dw.resize_plan(*T._size(f), n_px)["hk"] > 512 for f in files)
