"""The CLIP transform's resize + crop stage (csrc/resize.hip, jpeg_color_resize_h_kernel in csrc/jpeg.hip, the host tables of
decode_worker) for the tests that place known data at its edges: tests/test_transform_tables.py, test_transform_exact_gpu.py and
test_transform_saturating_gpu.py. No tests here.

  resample_ref      one pass of Pillow's 8-bit resampling in int64 numpy, the unclipped quotients beside the bytes
  transform_ref     the whole stage for the four pixel kinds, from a job's explicit fields - a plan of decode_worker.resize_plan /
                    nearest_plan, or a hand-made job no planner would emit
  pack_raw_jobs     hand-made jobs -> the records, coefficient array and pixel buffer the C entries take; launch() calls an entry
  hard-edged images 0/255 content, whose resampled sums leave 0..255 on both sides
  corpus()          small hard-edged files of every format the file-level transform entries take, each with its CPU restatement

Nothing here imports the kernels' logic: the pixel rules are png_mode_cases.premultiply / unpremultiply and jpeg_cmyk.cmyk2rgb,
which their own test files pin against Pillow.
"""
import functools
import io

import numpy as np

import jpeg_cmyk
import jpeg_layouts
import png_cases
import png_mode_cases as M
from clipmi import decode_worker as dw

PREC = 22                   # Pillow's PRECISION_BITS for 8-bit images
ONE = 1 << PREC
HALF = 1 << (PREC - 1)
POISON = 1 << 30            # a coefficient behind a job's tap count: one pixel of value 4 under it wraps an int32 sum


# ---- the reference ------------------------------------------------------------------------------------------------------------
def resample_ref(img, first, count, kk, axis):
    """One pass of Pillow's 8-bit resampling along `axis` of img uint8 [..]: output o is the sum over taps k < count[o] of
    img[first[o] + k] * kk[o][k], started at 2^21, shifted right by 22 (arithmetic) and clipped to 0..255.
    -> (the bytes, the unclipped quotients as int64): the second says what clipped, and on which side. Every tap must lie inside
    the image and every sum inside int32 (Pillow and the kernels accumulate in int32)."""
    a = np.moveaxis(np.asarray(img), axis, 0).astype(np.int64)
    first, count, kk = np.asarray(first, np.int64), np.asarray(count, np.int64), np.asarray(kk, np.int64)
    bad = np.flatnonzero((first < 0) | (count < 0) | (first + count > a.shape[0]) | (count > kk.shape[1]))
    assert bad.size == 0, f"output {bad[0]}: taps [{first[bad[0]]}, +{count[bad[0]]}) outside an axis of {a.shape[0]} or its {kk.shape[1]} coefficients"
    rest = int(np.prod(a.shape[1:], dtype=np.int64))
    if len(first) * kk.shape[1] * rest <= 1 << 22:           # small: every output's taps gathered at once, the others masked
        k = np.arange(kk.shape[1])[None, :]
        live = k < count[:, None]
        taps = a[np.where(live, first[:, None] + k, 0)]        # [outputs][k][..]
        acc = HALF + np.einsum("ok,ok...->o...", np.where(live, kk, 0), taps)
    else:
        acc = np.empty((len(first),) + a.shape[1:], np.int64)
        for o in range(len(first)):
            f, n = int(first[o]), int(count[o])
            acc[o] = HALF + np.tensordot(kk[o, :n], a[f:f + n], axes=1)
    assert acc.size == 0 or (int(acc.min()) >= -(1 << 31) and int(acc.max()) < (1 << 31)), "a sum leaves int32"
    q = acc >> PREC
    return np.moveaxis(np.clip(q, 0, 255).astype(np.uint8), 0, axis), np.moveaxis(q, 0, axis)


def block(first, count, kk):
    """an axis's tables -> the coefficient block the kernels read: [n] first tap | [n] count | [n][k] coefficients"""
    return np.concatenate([np.asarray(first, np.int64), np.asarray(count, np.int64), np.asarray(kk, np.int64).reshape(-1)]).astype(np.int32)


def tables_of(job, n_px):
    """A job's two axes as (first, count, kk) or None. job: a plan of decode_worker.resize_plan (its "hcoef" / "vcoef" blocks
    are taken apart), or a hand-made one with the tables themselves under "h" / "v"."""
    out = []
    for need, key, blk, k in (("need_h", "h", "hcoef", "hk"), ("need_v", "v", "vcoef", "vk")):
        if not job[need]:
            out.append(None)
        elif key in job:
            out.append(tuple(np.asarray(t, np.int64) for t in job[key]))
        else:
            c = np.asarray(job[blk], np.int64)
            out.append((c[:n_px], c[n_px:2 * n_px], c[2 * n_px:].reshape(n_px, job[k])))
    return out


def two_passes(px, job, n_px, stats=None):
    """the job's rows through both passes, as the kernels order them: [h][w][c] -> [n_px][n_px][c]. Only rows r0 .. r0 + nrows - 1
    are touched: a job whose window reads another row fails here."""
    r0, nrows = int(job["r0"]), int(job["nrows"])
    assert 0 <= r0 and nrows >= 1 and r0 + nrows <= px.shape[0]
    h, v = tables_of(job, n_px)
    x = px[r0:r0 + nrows]
    hq = vq = np.zeros(0, np.int64)
    if h:
        x, hq = resample_ref(x, *h, axis=1)
    else:
        assert 0 <= job["left"] and job["left"] + n_px <= px.shape[1]
        x = x[:, job["left"]:job["left"] + n_px]
    if v:
        x, vq = resample_ref(x, v[0] - r0, v[1], v[2], axis=0)
    else:
        assert 0 <= job["top"] - r0 and job["top"] - r0 + n_px <= nrows
        x = x[job["top"] - r0:job["top"] - r0 + n_px]
    if stats is not None:
        stats.update(hq=hq, vq=vq, h_below=int((hq < 0).sum()), h_above=int((hq > 255).sum()), v_below=int((vq < 0).sum()), v_above=int((vq > 255).sum()))
    return x


def transform_ref(pixels, job, n_px, kind, stats=None):
    """What the stage leaves in a job's output block, uint8 [3][n_px][n_px], from the job's explicit fields (r0, nrows, left, top,
    need_h, need_v and the tables: tables_of).
      "rgb"    pixels uint8 [h][w][3]: the two passes
      "rgba"   [h][w][4]: premultiplied, the two passes, un-premultiplied, where the job resamples an axis; else a crop. Alpha dropped.
      "cmyk"   [h][w][4]: four plain bands through the two passes, then Pillow's CMYK -> RGB
      "index"  (indices uint8 [h][w], palette uint8 [256][3]); the job's "hcoef" / "vcoef" are nearest_plan's source column of each
               output column and source row of each output row, CLAMPED into the image here as the kernel clamps them
    stats: a dict that receives how many unclipped sums of each pass lay below 0 and above 255 (h_below, h_above, v_below,
    v_above), the quotients themselves (hq [nrows][n_px][c], vq [n_px][n_px][c]; empty for an axis that is not resampled) and,
    for "rgba", how many colour bytes reached the un-premultiply above their alpha (over_alpha)."""
    if kind == "index":
        idx, palette = pixels
        cols = np.clip(np.asarray(job["hcoef"], np.int64), 0, idx.shape[1] - 1)
        rows = np.clip(np.asarray(job["vcoef"], np.int64), 0, idx.shape[0] - 1)
        return np.ascontiguousarray(np.asarray(palette)[idx[rows][:, cols]].transpose(2, 0, 1))
    px = np.asarray(pixels)
    assert px.dtype == np.uint8 and px.ndim == 3 and px.shape[2] == (3 if kind == "rgb" else 4)
    if kind == "rgba":
        resampled = bool(job["need_h"] or job["need_v"])
        x = two_passes(M.premultiply(px) if resampled else px, job, n_px, stats)
        if stats is not None:
            a = x[..., 3:].astype(np.int64)
            stats["over_alpha"] = int(((x[..., :3] > a) & (a != 0) & (a != 255)).sum()) if resampled else 0
        x = M.unpremultiply(x) if resampled else x[..., :3]
    else:
        x = two_passes(px, job, n_px, stats)
        if kind == "cmyk":
            x = jpeg_cmyk.cmyk2rgb(x)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def window_in_bounds(plan, w, h, n_px):
    """every first tap + count of a resize_plan inside the image, and r0 / nrows exactly the rows its window reads -> None or what is off"""
    ht, vt = tables_of(plan, n_px)
    if ht is not None and not (ht[0].min() >= 0 and (ht[1] >= 1).all() and (ht[0] + ht[1]).max() <= w):
        return "a horizontal tap outside the image"
    if ht is None and not (0 <= plan["left"] and plan["left"] + n_px <= w):
        return "the crop's columns outside the image"
    lo, hi = (int(vt[0].min()), int((vt[0] + vt[1]).max())) if vt is not None else (plan["top"], plan["top"] + n_px)
    if vt is not None and not (vt[1] >= 1).all():
        return "a vertical tap count below 1"
    if not (0 <= lo and hi <= h):
        return "a vertical tap outside the image"
    if (plan["r0"], plan["nrows"]) != (lo, hi - lo):
        return f"r0 / nrows {plan['r0']} / {plan['nrows']} where the window reads rows [{lo}, {hi})"
    return None


# ---- hand-made jobs on the C entries --------------------------------------------------------------------------------------------
def pack_raw_jobs(jobs, n_px, px, out_index=None, tmp_order=None, src_lead=0, pad_h=0, pad_v=0, poison=POISON, slack=1 << 16):
    """Hand-made jobs -> (resize.JOB records, coefficient int32 array, pixel buffer uint8, scratch bytes, max_rows).
    jobs: dicts with "pixels" uint8 [h][w][px] and r0, nrows, left, top, need_h, need_v, "h" / "v" = (first, count, kk) tables.
    The pictures lie back to back behind src_lead bytes, so job i + 1's pixels follow job i's last byte directly and a read past
    an image's end changes a result instead of leaving the buffer; `slack` zero bytes behind the last one keep a kernel that is
    wrong in that way inside the allocation. tmp_order: the order in which the jobs' scratch rows are laid out (a permutation);
    out_index: the output block of each job. pad_h / pad_v widen every coefficient row by that many entries, and every entry
    behind a job's tap count, inside the tables' own width too, becomes `poison`."""
    from clipmi.resize import JOB
    n = len(jobs)
    recs = np.zeros(n, JOB)
    out_index = list(range(n)) if out_index is None else list(out_index)
    tmp_order = list(range(n)) if tmp_order is None else list(tmp_order)
    assert sorted(tmp_order) == list(range(n)) and len(set(out_index)) == n
    toff, tmp_off = 0, {}
    for i in tmp_order:
        tmp_off[i] = toff
        toff += jobs[i]["nrows"] * n_px * px
    coefs, coff, soff, pieces = [], 0, src_lead, [np.zeros(src_lead, np.uint8)]
    for i, j in enumerate(jobs):
        pix = np.ascontiguousarray(j["pixels"])
        h, w = pix.shape[:2]
        assert pix.dtype == np.uint8 and pix.shape[2] == px
        r = recs[i]
        r["src_off"], r["w"], r["h"], r["r0"], r["nrows"], r["out_index"] = soff, w, h, j["r0"], j["nrows"], out_index[i]
        r["need_h"], r["need_v"], r["left"], r["top"], r["tmp_off"] = j["need_h"], j["need_v"], j["left"], j["top"], tmp_off[i]
        for need, key, pad, off, kf in (("need_h", "h", pad_h, "hcoef_off", "hk"), ("need_v", "v", pad_v, "vcoef_off", "vk")):
            r[off] = coff
            if not j[need]:
                continue
            first, count, kk = (np.asarray(t, np.int64) for t in j[key])
            assert first.shape == count.shape == (n_px,) and kk.shape[0] == n_px
            wide = np.full((n_px, kk.shape[1] + pad), poison, np.int64)
            wide[:, :kk.shape[1]] = kk
            wide[np.arange(wide.shape[1])[None, :] >= count[:, None]] = poison
            r[kf] = wide.shape[1]
            coefs.append(block(first, count, wide))
            coff += coefs[-1].size
        pieces.append(pix.reshape(-1))
        soff += pix.size
    pieces.append(np.zeros(slack, np.uint8))
    coef = np.concatenate(coefs) if coefs else np.zeros(1, np.int32)
    return recs, coef, np.concatenate(pieces), max(toff, 1), max(int(j["nrows"]) for j in jobs)


def pack_nearest_jobs(jobs, n_px, out_index=None):
    """Hand-made nearest jobs -> (resize.NEAREST_JOB records, the tables' bytes, the index buffer). jobs: dicts with "pixels" =
    (indices uint8 [h][w], palette uint8 [256][3]) and "hcoef" / "vcoef" int [n_px]. The tables' buffer holds, per job, the palette
    (768 bytes) and the two int32 tables; the offsets of the latter count int32 words, as the kernel reads them."""
    from clipmi.resize import NEAREST_JOB
    recs = np.zeros(len(jobs), NEAREST_JOB)
    tabs, toff, pieces, soff = [], 0, [], 0
    for i, j in enumerate(jobs):
        idx, pal = j["pixels"]
        r = recs[i]
        r["src_off"], r["w"], r["h"], r["out_index"] = soff, idx.shape[1], idx.shape[0], i if out_index is None else out_index[i]
        r["pal_off"], r["col_off"], r["row_off"] = toff, (toff + 768) // 4, (toff + 768) // 4 + n_px
        tabs += [np.ascontiguousarray(pal, np.uint8).reshape(-1), np.asarray(j["hcoef"], np.int32).view(np.uint8), np.asarray(j["vcoef"], np.int32).view(np.uint8)]
        assert tabs[-3].size == 768
        toff += 768 + 8 * n_px
        pieces.append(np.ascontiguousarray(idx, np.uint8).reshape(-1))
        soff += idx.size
    return recs, np.concatenate(tabs), np.concatenate(pieces)


def launch(clipmi, entry, packed, n_px, out, device):
    """Call clipmi_resize_crop_rgb8 / _rgba8 / _cmyk8 (packed: pack_raw_jobs' five) or clipmi_nearest_crop_p8 (pack_nearest_jobs'
    three) directly, as resize.resize_crop_device does, on torch's current stream. out: a flat uint8 device tensor."""
    import torch
    lib, L = clipmi._lib, clipmi._lib.lib()
    recs = torch.from_numpy(packed[0].view(np.uint8).reshape(-1).copy()).to(device)
    tabs, raw = (torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(device) for a in packed[1:3])
    if entry == "clipmi_nearest_crop_p8":
        rc = L.clipmi_nearest_crop_p8(raw.data_ptr(), recs.data_ptr(), len(packed[0]), tabs.data_ptr(), n_px, out.data_ptr(), lib.stream_ptr(device))
    else:
        scratch = torch.empty(packed[3], dtype=torch.uint8, device=device)
        rc = getattr(L, entry)(raw.data_ptr(), recs.data_ptr(), len(packed[0]), packed[4], tabs.data_ptr(), n_px, out.data_ptr(),
                               scratch.data_ptr(), lib.stream_ptr(device))
    lib.check(rc, entry)
    torch.cuda.synchronize(device)


# ---- hard-edged pictures: nothing but 0, 255 (and 245), so that the negative lobes of the bicubic kernel carry sums out of 0..255
def checker(h, w, ch=3):
    """a 1-pixel checkerboard"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], ch, axis=2)


def blocks(rng, h, w, ch=3, size=None):
    """random 0 / 255 blocks of one random size 2..9 (or `size`), each channel its own"""
    b = int(rng.integers(2, 10)) if size is None else size
    a = (rng.integers(0, 2, (-(-h // b), -(-w // b), ch)) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(a, b, axis=0), b, axis=1)[:h, :w])


def text(rng, h, w, ch=3):
    """text-like: black runs of 1..5 pixels on a background of 245"""
    a = np.full((h, w, ch), 245, np.uint8)
    for y0 in range(1, h, 5):
        x = int(rng.integers(0, 4))
        while x < w:
            n = int(rng.integers(1, 6))
            a[y0:y0 + 3, x:x + n] = 0
            x += n + int(rng.integers(1, 6))
    return a


PRIMARIES = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (255, 255, 255), (0, 0, 0)], np.uint8)


def primaries(rng, h, w, stripe=None):
    """saturated primaries side by side in stripes of 3..8 columns, the order turned round every 11 rows"""
    s = int(rng.integers(3, 9)) if stripe is None else stripe
    yy, xx = np.mgrid[0:h, 0:w]
    return PRIMARIES[(xx // s + 3 * (yy // 11)) % len(PRIMARIES)]


def hard_plane(rng, h, w, size=None):
    """an alpha or K plane that is hard-edged itself: 0 / 255 blocks, both values present"""
    a = blocks(rng, h, w, 1, size)[..., 0]
    a[0, 0], a[-1, -1] = 0, 255
    return a


def lobes(h, w, n_px):
    """for a picture reduced to n_px with hundreds of taps an output: 0 / 255 rectangles laid under the kernel's lobes. With s the
    scale of an axis, output o weighs [(o - .5) s, (o + 1.5) s) positively and a further s on either side negatively; rectangles
    of 2 s starting at s / 2 put the whole positive lobe of every odd output on one value and its negative lobes on the other."""
    plan = dw.resize_plan(w, h, n_px)
    sx, sy = w / plan["nw"], h / plan["nh"]
    yy, xx = np.mgrid[0:h, 0:w]
    bx, by = np.floor((xx - 0.5 * sx) / (2 * sx)).astype(np.int64), np.floor((yy - 0.5 * sy) / (2 * sy)).astype(np.int64)
    return np.repeat((((bx + by) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


def hard(rng, h, w, k, ch=3):
    """the generators in turn"""
    if k % 4 == 0:
        return checker(h, w, ch)
    if k % 4 == 1:
        return blocks(rng, h, w, ch)
    if k % 4 == 2:
        return text(rng, h, w, ch)
    return primaries(rng, h, w) if ch == 3 else blocks(rng, h, w, ch, 3)


# ---- the saturating corpus: files of every format the file-level transform entries take, with the pixels a CPU restatement of
# the decoder gives for each. The contents are hard-edged; the JPEG qualities are high enough for the edges to survive.
class File:
    """name; path ("jpeg", "layouts", "cmyk", "png", "interlaced": which call of the GPU test takes it); blob; kind ("rgb", "rgba",
    "cmyk": what the transform resamples); pixels(): the decoded picture in that kind, from a CPU restatement"""
    __slots__ = ("name", "path", "blob", "kind", "pixels")

    def __init__(self, name, path, blob, kind, pixels):
        self.name, self.path, self.blob, self.kind, self.pixels = name, path, blob, kind, pixels


def _jpeg(name, a, **kw):
    from oracle import jpeg_oracle
    blob = jpeg_layouts.encode(a, **dict(dict(quality=95), **kw))
    if kw.get("progressive"):
        import jpeg_progressive
        return File(name, "jpeg", blob, "rgb", lambda: jpeg_progressive.decode(blob))
    return File(name, "jpeg", blob, "rgb", lambda: jpeg_oracle.decode(blob))


def _layout(name, a, layout, H, W, rgb=False, **kw):
    """jpeg_layouts.forge over a given picture: a Pillow file of the source shape relabelled to `layout` (and RGB-coded)"""
    sub = jpeg_layouts.source_shape(layout, H, W)[1] if layout in jpeg_layouts.FACTORS else {"1x1": 0, "2x1": 1, "2x2": 2}[layout]
    src = jpeg_layouts.encode(a, subsampling=sub, **dict(dict(quality=95), **kw))
    out = src
    if layout in jpeg_layouts.FACTORS:
        hs, vs = jpeg_layouts.FACTORS[layout]
        out = jpeg_layouts.relabel(src, luma=hs << 4 | vs, width=W, height=H)
    if rgb:
        out = jpeg_layouts.rgb_coded(out)
    return File(name, "layouts", out, "rgb", lambda: jpeg_layouts.restate_baseline(src, layout, H, W, rgb))


def _cmyk(name, a4, ycck, **kw):
    """jpeg_cmyk's restatement: the sample planes are the inverted pixels of the file's CMYK form (Pillow's decode of it: there is
    no four-component Huffman decoder on the CPU side), planes_to_cmyk gives both forms' mode-CMYK bytes"""
    stored = jpeg_cmyk.cmyk_file(a4, **dict(dict(quality=95, subsampling=0), **kw))
    blob = jpeg_cmyk.as_ycck(stored) if ycck else stored

    def pixels():
        planes = (255 - jpeg_cmyk.pillow4(stored).astype(np.int32)).transpose(2, 0, 1)
        return jpeg_cmyk.planes_to_cmyk(planes, jpeg_cmyk.YCCK if ycck else jpeg_cmyk.CMYK)
    return File(name, "cmyk", blob, "cmyk", pixels)


def _png(name, samples, ctype, lace=False):
    """filters None, Sub and Up only: the CPU restatement undoes the others a pixel at a time"""
    from clipmi import png_parse
    if lace:
        import png_interlace_cases as I
        blob = I.write(samples, ctype, 8, level=6)
        p = png_parse.parse(blob, modes=True, interlaced=True)
        return File(name, "interlaced", blob, "rgba", lambda: I.cpu_decode(p))
    h = samples.shape[0]
    if ctype in (0, 2):
        blob = png_cases.assemble(samples.shape[1], h, samples.shape[2], png_cases.deflate(png_cases.filter_rows(samples, [k % 3 for k in range(h)])))
        return File(name, "png", blob, "rgb", lambda: png_cases.cpu_decode(png_parse.parse(blob)))
    raw = png_cases.filter_rows(samples, [k % 3 for k in range(h)])
    blob = png_cases.assemble(samples.shape[1], h, samples.shape[2], png_cases.deflate(raw), depth=8, ctype=ctype)
    return File(name, "png", blob, "rgba", lambda: M.cpu_decode(png_parse.parse(blob, modes=True)))


N_PX = 224                  # the corpus resamples both axes at this size: no side of a file is 224
WIDE = (560, 600)           # more than JF_SPAN = 512 source columns under the window: the fused kernel walks two chunks
BIG_N_PX = 8
BIG = (1100, 1200)          # at n_px 8: 553 and 603 taps an output, more than a chunk stages - the tap-by-tap path


@functools.lru_cache(maxsize=None)
def corpus():
    """[File] for n_px = N_PX, sides 40..330 and one WIDE file"""
    rng = np.random.default_rng(2026)
    c4 = lambda h, w, k: np.concatenate([hard(rng, h, w, k), hard_plane(rng, h, w)[..., None]], axis=2)        # noqa: E731
    files = [
        _jpeg("baseline 4:4:4 250x330", hard(rng, 250, 330, 1), subsampling=0),
        _jpeg("baseline 4:2:2 330x260", hard(rng, 330, 260, 2), subsampling=1),
        _jpeg("baseline 4:2:0 120x90", blocks(rng, 120, 90, 3, 4)[..., :1].repeat(3, axis=2), subsampling=2),
        _jpeg("baseline grey 300x260", text(rng, 300, 260, 1)[..., 0]),
        _jpeg("progressive 4:2:0 260x300", blocks(rng, 260, 300, 1, 5).repeat(3, axis=2), subsampling=2, progressive=True),
        _jpeg("progressive 4:4:4 40x57", hard(rng, 40, 57, 3), subsampling=0, progressive=True),
        _jpeg("baseline 4:2:0 %dx%d" % WIDE, blocks(rng, *WIDE, 1, 7).repeat(3, axis=2), subsampling=2),
        _layout("1x2 100x75", blocks(rng, 75, 100, 1, 4).repeat(3, axis=2), "1x2", 100, 75),
        _layout("4x1 64x130", blocks(rng, 128, 65, 1, 4).repeat(3, axis=2), "4x1", 64, 130),
        _layout("1x4 130x64", blocks(rng, 65, 128, 1, 4).repeat(3, axis=2), "1x4", 130, 64),
        _layout("RGB-coded 1x1 90x140", hard(rng, 90, 140, 3), "1x1", 90, 140, rgb=True),
        _layout("RGB-coded 1x2 100x75", hard(rng, 75, 100, 1), "1x2", 100, 75, rgb=True),
        _cmyk("CMYK 150x110", c4(150, 110, 1), False),
        _cmyk("YCCK 110x150", c4(110, 150, 2), True),
        _cmyk("CMYK 4:2:0 300x250", c4(300, 250, 3), False, subsampling=2),
        _png("png RGB 230x300", hard(rng, 230, 300, 3), 2),
        _png("png grey 300x240", hard(rng, 300, 240, 2, 1), 0),
        _png("png RGBA 250x330", c4(250, 330, 1), 6),
        _png("png RGBA 60x47", c4(60, 47, 3), 6),
        _png("png LA 310x250", np.concatenate([text(rng, 310, 250, 1), hard_plane(rng, 310, 250)[..., None]], axis=2), 4),
        _png("png interlaced RGBA 200x270", c4(200, 270, 2), 6, lace=True),
    ]
    assert all(N_PX not in _size(f) for f in files)
    return files


@functools.lru_cache(maxsize=None)
def big_corpus():
    """[File] for n_px = BIG_N_PX: one baseline and one progressive file whose outputs have more taps than a chunk of the fused kernel"""
    a = lobes(*BIG, BIG_N_PX)
    return [_jpeg("baseline 4:2:0 %dx%d" % BIG, a, subsampling=2), _jpeg("progressive 4:4:4 %dx%d" % BIG, a, subsampling=0, progressive=True)]


def _size(f):
    from PIL import Image
    return Image.open(io.BytesIO(f.blob)).size


def file_ref(f, n_px, stats=None):
    """transform_ref of a corpus file over its CPU-decoded pixels and decode_worker.resize_plan"""
    px = f.pixels()
    assert px is not None, f.name
    return transform_ref(px, dw.resize_plan(px.shape[1], px.shape[0], n_px), n_px, f.kind, stats)


def load_uint8_blob(blob, n_px):
    return dw.load_uint8(io.BytesIO(blob), n_px)
