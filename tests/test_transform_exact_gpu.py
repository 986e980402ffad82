"""csrc/resize.hip through its four C entries on hand-made jobs whose right answer is known (tests/transform_cases.py:
transform_ref, an int64 numpy restatement of Pillow's rule that shares nothing with the kernels). Bit-exact, no tolerances.

What the jobs state as conditions, none of which a picture resized with resize_plan's tables pins down:
  clip boundaries   sums of each pass exactly on k 2^22 - 1 and k 2^22 for the quotients -2 .. 1 and 254 .. 257, another one in each
                    channel of the same pixel, the fourth channel of the RGBA and CMYK bodies included
  tap counts        every count 1 .. hk and 1 .. vk with hk, vk even and odd, sums that clip in both directions at every count in
                    every channel, and a poison coefficient behind each count. (A count of 0 is not run: resize_plan never emits it
                    and Pillow's rule does not define it apart from "the rounding constant alone".)
  source edges      taps that end on the image's last column and on the last needed row, the next job's pixels directly behind
  batch structure   five jobs of 1, n_px, n_px, 9 and 40 + n_px rows in one launch, the output blocks permuted, the scratch rows not in
                    job order, odd source offsets, all four (need_h, need_v) side by side, a spare output block and guard bands
  pixel functions   CMYK -> RGB, premultiply -> un-premultiply and the un-premultiply alone over every pair of bytes
A job never reads outside its buffers: transform_ref asserts every tap, row and column inside the job's picture before anything
is launched, and pack_raw_jobs lays a zeroed margin behind the last picture for a kernel that is wrong.

The vertical pass behind the fused JPEG entries (clipmi_jpeg_decode_transform_rgb8 and its progressive form) is
launch_resize_v_rgb8, the resize_v_kernel that clipmi_resize_crop_rgb8 launches here: it needs no case of its own."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image

import jpeg_cmyk
import png_mode_cases as M
import transform_cases as T
import ws_cases

pytestmark = pytest.mark.gpu

ENTRY = {"rgb": "clipmi_resize_crop_rgb8", "rgba": "clipmi_resize_crop_rgba8", "cmyk": "clipmi_resize_crop_cmyk8"}
KINDS = ["rgb", "rgba", "cmyk"]
ONE, HALF = T.ONE, T.HALF


def px_of(kind):
    return 3 if kind == "rgb" else 4


def run(clipmi, gpu, kind, jobs, n_px, out_index=None, spare=0, **pack):
    """The jobs through the kind's entry in one launch -> [(reference, device block)] per job. The references come first: they
    assert that no job reads outside its picture. The output has `spare` blocks no job writes, is prefilled with 0xFF and lies
    between guard bands; all of that has to survive."""
    n = len(jobs)
    out_index = list(range(n)) if out_index is None else list(out_index)
    nblocks = n + spare
    assert sorted(out_index) == sorted(set(out_index)) and max(out_index) < nblocks
    if kind == "index":
        refs = [T.transform_ref(j["pixels"], j, n_px, "index") for j in jobs]
        packed = T.pack_nearest_jobs(jobs, n_px, out_index)
    else:
        refs = [T.transform_ref(j["pixels"], j, n_px, kind) for j in jobs]
        packed = T.pack_raw_jobs(jobs, n_px, px_of(kind), out_index=out_index, **pack)
    block = 3 * n_px * n_px
    out = ws_cases.guarded(nblocks * block, ws_cases.ALL_FF, gpu)
    T.launch(clipmi, "clipmi_nearest_crop_p8" if kind == "index" else ENTRY[kind], packed, n_px, out.interior, gpu)
    front, behind, inner = (ws_cases._host(a) for a in out.snapshot())
    assert (front == ws_cases.GUARD_BYTE).all() and (behind == ws_cases.GUARD_BYTE).all(), "the call wrote outside its output"
    blocks = inner.reshape(nblocks, 3, n_px, n_px)
    for b in sorted(set(range(nblocks)) - set(out_index)):
        assert (blocks[b] == 0xFF).all(), f"output block {b} belongs to no job and was written"
    return [(r, blocks[o]) for r, o in zip(refs, out_index)]


def assert_same(pairs, what=""):
    for k, (ref, got) in enumerate(pairs):
        if not np.array_equal(ref, got):
            c, y, x = (int(v[0]) for v in np.nonzero(ref != got))
            raise AssertionError(f"{what} job {k}: {int((ref != got).sum())} of {ref.size} bytes differ, the first at channel {c} row {y} "
                                 f"column {x}: {int(got[c, y, x])} where the reference has {int(ref[c, y, x])}")


EVERY = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), -1)          # [a][b] = (a, b)


def raw_for(premultiplied, alpha):
    """the smallest byte that premultiplies to the wanted value under the given alpha (value <= alpha), elementwise"""
    table = M.premultiply(np.stack([EVERY[..., 0]] * 3 + [EVERY[..., 1]], axis=-1).astype(np.uint8))[..., 0]      # [raw][alpha]
    lowest = np.full((256, 256), -1, np.int64)                 # [alpha][value]
    for raw in range(255, -1, -1):
        lowest[np.arange(256), table[raw]] = raw
    out = lowest[alpha, premultiplied]
    assert (out >= 0).all()
    return out.astype(np.uint8)


# ---- clip boundaries ------------------------------------------------------------------------------------------------------------
def boundary_axis(n):
    """Tables of an axis of n outputs, three taps each at source 3 o, 3 o + 1, 3 o + 2 with the coefficients (c0, 2^22, 1): with
    the pixels (1, p1, p2) under them the sum is 2^21 + c0 + p1 2^22 + p2. c0 = (base - 1/2) 2^22 - 1 makes that
    (base + p1) 2^22 - 1 + p2: exactly one below the boundary of quotient base + p1 for p2 = 0, exactly on it for p2 = 1. Even
    outputs take base = -2, odd ones base = 254, so p1 = 0 .. 3 reaches the quotients -2 .. 1 and 254 .. 257."""
    base = np.where(np.arange(n) % 2 == 0, -2, 254).astype(np.int64)
    kk = np.stack([base * ONE - HALF - 1, np.full(n, ONE), np.ones(n, np.int64)], axis=1)
    return (3 * np.arange(n), np.full(n, 3), kk)


def boundary_pixels(kind, n, m):
    """[3 n][m][px] (the taps along axis 0; transposed by the caller for the horizontal pass): per output o and position t the
    three taps' bytes. Every channel of a pixel takes another (p1, p2): channel c at position t has p1 = (t + c) % 4 and
    p2 = (t // 4 + c) % 2, so eight consecutive positions see all eight in every channel.
    RGBA pictures are premultiplied on load, so there the bytes under the taps are chosen for their premultiplied value, and the
    alpha channel's own (p1, p2) = (a1, a2) goes with the output: a1 = (o // 2) % 4, a2 = (o // 8) % 2, all eight for each base
    within 32 outputs. Tap 0 is (255, 255, 255, alpha 1) = 1 1 1 1 premultiplied; tap 1 has alpha a1 and the colour bytes that
    premultiply to min(p1, a1); tap 2 has alpha a2 and colours 255 or 0 = min(p2, a2) premultiplied."""
    px = px_of(kind)
    o, t, c = np.meshgrid(np.arange(n), np.arange(m), np.arange(px), indexing="ij")
    p1, p2 = (t + c) % 4, (t // 4 + c) % 2
    a = np.empty((n, 3, m, px), np.uint8)
    if kind != "rgba":
        a[:, 0], a[:, 1], a[:, 2] = 1, p1, p2
        return a.reshape(3 * n, m, px)
    a1, a2 = ((o // 2) % 4)[..., :3], ((o // 8) % 2)[..., :3]
    a[:, 0] = (255, 255, 255, 1)
    a[:, 1, :, :3] = raw_for(np.minimum(p1[..., :3], a1), a1)
    a[:, 1, :, 3] = a1[..., 0]
    a[:, 2, :, :3] = 255 * np.minimum(p2[..., :3], a2)
    a[:, 2, :, 3] = a2[..., 0]
    return a.reshape(3 * n, m, px)


def boundary_jobs(kind, n_px, v_only=False):
    """one job whose horizontal pass lands on the boundaries (the vertical one a crop), one the other way round, and one whose
    horizontal sums pass an identity vertical pass (one tap of 2^22)"""
    tabs = boundary_axis(n_px)
    vert = boundary_pixels(kind, n_px, n_px)
    j_v = dict(pixels=vert, r0=0, nrows=3 * n_px, left=0, top=0, need_h=0, need_v=1, v=tabs)
    if v_only:
        return [j_v]
    horiz = np.ascontiguousarray(boundary_pixels(kind, n_px, n_px + 2).transpose(1, 0, 2))
    j_h = dict(pixels=horiz, r0=1, nrows=n_px, left=0, top=1, need_h=1, need_v=0, h=tabs)
    ident = (np.arange(n_px) + 2, np.ones(n_px, np.int64), np.full((n_px, 1), ONE))
    j_hv = dict(pixels=horiz, r0=2, nrows=n_px, left=0, top=0, need_h=1, need_v=1, h=tabs, v=ident)
    return [j_h, j_v, j_hv]


def quotients_seen(jobs, kind, n_px):
    """per channel, the unclipped quotients of the boundary jobs' three-tap passes, from the reference"""
    seen = [set() for _ in range(px_of(kind))]
    for j in jobs:
        stats = {}
        T.two_passes(M.premultiply(j["pixels"]) if kind == "rgba" else j["pixels"], j, n_px, stats)
        for key, q in (("h", stats["hq"]), ("v", stats["vq"])):
            if key in j and j[key][2].shape[1] == 3:
                for c in range(px_of(kind)):
                    seen[c] |= set(np.unique(q[..., c]).tolist())
    return seen


@pytest.mark.parametrize("n_px", [1, 7, 32])
@pytest.mark.parametrize("kind", KINDS)
def test_sums_on_the_clip_boundaries_in_every_channel(clipmi, gpu, kind, n_px):
    """Sums one below and exactly on the boundary of the quotients -2 .. 1 and 254 .. 257, in the horizontal pass, in the vertical
    pass and in both, a different one in each channel of a pixel. At n_px 32 every channel sees every one of the sixteen
    sums (asserted on the reference's unclipped quotients: -3 .. 1 and 253 .. 257)."""
    jobs = boundary_jobs(kind, n_px)
    if n_px == 32:
        want = set(range(-3, 2)) | set(range(253, 258))
        for c, seen in enumerate(quotients_seen(jobs, kind, n_px)):
            assert want <= seen, (c, sorted(want - seen))
    assert_same(run(clipmi, gpu, kind, jobs, n_px, out_index=[2, 0, 1], spare=1, src_lead=1 if kind == "rgb" else 4), kind)


@pytest.mark.parametrize("kind", KINDS)
def test_the_vertical_pass_on_the_clip_boundaries_at_224(clipmi, gpu, kind):
    """the vertical pass once at the product's size: 224 x 224 outputs over 672 rows, the same sixteen sums"""
    assert_same(run(clipmi, gpu, kind, boundary_jobs(kind, 224, v_only=True), 224), kind)


# ---- tap counts -----------------------------------------------------------------------------------------------------------------
def counted_axis(rng, n, K, shift, size, sign):
    """n outputs over an axis of `size`: count (o + shift) % K + 1, so K jobs of shift 0 .. K - 1 give every output every count;
    the first output starts at 0, the last one ends on the axis's last sample, the others lie between. The coefficients of a
    job's axis are mostly of one sign, the caller's, and sized so that no sum can leave int32 whatever the
    pixels: the sums leave 0 .. 255 on both sides."""
    count = (np.arange(n) + shift) % K + 1
    first = np.minimum(np.arange(n) * max(size - K, 0) // max(n - 1, 1), size - count)
    first[0] = 0
    first[-1] = size - count[-1]
    kk = np.zeros((n, K), np.int64)
    for o in range(n):
        c = int(count[o])
        other = int(rng.integers(0, c)) if c > 1 else -1       # one tap of the other sign among two or more
        hi = ((1 << 31) - HALF - 1) // (255 * (c - (c > 1)))    # (each sign's taps alone stay inside int32 under pixels of 255)
        kk[o, :c] = sign * rng.integers(6 * hi // 10, hi + 1, c)
        if c > 1:
            kk[o, other] = -sign * int(rng.integers(0, hi // 8))
    return first, count, kk


def counted_jobs(rng, kind, n_px):
    """14 jobs: hk = 6 with vk = 7 at seven shifts of the counts (every count of both axes at every output, at n_px 1 too), then
    hk = 7 with vk = 6"""
    jobs = []
    for K in (6, 7):
        for shift in range(7):
            w, h = n_px + K + 2, n_px + (13 - K) + 4
            col = T.blocks(rng, h, w, 3, 3 + shift % 4)
            pix = col if kind == "rgb" else np.concatenate([col, T.hard_plane(rng, h, w, 3)[..., None]], axis=2)
            # (the signs of the two axes go through all four pairs with the shift: a vertical sum above 255 needs rows that are not 0)
            sh, sv = 1 - 2 * ((shift + K) % 2), 1 - 2 * ((shift + K) // 2 % 2)
            ht, vt = counted_axis(rng, n_px, K, shift, w, sh), counted_axis(rng, n_px, 13 - K, shift, h - 1, sv)
            vt = (vt[0] + 1, vt[1], vt[2])                       # (rows 1 .. h - 1: r0 = 1, and the last needed row is the picture's last)
            r0 = int(vt[0].min())
            jobs.append(dict(pixels=pix, r0=r0, nrows=int((vt[0] + vt[1]).max()) - r0, left=0, top=0, need_h=1, need_v=1, h=ht, v=vt))
    return jobs


def clip_hits(jobs, kind, n_px):
    """{(pass, coefficient row width, tap count, channel, side)} for which the reference's unclipped quotient leaves 0 .. 255"""
    hits = set()
    for j in jobs:
        stats = {}
        T.two_passes(M.premultiply(j["pixels"]) if kind == "rgba" else j["pixels"], j, n_px, stats)
        for name, q, count in (("h", stats["hq"].transpose(1, 0, 2), j["h"][1]), ("v", stats["vq"], j["v"][1])):
            K = j[name][2].shape[1]
            for o, c in enumerate(count):
                for ch in range(px_of(kind)):
                    if (q[o, :, ch] < 0).any():
                        hits.add((name, K, int(c), ch, "below"))
                    if (q[o, :, ch] > 255).any():
                        hits.add((name, K, int(c), ch, "above"))
    return hits


@pytest.mark.parametrize("n_px", [1, 7, 32])
@pytest.mark.parametrize("kind", KINDS)
def test_every_tap_count_with_poison_behind_it(clipmi, gpu, kind, n_px):
    """Every tap count 1 .. 6 and 1 .. 7 in both passes, in rows of coefficients 6 and 7 wide and, padded, 7, 8 and 9 wide, 2^30 in every
    entry behind a count: a kernel that reads hk taps instead of `count`, or takes the parity of hk for that of the count, differs.
    At n_px 32 each count clips below 0 and above 255 in every channel of both passes at either width; that is asserted on the
    reference (n_px 1 and 7 have too few outputs for every combination, and run the same jobs for the launch geometry)."""
    rng = np.random.default_rng(3)
    jobs = counted_jobs(rng, kind, n_px)
    assert {int(c) for j in jobs for c in j["h"][1]} == set(range(1, 8)) and {int(c) for j in jobs for c in j["v"][1]} == set(range(1, 8))
    if n_px == 32:
        want = {(name, K, c, ch, side) for name in "hv" for K in (6, 7) for c in range(1, K + 1) for ch in range(px_of(kind))
                for side in ("below", "above")}
        hits = clip_hits(jobs, kind, n_px)
        assert want <= hits, sorted(want - hits)[:8]
    assert_same(run(clipmi, gpu, kind, jobs, n_px, src_lead=3 if kind == "rgb" else 8), f"{kind} unpadded")
    assert_same(run(clipmi, gpu, kind, jobs, n_px, pad_h=1, pad_v=2, src_lead=5 if kind == "rgb" else 4), f"{kind} padded")


# ---- batch structure --------------------------------------------------------------------------------------------------------------
def spread_axis(rng, n, rows, first0, blur=3):
    """n outputs whose taps span exactly `rows` samples from first0 on: `blur` taps each (all `rows` of them for one output),
    coefficients around a third each with a negative one among them"""
    cnt = min(blur, rows) if n > 1 else rows
    first = first0 + np.arange(n) * (rows - cnt) // max(n - 1, 1)
    kk = rng.integers(ONE // (2 * cnt), 2 * ONE // cnt, (n, cnt))
    kk[:, 0] = -kk[:, 0] // 2
    return first, np.full(n, cnt), kk


def batch_jobs(rng, kind, n_px):
    """Five jobs of 1, n_px, n_px, 9 and 40 + n_px needed rows; (need_h, need_v) = (1,1), (0,0), (1,0), (0,1), (1,1). Even widths, so
    that with an odd lead every 3-byte picture starts at an odd offset."""
    def pic(h, w, k):
        col = T.hard(rng, h, w, k)
        return col if kind == "rgb" else np.concatenate([col, T.hard_plane(rng, h, w)[..., None]], axis=2)

    w = n_px + 6 + n_px % 2
    jobs = [dict(pixels=pic(5, w, 1), left=0, top=0, need_h=1, need_v=1, h=spread_axis(rng, n_px, w, 0), v=(np.full(n_px, 3), np.ones(n_px, np.int64), rng.integers(ONE // 2, 3 * ONE // 2, (n_px, 1)))),
            dict(pixels=pic(n_px + 3, w, 2), left=w - n_px, top=3, need_h=0, need_v=0),
            dict(pixels=pic(n_px + 2, w, 3), left=0, top=1, need_h=1, need_v=0, h=spread_axis(rng, n_px, w - 1, 1)),
            dict(pixels=pic(12, w, 0), left=3, top=0, need_h=0, need_v=1, v=spread_axis(rng, n_px, 9, 2)),
            dict(pixels=pic(40 + n_px, w, 1), left=0, top=0, need_h=1, need_v=1, h=spread_axis(rng, n_px, w, 0, 5), v=spread_axis(rng, n_px, 40 + n_px, 0, 4))]
    for j in jobs:
        if j["need_v"]:
            j["r0"] = int(j["v"][0].min())
            j["nrows"] = int((j["v"][0] + j["v"][1]).max()) - j["r0"]
        else:
            j["r0"], j["nrows"] = j["top"], n_px
    assert [j["nrows"] for j in jobs] == [1, n_px, n_px, 9, 40 + n_px]
    return jobs


@pytest.mark.parametrize("n_px", [1, 7, 32])
@pytest.mark.parametrize("kind", KINDS)
def test_a_batch_of_unlike_jobs(clipmi, gpu, kind, n_px):
    """One launch: max_rows comes from the largest job, so the workgroups of the others mostly fall behind their rows, and at
    n_px 7 and 32 a workgroup of 256 threads straddles rows. The output blocks are a permutation with block 2 of six left out, the
    scratch rows lie in another order than the jobs, the pictures lie back to back from an odd offset (3-byte entry; a multiple of
    4 for the 4-byte entries), the crop of job 1 ends on its picture's last column and last row."""
    jobs = batch_jobs(np.random.default_rng(4), kind, n_px)
    pairs = run(clipmi, gpu, kind, jobs, n_px, out_index=[3, 0, 5, 1, 4], spare=1, tmp_order=[2, 4, 0, 3, 1], src_lead=1 if kind == "rgb" else 4)
    assert_same(pairs, kind)


# ---- the pixel functions, exhaustively ----------------------------------------------------------------------------------------------


def crop256(pix):
    return dict(pixels=pix, r0=0, nrows=256, left=0, top=0, need_h=0, need_v=0)


def test_cmyk_to_rgb_over_every_c_and_k(clipmi, gpu):
    """a 256 x 256 picture of (c, c, 255 - c, K) for every (c, K), cropped only: jpeg_cmyk.cmyk2rgb, and Pillow's own convert("RGB")"""
    c, k = EVERY[..., 0], EVERY[..., 1]
    pix = np.stack([c, c, 255 - c, k], axis=-1).astype(np.uint8)
    (ref, got), = run(clipmi, gpu, "cmyk", [crop256(pix)], 256)
    assert np.array_equal(ref, jpeg_cmyk.cmyk2rgb(pix).transpose(2, 0, 1))
    assert np.array_equal(ref, np.asarray(Image.fromarray(pix, "CMYK").convert("RGB")).transpose(2, 0, 1))
    assert_same([(ref, got)])


def over_alpha_picture():
    """[512][256][4]: rows 2 y and 2 y + 1 under the taps (2 x 2^22, -2^22) of output row y, so the resampled byte is 2 p1 - p2 of
    the premultiplied bytes. Output (y, x) is to reach the un-premultiply with alpha y and the colours x, 255 - x, (x + 128) % 256:
    alpha a2 = 255 or 254 (the parity of y) and a1 = (y + a2) / 2 give 2 a1 - a2 = y; a colour C takes p1 = ceil(C / 2) <= a1 and
    p2 = 2 p1 - C. Only C = 255 under alpha 0 is out of reach (2 a1 <= a2 bounds C by 254 there); it arrives as 254."""
    y, x = EVERY[..., 0], EVERY[..., 1]
    a2 = np.where(y % 2 == 1, 255, 254)
    a1 = (y + a2) // 2
    pic = np.empty((256, 2, 256, 4), np.uint8)
    for ch, C in enumerate((x, 255 - x, (x + 128) % 256)):
        p1 = np.minimum((C + 1) // 2, a1)
        p2 = np.maximum(2 * p1 - C, 0)
        pic[:, 0, :, ch], pic[:, 1, :, ch] = raw_for(p1, a1), raw_for(p2, a2)
    pic[:, 0, :, 3], pic[:, 1, :, 3] = a1, a2
    return pic.reshape(512, 256, 4)


def test_rgba_pixel_functions_over_every_colour_and_alpha(clipmi, gpu):
    """Three jobs over every pair of bytes, one launch. (0) every (colour, alpha) through an identity vertical pass, one tap of
    2^22: premultiply, then un-premultiply - png_mode_cases' pair, which its own tests pin against Pillow. (1) the un-premultiply
    alone over every (colour', alpha) that can reach it, colour' > alpha, alpha 0 and alpha 255 included (over_alpha_picture).
    (2) a job that resamples nothing: the colours come back untouched at every alpha."""
    c, a = EVERY[..., 0], EVERY[..., 1]
    pix = np.stack([c, 255 - c, c * 7 % 256, a], axis=-1).astype(np.uint8)
    ident = (np.arange(256), np.ones(256, np.int64), np.full((256, 1), ONE))
    two = (2 * np.arange(256), np.full(256, 2), np.tile(np.array([2 * ONE, -ONE]), (256, 1)))
    jobs = [dict(crop256(pix), need_v=1, v=ident), dict(pixels=over_alpha_picture(), r0=0, nrows=512, left=0, top=0, need_h=0, need_v=1, v=two), crop256(pix)]
    reached = T.two_passes(M.premultiply(jobs[1]["pixels"]), jobs[1], 256)
    pairs = set(map(tuple, reached[..., [0, 3]].reshape(-1, 2).tolist()))
    assert pairs == {(col, al) for col in range(256) for al in range(256)} - {(255, 0)}
    assert int((reached[..., :3] > reached[..., 3:]).sum()) > 90000
    got = run(clipmi, gpu, "rgba", jobs, 256, out_index=[1, 2, 0])
    assert np.array_equal(got[0][0], M.unpremultiply(M.premultiply(pix)).transpose(2, 0, 1))
    assert np.array_equal(got[2][0], pix[..., :3].transpose(2, 0, 1))
    assert_same(got)


# ---- clipmi_nearest_crop_p8 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_px", [1, 7])
def test_nearest_gathers_through_all_palette_entries_and_clamps(clipmi, gpu, n_px):
    """Index pictures that hold all 256 indices under random palettes; tables that point at the first and the last row and column,
    and at -1 and w / h, which the kernel clamps into the picture - the reference (transform_ref "index") clamps in the same way,
    which is the contract here: decode_worker.nearest_plan never emits such a value. The output blocks are permuted."""
    rng = np.random.default_rng(5)
    jobs = []
    for k, (h, w) in enumerate([(19, 23), (16, 16), (300, 1), (1, 300), (37, 41)]):
        idx = ((np.arange(h)[:, None] * w + np.arange(w)[None, :] + 11 * k) % 256).astype(np.uint8)
        edge_c, edge_r = np.array([-1, 0, w - 1, w, w // 2, 1, w - 2]), np.array([0, h - 1, -1, h, 1, h // 2, h - 2])
        cols, rows = np.roll(edge_c, -k)[:n_px], np.roll(edge_r, -2 * k)[:n_px]
        jobs.append(dict(pixels=(idx, rng.integers(0, 256, (256, 3), dtype=np.uint8)), hcoef=cols, vcoef=rows))
    assert all(len(np.unique(j["pixels"][0])) == 256 for j in jobs if j["pixels"][0].size >= 256)
    full = [dict(j, hcoef=np.arange(n_px) % j["pixels"][0].shape[1], vcoef=np.arange(n_px) % j["pixels"][0].shape[0]) for j in jobs[:1]]
    assert_same(run(clipmi, gpu, "index", jobs + full, n_px, out_index=[4, 2, 0, 5, 1, 6], spare=1), "nearest")


def test_nearest_reads_every_palette_entry(clipmi, gpu):
    """a 16 x 16 picture of the indices 0 .. 255 taken whole (n_px 16): every palette entry arrives"""
    idx = np.arange(256, dtype=np.uint8).reshape(16, 16)
    pal = np.random.default_rng(6).integers(0, 256, (256, 3), dtype=np.uint8)
    (ref, got), = run(clipmi, gpu, "index", [dict(pixels=(idx, pal), hcoef=np.arange(16), vcoef=np.arange(16))], 16)
    assert np.array_equal(ref, pal.reshape(16, 16, 3).transpose(2, 0, 1))
    assert_same([(ref, got)])


# ---- refusals: answered from the arguments, nothing is launched ---------------------------------------------------------------------
def test_the_entries_refuse_bad_arguments_and_do_nothing_for_no_jobs(clipmi):
    """null pointers, n_px 0 and 4097, max_rows 0, a negative job count, nearest tables off a 4-byte boundary: an error code and a
    message that names the entry; no jobs: 0, and the output keeps what it held. No pointer is dereferenced on these paths, so the
    output is a host array between guard bands."""
    lib, L = clipmi._lib, clipmi._lib.lib()
    p = C.c_void_p(4096)                                       # never dereferenced: every call below returns from its checks
    out = ws_cases.guarded(3 * 7 * 7, ws_cases.RANDOM)
    before = out.snapshot()
    o = C.c_void_p(out.interior.ctypes.data)
    for name in ENTRY.values():
        f = getattr(L, name)
        ok = [p, p, 1, 1, p, 7, o, p, None]                    # raw, jobs, njobs, max_rows, coef, n_px, out, scratch, stream
        for k in (0, 1, 4, 6, 7):
            bad = list(ok)
            bad[k] = None
            assert f(*bad) != 0 and name[7:] in lib.last_error(), (name, k)
        for k, v in ((5, 0), (5, 4097), (5, -1), (3, 0), (2, -1)):
            bad = list(ok)
            bad[k] = v
            assert f(*bad) != 0 and name[7:] in lib.last_error(), (name, k, v)
        assert f(None, None, 0, 0, None, 0, o, None, None) == 0
        assert f(p, p, 0, 1, p, 7, o, p, None) == 0
    f = L.clipmi_nearest_crop_p8
    ok = [p, p, 1, p, 7, o, None]                              # raw, jobs, njobs, tables, n_px, out, stream
    for k in (0, 1, 3, 5):
        bad = list(ok)
        bad[k] = None
        assert f(*bad) != 0 and "nearest_crop_p8" in lib.last_error(), k
    for k, v in ((4, 0), (4, 4097), (2, -1), (3, C.c_void_p(4097)), (3, C.c_void_p(4098))):
        bad = list(ok)
        bad[k] = v
        assert f(*bad) != 0 and "nearest_crop_p8" in lib.last_error(), (k, v)
    assert f(None, None, 0, None, 0, o, None) == 0
    assert f(p, p, 0, p, 7, o, None) == 0
    assert all(np.array_equal(a, b) for a, b in zip(before, out.snapshot())), "a call without jobs touched its output"
