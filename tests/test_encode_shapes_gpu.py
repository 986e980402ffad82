"""-m gpu: the whole towers at the batch sizes the product runs, and every prompt length.

DESIGN.md §4 promises that each row's bits depend neither on the batch size, the chunk cuts, the lane nor the kernel choice,
and that a prompt's bits do not depend on how far the text tower is trimmed. The other encode tests check that at a few rows
of small batches; here every row of the production shapes is held to it. The reference chain has two links:

1. bitwise: row k of a large call == the same input encoded in a small call of another size (chunks of 7 images, B = 1 for
   the wide geometries, Q = 1 for prompts), f32 bits compared, every row finite;
2. oracle: rows on every boundary of the large call (first / last row, both sides of each chunk and lane cut, the image that
   holds the first token row of the last 256-row M-tile) against oracle/clip_oracle.py under the measured-noise rules of
   test_encode_gpu._tolerances (bf16) and test_fp8_gpu's FP8_* constants.

Pixels are generated on the device as uint8 (the CLI's input); each batch size is fed a shifted slice of one pool, so that an
image lands at different row positions in different calls.
"""
import os
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import clip_case  # noqa: E402
from oracle import clip_oracle  # noqa: E402
from test_encode_gpu import _cos, _tolerances  # noqa: E402
from test_fp8_gpu import FP8_COS_FLOOR, FP8_COS_SLACK_REF, FP8_ERR_FACTOR  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = 1


def _pixels(gpu, n, res, seed):
    g = torch.Generator(device=gpu)
    g.manual_seed(seed)
    return torch.randint(0, 256, (n, 3, res, res), generator=g, dtype=torch.uint8, device=gpu)


def _normalized(clipmi, u8):
    """The transform's float tail (what encode_image fuses for uint8 input), in f32 on the tensor's device."""
    mean = torch.tensor(clipmi.model.CLIP_MEAN, device=u8.device).reshape(1, 3, 1, 1)
    std = torch.tensor(clipmi.model.CLIP_STD, device=u8.device).reshape(1, 3, 1, 1)
    return (u8.float() / 255.0 - mean) / std


def _in_chunks(model, x, step=7, **kw):
    return torch.cat([model.encode_image(x[i:i + step], **kw) for i in range(0, x.shape[0], step)])


def _shift(B, n):
    """Where batch size B starts in a pool of n images: a different offset per B."""
    return (B * 389) % (n - B + 1)


def _boundary_rows(lanes, tokens):
    """First and last row of every kernel sequence (both sides of each cut) and the image that holds the first token row of
    the sequence's last 256-row M-tile."""
    rows = set()
    for lo, hi, _ in lanes:
        n = hi - lo
        rows |= {lo, hi - 1, lo + ((n * tokens - 1) // 256 * 256) // tokens}
    return sorted(rows)


def _assert_same_bits(got, ref, what):
    assert got.shape == ref.shape, what
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    diff = (got.contiguous().view(torch.int32) != ref.contiguous().view(torch.int32)).reshape(got.shape[0], -1).any(dim=1)
    if diff.any():
        rows = diff.nonzero().flatten().tolist()
        raise AssertionError(f"{what}: {len(rows)} of {got.shape[0]} rows differ in bits, first {rows[:10]}")


def _check_oracle(clipmi, sd, fn, x, got, what):
    ref, noise = _tolerances(clipmi, sd, fn, x)
    err = (got - ref).abs().max().item()
    cos = _cos(got, ref).min().item()
    print(f"{what}: oracle err {err:.4g} (bf16-emulation noise {noise:.4g}), min cosine {cos:.6f} over {x.shape[0]} rows")
    assert err <= 3 * noise + 1e-3, f"{what}: err {err} vs measured bf16 noise {noise}"
    assert cos >= 0.9995, what


# ---- 1. ViT-B/32, bf16, the residual stream of real checkpoints, every batch form ------------------------------------------

POOL_B32 = 2000
B32_LANES = {
    1: [(0, 1, 0)], 2: [(0, 2, 0)], 5: [(0, 5, 0)], 6: [(0, 6, 0)],
    434: [(0, 434, 0)], 435: [(0, 435, 0)], 436: [(0, 436, 0)],
    869: [(0, 869, 0)], 870: [(0, 435, 0), (435, 870, 1)], 871: [(0, 871, 0)],
    1023: [(0, 1023, 0)], 1024: [(0, 1024, 0)], 1025: [(0, 870, 0), (870, 1025, 0)],
    1305: [(0, 435, 0), (435, 870, 1), (870, 1305, 0)], 1306: [(0, 870, 0), (870, 1306, 0)],
    1740: [(0, 435, 0), (435, 870, 1), (870, 1305, 0), (1305, 1740, 1)],
    2000: [(0, 870, 0), (870, 1740, 0), (1740, 2000, 0)],
}


@pytest.fixture(scope="module")
def b32(clipmi, gpu):
    sd = clip_case.state_dict("vitb32_realstats")
    model = clipmi.CLIP(sd, device=gpu)
    assert model.dims["v_tokens"] == 50 and model.image_chunk(limit=model.max_batch // 2) == 435
    pool = _pixels(gpu, POOL_B32, 224, seed=20)
    ref = _in_chunks(model, pool)
    refn = _in_chunks(model, pool, normalize=True)
    return dict(sd=sd, model=model, pool=pool, ref=ref, refn=refn)


@pytest.mark.parametrize("B", sorted(B32_LANES))
def test_vitb32_every_row_at_every_batch_size(b32, B):
    """One tile's M-tail, one and two rounds, the two-lane forms (870, 1305, 1740), one sequence up to max_batch and the
    chunked forms above it: every row == the chunk-of-7 encode of the same image, with and without the fused normalisation."""
    model, pool = b32["model"], b32["pool"]
    assert model.image_lanes(B) == B32_LANES[B]
    s = _shift(B, POOL_B32)
    x = pool[s:s + B]
    got = model.encode_image(x)
    _assert_same_bits(got, b32["ref"][s:s + B], f"ViT-B/32 B={B}")
    gotn = model.encode_image(x, normalize=True)
    _assert_same_bits(gotn, b32["refn"][s:s + B], f"ViT-B/32 B={B} normalize=True")
    assert torch.allclose(gotn, got / got.norm(dim=-1, keepdim=True), atol=2e-6)


@pytest.mark.parametrize("B", [870, 1025])
def test_vitb32_f32_input_rows_at_batch_size(clipmi, b32, B):
    """Pre-normalised f32 input through the two-lane (870) and the chunked (1025) form == its own chunk-of-7 encode."""
    model = b32["model"]
    s = _shift(B, POOL_B32)
    x = _normalized(clipmi, b32["pool"][s:s + B])
    _assert_same_bits(model.encode_image(x), _in_chunks(model, x), f"ViT-B/32 f32 B={B}")


def test_vitb32_callers_raw_stream_is_one_lane(clipmi, b32, gpu, monkeypatch):
    """encode_image(out=, stream=) keeps every kernel sequence on the caller's stream (no internal side stream) and gives the
    same bits as the two-lane form at B = 870."""
    model, B = b32["model"], 870
    s = _shift(B, POOL_B32)
    x = b32["pool"][s:s + B]

    def no_side_stream(*a, **k):
        raise AssertionError("a caller's raw stream must not be paired with the internal side stream")

    monkeypatch.setattr(clipmi._lib, "side_stream", no_side_stream)
    out = torch.full((B, model.embed_dim), float("nan"), device=gpu)
    stream = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize(gpu)
    assert model.encode_image(x, out=out, stream=stream.cuda_stream) is out
    stream.synchronize()
    _assert_same_bits(out, b32["ref"][s:s + B], "ViT-B/32 B=870 on a caller's raw stream")


def test_vitb32_boundary_rows_match_oracle(clipmi, b32):
    model, pool = b32["model"], b32["pool"]
    got, idx = [], []
    for B in (870, 1025, 2000):
        s = _shift(B, POOL_B32)
        rows = _boundary_rows(model.image_lanes(B), 50)
        out = model.encode_image(pool[s:s + B])
        for r in rows:
            if s + r not in idx:
                idx.append(s + r)
                got.append(out[r])
    print(f"ViT-B/32 oracle rows: pool images {idx}")
    x = _normalized(clipmi, pool[idx].cpu())
    _check_oracle(clipmi, b32["sd"], clip_oracle.encode_image, x, torch.stack(got).cpu(), "ViT-B/32 realstats B=870/1025/2000")


# ---- 3. the FP8 tower (section 2, the wide geometries, is at the end of the module) ---------------------------------------

POOL_FP8 = 1100


def test_fp8_tower_every_row_at_every_batch_size(clipmi, gpu):
    """vision_weights="fp8": activations are quantised with one scale per row or per 32-value block of a row, so a row's bits
    do not depend on its neighbours either. Every row of B in {1, 6, 435, 870, 1025} == the chunk-of-7 encode; the boundary
    rows of 870 and 1025 against the emulation of the product's quantisers (test_fp8_gpu's rule)."""
    sd = clip_case.state_dict("vitb32_seed0")
    model = clipmi.CLIP(sd, device=gpu, vision_weights="fp8")
    assert model.vision.weight_format == 1
    pool = _pixels(gpu, POOL_FP8, 224, seed=21)
    ref = _in_chunks(model, pool)
    got, idx = [], []
    for B in (1, 6, 435, 870, 1025):
        s = _shift(B, POOL_FP8)
        out = model.encode_image(pool[s:s + B])
        _assert_same_bits(out, ref[s:s + B], f"FP8 ViT-B/32 B={B}")
        if B >= 870:
            for r in _boundary_rows(model.image_lanes(B), 50):
                if s + r not in idx:
                    idx.append(s + r)
                    got.append(out[r])
    got = torch.stack(got).cpu()
    x = _normalized(clipmi, pool[idx].cpu())
    sdr = clipmi.weights.bf16_round_state_dict(sd)
    oref = clip_oracle.encode_image(sdr, x)
    with clip_oracle.act_round(torch.bfloat16), clip_oracle.linear_fp8():
        emu = clip_oracle.encode_image(sdr, x)
    noise = (emu - oref).abs().max().item()
    err = (got - oref).abs().max().item()
    cos, cos_own = _cos(got, oref).min().item(), _cos(emu, oref).min().item()
    print(f"FP8 ViT-B/32 B=870/1025, {len(idx)} boundary rows: err {err:.4g} (emulation noise {noise:.4g}), "
          f"min cosine {cos:.5f} (emulation itself {cos_own:.5f})")
    assert err <= FP8_ERR_FACTOR * noise + 1e-3, f"err {err} vs measured e4m3 noise {noise}"
    assert cos >= max(FP8_COS_FLOOR, cos_own - FP8_COS_SLACK_REF)


# ---- 4. text tower: every prompt length, Q across the chunk cuts -----------------------------------------------------------

def _prompts(d, seed, eots):
    """One prompt per EOT position (EOT = the top id); then one with the top id at two positions (pooled at the first) and
    one whose positions after EOT hold non-zero ids (both built from the EOT 9 / EOT 6 prompts). Returns (ids [P, ctx] int64,
    pooled position per prompt)."""
    ctx, vocab = d["ctx"], d["vocab"]
    assert 6 in eots and 9 in eots
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    rows, pos = [], []
    for eot in eots:
        r = torch.zeros(ctx, dtype=torch.int64)
        r[0] = vocab - 2
        r[1:eot] = torch.randint(1, vocab - 2, (eot - 1,), generator=g)
        r[eot] = vocab - 1
        rows.append(r)
        pos.append(eot)
    r = rows[eots.index(9)].clone()
    r[40] = vocab - 1
    rows.append(r)
    pos.append(9)
    r = rows[eots.index(6)].clone()
    r[7:] = torch.randint(1, vocab - 2, (ctx - 7,), generator=g)
    rows.append(r)
    pos.append(6)
    return torch.stack(rows), pos


def test_text_every_prompt_length_in_every_form(clipmi, gpu):
    """EOT at every position 1 .. 76, a repeated top id, ids after EOT. Each prompt's row is the same bits as Q = 1 with host
    ids (tower trimmed to EOT + 1 positions, skinny GEMM) in: one batch of all prompts (host ids, trimmed to the batch's
    largest EOT + 1), the same with device-resident ids (all 77 positions), batches of prompts of nearby lengths (trimmed to
    each batch's own length), and shuffled batches of Q in {2, 3, 1023, 1024, 1025, 2100} - the last two cross max_batch."""
    sd = clip_case.state_dict("vitb32_seed0")
    model = clipmi.CLIP(sd, device=gpu)
    d = model.dims
    ids, pos = _prompts(d, 31, list(range(1, d["ctx"])))
    P = ids.shape[0]
    assert [int(a) for a in ids.argmax(dim=1)] == pos
    one = torch.cat([model.encode_text(ids[i:i + 1]) for i in range(P)])
    onen = torch.cat([model.encode_text(ids[i:i + 1], normalize=True) for i in range(P)])
    assert torch.isfinite(one).all()
    assert torch.allclose(onen, one / one.norm(dim=-1, keepdim=True), atol=2e-6)
    allh = model.encode_text(ids)
    _assert_same_bits(allh, one, "all prompts, host ids")
    _assert_same_bits(model.encode_text(ids.to(gpu)), one, "all prompts, device ids")
    _assert_same_bits(model.encode_text(ids, normalize=True), onen, "all prompts, host ids, normalize=True")
    order = sorted(range(P), key=lambda i: pos[i])
    for k in range(0, P, 10):                           # batches of nearby lengths: trimmed to 2 .. 77 positions
        grp = order[k:k + 10]
        _assert_same_bits(model.encode_text(ids[grp]), one[grp], f"prompts {grp}, host ids")
    g = torch.Generator(device="cpu")
    g.manual_seed(32)
    for Q in (2, 3, 1023, 1024, 1025, 2100):
        idx = torch.cat([torch.randperm(P, generator=g) for _ in range(-(-Q // P))])[:Q]
        _assert_same_bits(model.encode_text(ids[idx]), one[idx], f"Q={Q}, host ids")
        if Q >= 1024:
            _assert_same_bits(model.encode_text(ids[idx].to(gpu), normalize=True), onen[idx], f"Q={Q}, device ids, normalize=True")
    short = [i for i in range(P) if pos[i] <= 20]      # Q = 1025 on a tower trimmed to 21 positions
    idx = torch.tensor(short)[torch.randint(0, len(short), (1025,), generator=g)]
    _assert_same_bits(model.encode_text(ids[idx]), one[idx], "Q=1025 of prompts with EOT <= 20, host ids")
    sel = [pos.index(e) for e in (1, 2, 3, 8, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 75, 76)] + [P - 2, P - 1]
    _check_oracle(clipmi, sd, clip_oracle.encode_text, ids[sel], allh[sel].cpu(), "ViT-B/32 text, EOT 1 .. 76")


# ---- 5. the stand-alone row entry points -----------------------------------------------------------------------------------

@pytest.mark.parametrize("E", [512, 768, 1024])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1001])
def test_l2_normalize_rows_matches_float64(clipmi, gpu, n, E):
    """clipmi_l2_normalize_rows (include/clipmi.h): x / ||x|| per row in place, four rows per block (n = 3, 5, 1001: ragged
    last block); rows with a norm below 1e-9 (all zero, ~1e-12) stay unchanged; the row behind the last one is not touched.
    Measured on MI355X: max relative error 1.5e-7 against float64 over these shapes (an f32 sum of squares, one division)."""
    L = clipmi._lib.lib()
    rng = np.random.default_rng(n * 7 + E)
    x = (rng.standard_normal((n + 1, E)) * 10.0 ** rng.uniform(-3, 3, (n + 1, 1))).astype(np.float32)
    if n >= 3:
        x[1] = 0.0
        x[2] *= np.float32(1e-12 / np.linalg.norm(x[2].astype(np.float64)))
    if n >= 4:
        x[3] *= np.float32(1e-6 / np.linalg.norm(x[3].astype(np.float64)))     # small, but above the threshold
    xd = torch.from_numpy(x).to(gpu)
    clipmi._lib.check(L.clipmi_l2_normalize_rows(xd.data_ptr(), n, E, clipmi._lib.stream_ptr(gpu)), "l2_normalize_rows")
    got = xd.cpu().numpy()
    x64 = x.astype(np.float64)
    nrm = np.linalg.norm(x64, axis=1, keepdims=True)
    keep = nrm[:, 0] < 1e-9
    keep[n] = True                                      # the row past n
    want = np.where(keep[:, None], x64, x64 / np.where(keep[:, None], 1.0, nrm))
    assert np.array_equal(got[keep].view(np.uint32), x[keep].view(np.uint32)), "rows below the threshold / past n changed"
    nz = ~keep[:, None] & (want != 0)
    rel = np.abs(got.astype(np.float64) - want)[nz] / np.abs(want[nz])
    print(f"l2_normalize_rows n={n} E={E}: max relative error {rel.max():.3g}")
    assert rel.max() <= 1e-6


def test_l2_normalize_rows_n0_and_bad_arguments(clipmi, gpu):
    L = clipmi._lib.lib()
    x = torch.randn(4, 512, device=gpu)
    before = x.clone()
    assert L.clipmi_l2_normalize_rows(x.data_ptr(), 0, 512, None) == 0
    torch.cuda.synchronize(gpu)
    assert torch.equal(x, before)
    assert L.clipmi_l2_normalize_rows(None, 4, 512, None) == EINVAL
    assert L.clipmi_l2_normalize_rows(x.data_ptr(), -1, 512, None) == EINVAL
    assert L.clipmi_l2_normalize_rows(x.data_ptr(), 4, 0, None) == EINVAL
    assert "l2_normalize_rows" in clipmi._lib.last_error()
    torch.cuda.synchronize(gpu)
    assert torch.equal(x, before)


def _absmax(clipmi, gpu, xd):
    L = clipmi._lib.lib()
    N, E = xd.shape
    out = torch.full((N + 1,), -1.0, device=gpu)
    clipmi._lib.check(L.clipmi_rows_absmax(xd.data_ptr(), N, E, out.data_ptr(), clipmi._lib.stream_ptr(gpu)), "rows_absmax")
    got = out.cpu().numpy()
    assert got[N] == -1.0, "wrote past row N"
    return got[:N]


@pytest.mark.parametrize("E", [512, 768])
@pytest.mark.parametrize("N", [1, 33, 2049, 300_007])
def test_rows_absmax_matches_numpy(clipmi, gpu, N, E):
    """clipmi_rows_absmax (include/clipmi.h) == numpy's abs().max(1), bit for bit: row magnitudes over 80 binades, +-inf,
    zero and denormal rows, the largest component in the first / last column; grid-stride rows past 16 waves per CU."""
    g = torch.Generator(device=gpu)
    g.manual_seed(N + E)
    xd = torch.randn(N, E, generator=g, device=gpu) * torch.exp2(torch.randint(-40, 40, (N, 1), generator=g, device=gpu).float())
    if N > 1:
        xd[N // 2, 7] = float("inf")
        xd[N - 1, E - 1] = float("-inf")
        xd[0] = 0.0
        xd[0, 3] = -1e-40                               # denormal
        xd[N // 3, 0] = -3e38
    got = _absmax(clipmi, gpu, xd)
    want = np.abs(xd.cpu().numpy()).max(axis=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_rows_absmax_nan_rule_and_bad_arguments(clipmi, gpu):
    """The rule include/clipmi.h states: NaN components are skipped (fmaxf), so a row of NaN and finite values gives the
    largest finite |x|, NaN beside +-inf gives +inf and a row of NaN only gives 0 (numpy would return NaN for all three)."""
    L = clipmi._lib.lib()
    x = torch.randn(5, 512, dtype=torch.float64).float()
    x[0, ::3] = float("nan")
    x[1, 5] = float("nan")
    x[1, 400] = -float("inf")
    x[2] = float("nan")
    x[3, 0] = float("nan")                              # NaN as the first value of the row
    xd = x.to(gpu)
    got = _absmax(clipmi, gpu, xd)
    finite = torch.where(torch.isnan(x), torch.zeros_like(x), x).abs().amax(dim=1).numpy()
    assert got[0] == finite[0] and got[3] == finite[3] and got[4] == finite[4] and np.isfinite(got[0])
    assert got[1] == np.inf and got[2] == 0.0
    assert L.clipmi_rows_absmax(xd.data_ptr(), 5, 510, xd.data_ptr(), None) == EINVAL        # E % 4
    assert L.clipmi_rows_absmax(xd.data_ptr(), 0, 512, xd.data_ptr(), None) == EINVAL
    assert L.clipmi_rows_absmax(None, 5, 512, xd.data_ptr(), None) == EINVAL


# ---- 2. the other geometries at their largest single sequence --------------------------------------------------------------

def _wide_geometry(clipmi, gpu, model, forms, extra, seed, what):
    """Encode a device pool of max(forms) images as B in `forms` (pool[n - B:]), check image_lanes, and compare the boundary
    rows (plus `extra[B]`) bitwise with B = 1 encodes of the same images. Returns (pool, {pool index: row}, seconds per B)."""
    tokens, R = model.dims["v_tokens"], model.dims["res"]
    n = max(forms)
    pool = _pixels(gpu, n, R, seed)
    rows, secs = {}, {}
    for B, lanes in forms.items():
        assert model.image_lanes(B) == lanes, (what, B, model.image_lanes(B))
        s = n - B
        torch.cuda.synchronize(gpu)
        t0 = time.perf_counter()
        out = model.encode_image(pool[s:])
        torch.cuda.synchronize(gpu)
        secs[B] = time.perf_counter() - t0
        assert torch.isfinite(out).all(), f"{what} B={B}"
        for r in sorted(set(_boundary_rows(lanes, tokens)) | set(extra.get(B, ()))):
            row = out[r]
            if s + r in rows:
                _assert_same_bits(row[None], rows[s + r][None], f"{what}: B={B} row {r}")
            rows[s + r] = row
    for i, row in sorted(rows.items()):
        _assert_same_bits(row[None], model.encode_image(pool[i:i + 1]), f"{what}: pool image {i} vs B=1")
    print(f"{what}: {len(rows)} boundary rows bitwise == B=1; seconds per call " + ", ".join(f"B={B}: {t:.3f}" for B, t in secs.items()))
    return pool, rows, secs


def test_vit_b16_largest_sequences(clipmi, gpu):
    """ViT-B/16, 197 tokens (one-round chunk 443, full round 998): two lanes at 886, one sequence at max_batch, 998 + 27."""
    sd = clipmi.weights.random_state_dict("ViT-B/16", seed=2)
    model = clipmi.CLIP(sd, device=gpu)
    forms = {886: [(0, 443, 0), (443, 886, 1)], 1024: [(0, 1024, 0)], 1025: [(0, 998, 0), (998, 1025, 0)]}
    pool, rows, _ = _wide_geometry(clipmi, gpu, model, forms, {}, 22, "ViT-B/16")
    sel = [1025 - 886, 998, 1024]                       # first row of the two-lane call, both ends of the 1025 call's cut
    x = _normalized(clipmi, pool[sel].cpu())
    _check_oracle(clipmi, sd, clip_oracle.encode_image, x, torch.stack([rows[i] for i in sel]).cpu(), "ViT-B/16")


def test_vit_l14_336_largest_sequences(clipmi, gpu):
    """ViT-L/14@336px, 577 tokens (one-round chunk 511, full round 1022): two lanes at 1022; ONE sequence of 1024 images =
    590 848 token rows, whose c_fc output (x 4096) has 2.42e9 elements - every image from 909 on lies past element 2^31;
    1022 + 3 at 1025. Rows 908, 909, 1000, 1023 of the 1024 call bitwise == B = 1, row 1023 against the oracle; and the
    L/14 text tower's 77-position prompt (EOT 76) in Q = 1 / batch / device-id form and against the oracle."""
    sd = clipmi.weights.random_state_dict("ViT-L/14@336px", seed=0)
    model = clipmi.CLIP(sd, device=gpu)
    assert model.dims["v_tokens"] == 577 and 1024 * 577 * 4096 > 2 ** 31 > 908 * 577 * 4096 and 909 * 577 * 4096 > 2 ** 31 - 1
    forms = {1022: [(0, 511, 0), (511, 1022, 1)], 1024: [(0, 1024, 0)], 1025: [(0, 1022, 0), (1022, 1025, 0)]}
    pool, rows, secs = _wide_geometry(clipmi, gpu, model, forms, {1024: (908, 909, 1000, 1023)}, 23, "ViT-L/14@336px")
    torch.cuda.synchronize(gpu)
    t0 = time.perf_counter()
    again = model.encode_image(pool[1:])                # B = 1024 once more, its workspace already in place
    torch.cuda.synchronize(gpu)
    print(f"ViT-L/14@336px B=1024 (one sequence, 590 848 token rows): {time.perf_counter() - t0:.3f} s warm, "
          f"{secs[1024]:.3f} s first")
    for i in (909, 910, 1001, 1024):
        _assert_same_bits(again[i - 1][None], rows[i][None], f"ViT-L/14@336px B=1024 repeated, row {i - 1}")
    x = _normalized(clipmi, pool[1024:1025].cpu())
    _check_oracle(clipmi, sd, clip_oracle.encode_image, x, rows[1024][None].cpu(), "ViT-L/14@336px B=1024 row 1023")
    ids, pos = _prompts(model.dims, 33, [1, 6, 9, 40, 76])
    one = torch.cat([model.encode_text(ids[i:i + 1]) for i in range(ids.shape[0])])
    _assert_same_bits(model.encode_text(ids), one, "ViT-L/14 text, host ids")
    _assert_same_bits(model.encode_text(ids.to(gpu)), one, "ViT-L/14 text, device ids")
    k = pos.index(76)
    _check_oracle(clipmi, sd, clip_oracle.encode_text, ids[k:k + 1], one[k:k + 1].cpu(), "ViT-L/14 text, EOT 76")
