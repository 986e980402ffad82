"""-m gpu: the kernels in front of the first transformer block, one by one and bit for bit where the arithmetic allows,
through clipmi_dbg_embed_image / clipmi_dbg_embed_text - the product's own launch sequence (csrc/encode.hip embed_image /
embed_text) with copies of what it leaves in the workspace. Cases, references and comparisons: tests/embed_cases.py
(checked on the CPU by tests/test_embed.py).

  patches      patchify_kernel (vector and scalar path, three input types), patchify_strip_u8_kernel: bit-equal to the
               reference (f32 rounded to nearest even, bf16 moved, u8 through the 256-entry table of float64 values)
  rows         EPI_PATCH_F32 in the skinny, the 128 x 128 and the 256 x 256 kernel + cls_rows_kernel: integer data
               bit-equal to the float64 reference at every batch size and kernel; u8 pixels with Gaussian weights within
               2e-4 x max |ref| (the f32-output rule of test_kernels_gpu.py); the kernels bit-equal to each other
  ln_pre       f32 form within 2e-5 x max |ref| of a float64 LayerNorm of the device's own rows; split form bit-equal to
               clipmi_dbg_layernorm + clipmi_dbg_split_stats
  text         text_embed_kernel + eot_rows_kernel bit-equal to one f32 add and the first argmax; text_embed_split_kernel
               bit-equal to clipmi_dbg_split_stats of those rows
Every output buffer and the workspace are pre-filled with NaN bit patterns: a row nobody wrote shows.

Measured on an MI355X, largest max |got - ref| / tolerance per geometry (the same for every kernel): u8 rows G1 0.0056,
G2 0.0015, G3 0.0016, G4 0.0008, G5 0.0055; ln_pre in f32 G1 0.0065 (bf16 and FP8 tower), G2 0.0069, G3 0.0068, G4 0.0052,
G5 0.0085. The tests print each figure."""
import pytest
import torch

import embed_cases as ec
from test_kernels_gpu import _check_split, _split

pytestmark = pytest.mark.gpu

_CODE = {torch.float32: ec.F32, torch.bfloat16: ec.BF16, torch.uint8: ec.U8}


@pytest.fixture(scope="module")
def towers(clipmi, gpu):
    """(geometry or text width, mode, weight format) -> (state dict, tower, blob), packed once per module."""
    cache = {}

    def get(name, mode, fmt="bf16"):
        key = (name, mode, fmt)
        if key not in cache:
            if isinstance(name, int):
                sd = ec.text_state_dict(name)
                tw, blob = clipmi.weights.pack_text(sd, gpu)
            else:
                sd = ec.vision_state_dict(name, mode)
                tw, blob = clipmi.weights.pack_vision(sd, gpu, weight_format=fmt)
            cache[key] = (sd, tw, blob)
        return cache[key]

    yield get
    cache.clear()


def _nan_bytes(n, gpu):
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=gpu)          # f32 0xFFFFFFFF and bf16 0xFFFF are NaNs


def _embed_image(clipmi, gpu, name, tw, blob, pix, algo, with_ln, want):
    """Run the hook; `want` names the outputs: "patches", "rows", "split" (x3 + part). Returns them in a dict."""
    L = clipmi._lib.lib()
    d = ec.dims(name)
    B = pix.shape[0]
    need = L.clipmi_encode_image_workspace_bytes(tw, B)
    assert need > 0, clipmi._lib.last_error()
    ws = _nan_bytes(need, gpu)
    out = {}
    if "patches" in want:
        out["patches"] = _nan_bytes(B * d["np"] * d["patch_k"] * 2, gpu).view(torch.bfloat16).reshape(B * d["np"], d["patch_k"])
    if "rows" in want:
        out["rows"] = torch.full((B * d["L"], d["W"]), float("nan"), dtype=torch.float32, device=gpu)
    if "split" in want:
        out["x3"] = _nan_bytes(B * d["L"] * 3 * d["W"], gpu).reshape(B * d["L"], 3 * d["W"])
        out["part"] = torch.full((B * d["L"], d["W"] // 256, 2), float("nan"), dtype=torch.float32, device=gpu)
    ptr = lambda k: out[k].data_ptr() if k in out else None
    rc = L.clipmi_dbg_embed_image(tw, blob.data_ptr(), pix.data_ptr(), _CODE[pix.dtype], B, algo, with_ln, ptr("patches"),
                                  ptr("rows"), ptr("x3"), ptr("part"), ws.data_ptr(), ws.numel(), None)
    clipmi._lib.check(rc, f"dbg_embed_image {name} B={B} algo={algo}")
    torch.cuda.synchronize()
    return out


_CASES = [(n, b) for n in ec.GEOMS for b in ec.BATCHES[n]]


@pytest.mark.parametrize("name,B", _CASES)
def test_patches_are_bit_exact(clipmi, gpu, towers, name, B):
    """u8 (strip kernel: G1, G2, G5; generic kernel's vector path: G4, scalar path: G3), f32 values that need rounding,
    bf16 values moved: every bit of the patch matrix, the +0 columns beyond 3 P^2 included."""
    _, tw, blob = towers(name, "gauss")
    x32 = ec.rounding_pixels(name, B)
    for pix in (ec.u8_pixels(name, B), x32, x32.to(torch.bfloat16)):
        pix = pix.to(gpu)
        got = _embed_image(clipmi, gpu, name, tw, blob, pix, 0, 0, ("patches",))["patches"]
        ok, bad = ec.same_bits(got, ec.ref_patches(pix, name))
        assert ok, f"{name} B={B} {pix.dtype}: {bad} patch elements differ"


@pytest.mark.parametrize("name,B", _CASES)
def test_rows_exact_mode(clipmi, gpu, towers, name, B):
    """Integer pixels and weights, positional rows in eighths: the rows in front of ln_pre equal the float64 reference
    bit for bit, for f32 and bf16 input, every batch size and every kernel that takes the shape."""
    sd, tw, blob = towers(name, "exact")
    x = ec.exact_pixels(name, B).to(gpu)
    ref = ec.ref_rows(ec.ref_patches(x, name), sd, name)
    first = None
    for dtype in (torch.float32, torch.bfloat16):
        for algo in ec.algos(name):
            got = _embed_image(clipmi, gpu, name, tw, blob, x.to(dtype), algo, 0, ("patches", "rows"))
            assert ec.same_bits(got["patches"], ec.ref_patches(x.to(dtype), name))[0]
            ok, bad = ec.rows_exact(got["rows"], ref)
            assert ok, f"{name} B={B} {dtype} algo {algo}: {bad} elements differ from the exact reference"
            first = got["rows"] if first is None else first
            assert ec.same_bits(got["rows"], first)[0]


@pytest.mark.parametrize("name,B", _CASES)
def test_rows_u8_within_gemm_tolerance(clipmi, gpu, towers, name, B):
    """u8 pixels, Gaussian weights: max |got - ref| <= 2e-4 x max |ref| against float64 on the verified bf16 patches;
    the kernels agree bit for bit."""
    sd, tw, blob = towers(name, "gauss")
    pix = ec.u8_pixels(name, B).to(gpu)
    patches = ec.ref_patches(pix, name)
    ref = ec.ref_rows(patches, sd, name)
    first = None
    for algo in ec.algos(name):
        got = _embed_image(clipmi, gpu, name, tw, blob, pix, algo, 0, ("patches", "rows"))
        assert ec.same_bits(got["patches"], patches)[0]
        ok, ratio = ec.rows_within(got["rows"], ref, ec.GEMM_REL)
        print(f"embed figure: rows {name} u8 B={B} algo {algo}: max |got - ref| / tolerance = {ratio:.4g}")
        assert ok, f"{name} B={B} algo {algo}: {ratio:.4g} x the tolerance"
        first = got["rows"] if first is None else first
        assert ec.same_bits(got["rows"], first)[0], f"algo {algo} differs from algo 0"


@pytest.mark.parametrize("name,B,fmt", [(n, b, "bf16") for n, b in _CASES] + [("G1", b, "fp8") for b in ec.BATCHES["G1"]])
def test_ln_pre(clipmi, gpu, towers, name, B, fmt):
    """ln_pre on the device's own rows. Towers that keep f32 rows (ln_fold 0: G2, G4; FP8 weights): a float64 LayerNorm
    within 2e-5 x max |ref|. bf16 LN-folded towers (G1, G3, G5): the split rows and statistics partials it writes itself
    are the bits of a LayerNorm pass to f32 followed by split_stats_kernel ("what split_stats_kernel would make of it")."""
    L = clipmi._lib.lib()
    d = ec.dims(name)
    sd, tw, blob = towers(name, "gauss", fmt)
    split = fmt == "bf16" and d["W"] % 256 == 0
    assert bool(tw.ln_fold) == split
    pix = ec.u8_pixels(name, B).to(gpu)
    pre = _embed_image(clipmi, gpu, name, tw, blob, pix, 0, 0, ("rows",))["rows"]
    assert torch.isfinite(pre).all()
    lnw, lnb = sd["visual.ln_pre.weight"].to(gpu), sd["visual.ln_pre.bias"].to(gpu)
    if not split:
        got = _embed_image(clipmi, gpu, name, tw, blob, pix, 0, 1, ("rows",))["rows"]
        ok, ratio = ec.rows_within(got, ec.ref_ln(pre, lnw, lnb), ec.LN_REL)
        print(f"embed figure: ln_pre {name} {fmt} B={B}: max |got - ref| / tolerance = {ratio:.4g}")
        assert ok, f"{name} {fmt} B={B}: {ratio:.4g} x the tolerance"
        return
    got = _embed_image(clipmi, gpu, name, tw, blob, pix, 0, 1, ("split",))
    M, W = pre.shape
    y = torch.full((M, W), float("nan"), dtype=torch.float32, device=gpu)
    clipmi._lib.check(L.clipmi_dbg_layernorm(pre.data_ptr(), lnw.data_ptr(), lnb.data_ptr(), y.data_ptr(), M, W, 0, None), "ln")
    torch.cuda.synchronize()
    ok, ratio = ec.rows_within(y, ec.ref_ln(pre, lnw, lnb), ec.LN_REL)
    print(f"embed figure: ln_pre {name} {fmt} B={B} (f32 pass behind the split form): max |got - ref| / tolerance = {ratio:.4g}")
    assert ok
    x3, part = _split(clipmi, L, y)
    assert torch.equal(got["x3"], x3), "split rows differ from LayerNorm + split_stats"
    assert ec.same_bits(got["part"], part)[0], "statistics partials differ from LayerNorm + split_stats"
    _check_split(y, got["x3"], got["part"])


def _embed_text(clipmi, gpu, tw, blob, ids, want_split):
    L = clipmi._lib.lib()
    Q, ctx = ids.shape
    W = tw.width
    need = L.clipmi_encode_text_workspace_bytes(tw, Q)
    assert need > 0, clipmi._lib.last_error()
    ws = _nan_bytes(need, gpu)
    out = {"rowidx": torch.full((Q,), -1, dtype=torch.int32, device=gpu)}
    if want_split:
        out["x3"] = _nan_bytes(Q * ctx * 3 * W, gpu).reshape(Q * ctx, 3 * W)
        out["part"] = torch.full((Q * ctx, W // 256, 2), float("nan"), dtype=torch.float32, device=gpu)
    else:
        out["rows"] = torch.full((Q * ctx, W), float("nan"), dtype=torch.float32, device=gpu)
    ptr = lambda k: out[k].data_ptr() if k in out else None
    rc = L.clipmi_dbg_embed_text(tw, blob.data_ptr(), ids.data_ptr(), Q, ptr("rows"), ptr("x3"), ptr("part"),
                                 out["rowidx"].data_ptr(), ws.data_ptr(), ws.numel(), None)
    clipmi._lib.check(rc, f"dbg_embed_text W={W} Q={Q}")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("Q", ec.TEXT_Q)
@pytest.mark.parametrize("width", sorted(ec.TEXT_TOWERS))
def test_text_embedding(clipmi, gpu, towers, width, Q):
    """Width 128: text_embed_kernel + eot_rows_kernel; 512 and 768: text_embed_split_kernel, whose split rows and
    partials must be "the bits of the three kernels". Prompts with the maximum id first, last, twice, all ids equal and
    ids outside [0, vocab)."""
    L = clipmi._lib.lib()
    sd, tw, blob = towers(width, None)
    fused = width % 256 == 0
    assert bool(tw.ln_fold) == fused
    ids = ec.text_ids(width, Q).to(gpu)
    rows = ec.ref_text_rows(sd, ids)
    got = _embed_text(clipmi, gpu, tw, blob, ids, fused)
    assert torch.equal(got["rowidx"], ec.ref_rowidx(ids))
    if not fused:
        ok, bad = ec.same_bits(got["rows"], rows)
        assert ok, f"{bad} elements differ from token + positional embedding"
        return
    x3, part = _split(clipmi, L, rows)
    assert torch.equal(got["x3"], x3), "split rows differ from split_stats of the f32 rows"
    assert ec.same_bits(got["part"], part)[0], "statistics partials differ from split_stats of the f32 rows"
    _check_split(rows, got["x3"], got["part"])


def test_embed_hooks_reject_bad_arguments(clipmi, gpu, towers):
    L = clipmi._lib.lib()
    err = clipmi._lib.last_error
    _, tw, blob = towers("G2", "gauss")                      # width 128: f32 rows, no 256 x 256 kernel
    pix = ec.u8_pixels("G2", 2).to(gpu)
    need = L.clipmi_encode_image_workspace_bytes(tw, 2)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    x = torch.empty(1 << 20, dtype=torch.float32, device=gpu)

    def image(blob_p=blob.data_ptr(), pix_p=pix.data_ptr(), dtype=ec.U8, B=2, algo=0, with_ln=0, rows=None, x3=None, part=None,
              ws_p=ws.data_ptr(), ws_bytes=need, tower=tw):
        return L.clipmi_dbg_embed_image(tower, blob_p, pix_p, dtype, B, algo, with_ln, None, rows, x3, part, ws_p, ws_bytes, None)

    assert image() == 0
    assert image(tower=None) == 1 and "NULL tower" in err()
    for kw in (dict(blob_p=None), dict(pix_p=None), dict(ws_p=None)):
        assert image(**kw) == 1 and "dbg_embed_image: NULL pointer" in err()
    assert image(B=0) == 1 and "B=0" in err()
    assert image(B=-3) == 1 and "B=-3" in err()
    assert image(dtype=3) == 1 and "pix_dtype 3" in err()
    assert image(ws_bytes=need - 1) == 2 and "workspace" in err()
    assert image(algo=3) == 1 and "algo 3" in err()
    assert image(algo=2) == 1 and "algo 2" in err()
    assert image(with_ln=1, x3=x.data_ptr(), part=x.data_ptr()) == 1 and "f32 rows" in err()
    _, tw1, blob1 = towers("G1", "gauss")                    # LN-folded: split rows behind ln_pre, f32 rows in front of it
    need1 = L.clipmi_encode_image_workspace_bytes(tw1, 1)
    ws1 = torch.empty(need1, dtype=torch.uint8, device=gpu)
    pix1 = ec.u8_pixels("G1", 1).to(gpu)
    assert image(tower=tw1, blob_p=blob1.data_ptr(), pix_p=pix1.data_ptr(), B=1, with_ln=1, rows=x.data_ptr(), ws_p=ws1.data_ptr(),
                 ws_bytes=need1) == 1 and "split rows" in err()
    assert image(tower=tw1, blob_p=blob1.data_ptr(), pix_p=pix1.data_ptr(), B=1, with_ln=0, x3=x.data_ptr(), ws_p=ws1.data_ptr(),
                 ws_bytes=need1) == 1 and "f32 rows" in err()
    _, tt, tblob = towers(128, None)
    assert image(tower=tt) == 1 and "tower kind" in err()

    ids = ec.text_ids(128, 2).to(gpu)
    tneed = L.clipmi_encode_text_workspace_bytes(tt, 2)
    tws = torch.empty(tneed, dtype=torch.uint8, device=gpu)

    def text(blob_p=tblob.data_ptr(), ids_p=ids.data_ptr(), Q=2, x3=None, ws_p=tws.data_ptr(), ws_bytes=tneed, tower=tt):
        return L.clipmi_dbg_embed_text(tower, blob_p, ids_p, Q, None, x3, None, None, ws_p, ws_bytes, None)

    assert text() == 0
    for kw in (dict(blob_p=None), dict(ids_p=None), dict(ws_p=None)):
        assert text(**kw) == 1 and "dbg_embed_text: NULL pointer" in err()
    assert text(Q=0) == 1 and "Q=0" in err()
    assert text(ws_bytes=tneed - 1) == 2 and "workspace" in err()
    assert text(x3=x.data_ptr()) == 1 and "f32 rows" in err()
    assert text(tower=tw) == 1 and "tower kind" in err()
    torch.cuda.synchronize()
