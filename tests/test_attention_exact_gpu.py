"""-m gpu: the attention kernels of csrc/attention.hpp on data whose right answer is known to the bit, on random data under a
per-element bound, and the fused FP8 output stage byte for byte (data, conditions, references: tests/attention_exact.py; the
same conditions and float32 models of the kernels run without a GPU in tests/test_attention_exact.py).

1. Exact classes (test_exact_classes): selection, causal trap, ties, ramps, uniform and L = 1 over attention_exact.exact_shapes(),
   which names the instantiation and edge every shape is there for. The output must EQUAL the expected bytes. Two hardware facts
   carry the equalities: v_exp_f32 gives exactly 1 at 0 and exactly 0 at or below 2^-184.
2. Random data (test_random_data_within_the_bound): test_attention's and test_attention_long_sequences' inputs at three scales
   and with outlier rows, element by element under |got - o| <= 2^-8 (|o| + pav) (1 + 2^-6): 2^-8 |o| is the half-ulp of the
   bf16 output, 2^-8 pav = 2^-8 softmax(s) |v| the half-ulp of every P's bf16 rounding weighted by |v| (normalised P in the short
   kernels, unnormalised in the flash kernel), 2^-6 of that for the f32 accumulation over at most 577 keys and the 1-ulp exp.
3. attention52x4_kernel<true> through clipmi_dbg_attention_fp8mx: its e4m3 rows and MX scale bytes equal what
   clipmi_dbg_quantize_rows_fp8mx makes of clipmi_dbg_attention's bf16 rows, equal the torch model of the quantiser on V[pi(q)]
   for selection data, and meet per-head magnitudes (zero, 2^-20, below the scale clamp, 2^20, two blocks 2^10 apart).
4. The launcher's refusals and its empty batch.
Every output buffer is NaN- (or byte-) filled and followed by guard rows of a byte pattern that must survive; every row below
them must be finite. The entry has no mask argument, so "L = 50 causal is not fused" cannot be asked of it: that the mask takes
49 <= L <= 52 off the ViT-B/32 kernels is seen in the exact causal cases at L = 50 and 52."""
import ctypes as C

import pytest
import torch

import attention_exact as ax
from test_fp8_gpu import _quant_mx

pytestmark = pytest.mark.gpu

FILL8 = 0x5C
NAN_BF16 = 0x7FC0


# ---- 1. exact classes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,build,flags", [pytest.param(n, b, f, id=i) for i, n, b, f in ax.exact_params()])
def test_exact_classes(clipmi, gpu, name, build, flags):
    c = build()
    for f in flags:
        ax.check_exact(clipmi, gpu, c, f)


# ---- 2. random data ---------------------------------------------------------------------------------------------------------------
RANDOM = [(B, L, h, c, f) for B, L, h, c in ax.SHORT_RANDOM for f in (0, 2)] + [(B, L, h, 0, 0) for B, L, h in ax.LONG_RANDOM]


@pytest.mark.parametrize("scale", ax.SCALES)
@pytest.mark.parametrize("B,L,heads,causal,flags", RANDOM)
def test_random_data_within_the_bound(clipmi, gpu, B, L, heads, causal, flags, scale):
    """The bound is derived (module docstring), not measured. For the record, the largest |got - o| / bound on an MI355X, equal to
    three digits to the float32 models' on the CPU (flags 0 and 2 give the same bits):
        B   L  heads causal   x 0.25  x 1.5   x 4   outliers        B   L  heads   x 0.25  x 1.5   x 4   outliers
        5   5    2     0      0.588  0.680  0.727   0.680           3   81    2    0.296  0.548  0.760   0.624
        4  16    2     1      0.674  0.828  0.697   0.828           1  128    1    0.205  0.466  0.699   0.466
        7  33    3     0      0.471  0.757  0.812   0.757           1  129    3    0.285  0.525  0.672   0.531
        3  50   12     0      0.438  0.727  0.848   0.812           2  197   12    0.247  0.660  0.729   0.641
      257  50   12     0      0.468  0.861  0.935   0.861           1  257   16    0.200  0.596  0.856   0.580
        1  64   12     0      0.342  0.765  0.889   0.795           2  577   16    0.175  0.532  0.806   0.548
        2  77    8     1      0.750  0.852  0.797   0.852
        2  80    8     1      0.812  0.796  0.893   0.796
    A float32 model whose P is truncated to bf16 instead of rounded reaches 1.04 to 1.38 at x 4 in each of these cases but the
    first (0.98)."""
    c = ax.random_case(B, L, heads, causal, scale)
    got = ax.run_attention(clipmi, gpu, c, flags | causal)
    ratio, outside = ax.worst_ratio(got, c)
    print(f"RATIO {c['what']} flags={flags | causal}: {ratio:.3f}")
    assert outside == 0, f"{c['what']} flags={flags | causal}: {outside} elements outside the bound, worst err / bound {ratio}"


# ---- 3. the fused FP8 output stage ------------------------------------------------------------------------------------------------
def run_fp8(clipmi, gpu, qkv, B, L, heads):
    """clipmi_dbg_attention_fp8mx into guarded buffers -> (out_bf16, out_fp8, bscale, fused), guards checked"""
    rows, W = B * L, heads * 64
    o16 = ax.guarded(rows, W, torch.bfloat16, gpu, ax.NAN)
    o8 = ax.guarded(rows, W, torch.uint8, gpu, FILL8)
    bs = ax.guarded(rows, W // 32, torch.uint8, gpu, FILL8)
    qd = qkv.to(gpu)
    fused = C.c_int(-1)
    rc = clipmi._lib.lib().clipmi_dbg_attention_fp8mx(qd.data_ptr(), o16.data_ptr(), o8.data_ptr(), bs.data_ptr(), B, L, heads,
                                                     C.byref(fused), None)
    clipmi._lib.check(rc, "attention_fp8mx")
    torch.cuda.synchronize()
    assert ax.guards_intact(o16, rows) and ax.guards_intact(o8, rows) and ax.guards_intact(bs, rows), "wrote past row B L"
    return o16[:rows], o8[:rows], bs[:rows], fused.value


def quantize_on_device(clipmi, gpu, rows16):
    M, W = rows16.shape
    q = torch.full((M, W), FILL8, dtype=torch.uint8, device=gpu)
    s = torch.full((M, W // 32), FILL8, dtype=torch.uint8, device=gpu)
    clipmi._lib.check(clipmi._lib.lib().clipmi_dbg_quantize_rows_fp8mx(rows16.data_ptr(), q.data_ptr(), s.data_ptr(), M, W, None), "quantize")
    torch.cuda.synchronize()
    return q, s


def check_fused(clipmi, gpu, c):
    """fused == 1, bf16 buffer untouched, bytes == the stand-alone quantiser's of clipmi_dbg_attention's rows -> (rows16, o8, bs)"""
    B, L, heads, what = c["B"], c["L"], c["heads"], c["what"]
    o16, o8, bs, fused = run_fp8(clipmi, gpu, c["qkv"], B, L, heads)
    assert fused == 1, what
    assert (o16.view(torch.int16) == NAN_BF16).all(), f"{what}: the fused stage wrote bf16 rows"
    rows16 = ax.run_attention(clipmi, gpu, c, 0)
    q, s = quantize_on_device(clipmi, gpu, rows16)
    ax.assert_same_bytes(bs, s, f"{what}: scale bytes against the stand-alone quantiser")
    ax.assert_same_bytes(o8, q, f"{what}: e4m3 bytes against the stand-alone quantiser")
    return rows16, o8, bs


def random_qkv(B, L, heads):
    x = torch.randn(B * L, 3 * heads * 64, generator=ax.gen(B * 77 + L * 5 + heads)) * 1.5
    return dict(qkv=x.to(torch.bfloat16), B=B, L=L, heads=heads, causal=0, what=f"fp8 random B={B} L={L} heads={heads}")


@pytest.mark.parametrize("B,L,heads", [(2, L, h) for L in (49, 50, 51, 52) for h in (1, 3, 12)] + [ax.MANY_ITEMS])
def test_fused_fp8_bytes_equal_the_quantiser(clipmi, gpu, B, L, heads):
    check_fused(clipmi, gpu, random_qkv(B, L, heads))


@pytest.mark.parametrize("B,L,heads", [(1, 49, 1), (7, 50, 3), (3, 51, 2), (1, 52, 3), (1, 50, 12), ax.MANY_ITEMS])
def test_fused_fp8_anchor_on_selection_data(clipmi, gpu, B, L, heads):
    """out[q] = V[pi(q)] exactly, so the bytes are the torch model of the MX quantiser applied to the expected rows: the scale
    byte is the block maximum's exponent field - 7 clamped at 0, the values e4m3 of x 2^-(sb - 127), nearest even, saturating."""
    c = ax.selection_case(B, L, heads, 0, "perm")
    _, o8, bs = check_fused(clipmi, gpu, c)
    q_ref, s_ref = _quant_mx(c["expect"])
    ax.assert_same_bytes(bs, s_ref, f"{c['what']}: scale bytes against the model")
    ax.assert_same_bytes(o8, q_ref, f"{c['what']}: e4m3 bytes against the model")


HEAD_SCALES = [0.0, 2.0 ** -20, 2.0 ** -130, 2.0 ** 20, None, 2.0 ** -124, 1.0]    # None: columns 32 .. 63 times 2^10


@pytest.mark.parametrize("L", [49, 50, 51, 52])
def test_fused_fp8_per_head_magnitudes(clipmi, gpu, L):
    """Selection data with V scaled per head (powers of two: P stays one-hot, the rows stay exact): all zero (scale byte 127 =
    2^0), 2^-20, 2^-130 (bf16 subnormals, below the scale clamp), 2^20, one head whose second 32-column block is 2^10 louder than
    its first (a swapped h * 2 + j, or a block maximum over the wrong lanes, changes a scale byte by 10), 2^-124 (normal numbers
    below the clamp) and 1."""
    B, heads = 2, len(HEAD_SCALES)
    W = heads * 64
    c = dict(ax.selection_case(B, L, heads, 0, "perm"))
    mul = torch.ones(W, dtype=torch.float64)
    for h, sc in enumerate(HEAD_SCALES):
        if sc is None:
            mul[h * 64 + 32:(h + 1) * 64] = 2.0 ** 10
        else:
            mul[h * 64:(h + 1) * 64] = sc
    qkv = c["qkv"].clone()
    v = qkv[:, 2 * W:].double() * mul + 0.0                      # (+ 0.0: the zero head holds +0 only)
    qkv[:, 2 * W:] = v.to(torch.bfloat16)
    want = c["expect"].double() * mul + 0.0
    expect = want.to(torch.bfloat16)
    assert torch.equal(qkv[:, 2 * W:].double(), v) and torch.equal(expect.double(), want)
    c.update(qkv=qkv, expect=expect, what=f"fp8 per-head magnitudes L={L}")
    rows16, o8, bs = check_fused(clipmi, gpu, c)
    q_ref, s_ref = _quant_mx(rows16.cpu())
    ax.assert_same_bytes(bs, s_ref, f"{c['what']}: scale bytes against the model of the kernel's own rows")
    ax.assert_same_bytes(o8, q_ref, f"{c['what']}: e4m3 bytes against the model of the kernel's own rows")
    sub = slice(2 * 64, 3 * 64)                                  # the 2^-130 head: whether the matrix cores keep bf16 subnormals
    keep = torch.ones(W, dtype=torch.bool)
    keep[sub] = False
    print(f"{c['what']}: subnormal head exact: {torch.equal(rows16.cpu()[:, sub], expect[:, sub])}")
    ax.assert_same_bytes(rows16[:, keep], expect[:, keep], f"{c['what']}: bf16 rows")
    bs = bs.cpu().reshape(B * L, heads, 2)
    assert (bs[:, 0] == 127).all(), "a block of zeros takes the scale byte of 2^0"
    assert (bs[:, 5] == 0).all(), "2^-124 .. 2^-120: the clamp at 0"
    e = expect.double().reshape(B * L, heads, 2, 32).abs().amax(-1)
    both = (e[:, 4, 0] > 0) & (e[:, 4, 1] > 0)
    lo, hi = torch.floor(torch.log2(e[both, 4, 0])), torch.floor(torch.log2(e[both, 4, 1]))
    assert both.any() and torch.equal(bs[both, 4, 0].double(), lo + 120) and torch.equal(bs[both, 4, 1].double(), hi + 120)
    assert (bs[both, 4, 1].int() - bs[both, 4, 0].int() >= 6).all()           # 2^10 apart, |v| in [1, 16]


@pytest.mark.parametrize("B,L,heads", [(3, 53, 3), (3, 48, 3), (1, 197, 2)])
def test_shapes_without_a_fused_stage_write_bf16_rows(clipmi, gpu, B, L, heads):
    c = ax.selection_case(B, L, heads, 0, "perm")
    o16, o8, bs, fused = run_fp8(clipmi, gpu, c["qkv"], B, L, heads)
    assert fused == 0
    assert (o8 == FILL8).all() and (bs == FILL8).all(), f"{c['what']}: the fp8 buffers were written"
    ax.assert_same_bytes(o16, c["expect"], c["what"])


# ---- 4. launcher answers ------------------------------------------------------------------------------------------------------------
def test_launcher_answers(clipmi, gpu):
    L = clipmi._lib.lib()
    qkv = torch.zeros(4 * 81, 3 * 128, dtype=torch.bfloat16, device=gpu)
    out = ax.guarded(4 * 81, 128, torch.bfloat16, gpu, ax.NAN)
    o8 = ax.guarded(4 * 81, 128, torch.uint8, gpu, FILL8)
    bs = ax.guarded(4 * 81, 4, torch.uint8, gpu, FILL8)
    fused = C.c_int(-1)
    args8 = (qkv.data_ptr(), out.data_ptr(), o8.data_ptr(), bs.data_ptr())
    assert L.clipmi_dbg_attention(qkv.data_ptr(), out.data_ptr(), 1, 0, 2, 0, None) == 1 and "L=0" in clipmi._lib.last_error()
    assert L.clipmi_dbg_attention(qkv.data_ptr(), out.data_ptr(), 4, 81, 2, 1, None) == 4 and "causal" in clipmi._lib.last_error()
    assert L.clipmi_dbg_attention(qkv.data_ptr(), out.data_ptr(), 1, 578, 2, 1, None) == 4 and "causal" in clipmi._lib.last_error()
    assert L.clipmi_dbg_attention(qkv.data_ptr(), out.data_ptr(), 0, 50, 2, 0, None) == 0
    assert L.clipmi_dbg_attention(None, out.data_ptr(), 1, 50, 2, 0, None) == 1
    assert L.clipmi_dbg_attention(qkv.data_ptr(), None, 1, 50, 2, 0, None) == 1
    assert L.clipmi_dbg_attention_fp8mx(*args8, 0, 50, 2, C.byref(fused), None) == 0 and fused.value == 0
    assert L.clipmi_dbg_attention_fp8mx(*args8, 1, 0, 2, C.byref(fused), None) == 1
    for i in range(4):
        a = list(args8)
        a[i] = None
        assert L.clipmi_dbg_attention_fp8mx(*a, 1, 50, 2, C.byref(fused), None) == 1
    assert L.clipmi_dbg_attention_fp8mx(*args8, 1, 50, 2, None, None) == 1
    torch.cuda.synchronize()
    assert (out[:4 * 81].view(torch.int16) == NAN_BF16).all() and ax.guards_intact(out, 4 * 81), "a refused or empty call wrote rows"
    assert (o8[:4 * 81] == FILL8).all() and (bs[:4 * 81] == FILL8).all()
