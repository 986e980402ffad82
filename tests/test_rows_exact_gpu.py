"""-m gpu: the towers' row kernels, kernel by kernel, in every form they run (data, references and bounds: tests/row_exact.py).

layernorm_kernel has seven forms selected by LnArgs; clipmi_dbg_layernorm_forms sets every field one to one.
* dense f32 -> f32 / bf16 (and in place): element by element under  C 2^-23 (A rstd |gamma| + |beta|)  (+ 2^-8 |ref| for bf16)
  against float64, on an exact data class (C = 3) and on test_layernorm's random data (C = 11); C comes from a float32
  restatement of the kernel's order on the CPU (test_rows_exact.py: worst ratios 0.636 and 2.623, times four, rounded up).
  A row that reads its neighbour's statistics is wrong by whole units of the per-row offset, a gamma or beta column off by one
  by eighths. The constant row must come out as beta exactly.
* gathered (rowidx) and strided (row_step) rows, f32 and split sources: bit-equal to the dense form's row of the same source
  row; every source row that must not be read is NaN.
* split input: bit-equal to the f32-input form on the joined values (random remainder bytes), and under the bound.
* e4m3 + row scale: the scale bit for bit and the bytes up to +-0 what torch's row quantiser makes of the bf16 form's rows.
* split output: the bytes and partials clipmi_dbg_split_stats makes of the f32 form's rows.
Every output buffer is NaN- or byte-pattern-filled and has a guard row behind row M; a buffer a form does not write stays so.

gather_rows, split_stats (integer rows: exact halves, remainder 128, exact statistics) and the two FP8 quantisers at the K
where their step loops change (512 values a step, a partly active last step) follow.

Worst observed err / bound on an MI355X, per form (the tests print every case's):
  dense f32, exact class   0.230      dense bf16, exact class   0.996 (the bf16 rounding's own half ulp against 2^-8 |ref|)
  dense f32, random class  0.232      dense bf16, random class  0.996
  split input (f32 out)    0.226      bf16 rows behind the FP8 form: beta0 0.184, random 0.996
The gathered, strided, in-place, FP8 and split-output forms are held bit for bit to these."""
import pytest
import torch

import gemm_exact as ge
import row_exact as rx

pytestmark = pytest.mark.gpu

NAN = rx.NAN
GUARD = rx.GUARD_BYTE


def _dev(c, gpu):
    return c["x"].to(gpu), c["gamma"].to(gpu), c["beta"].to(gpu)


# ---- LayerNorm: the dense forms carry the bound -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", rx.LN_W)
@pytest.mark.parametrize("cls", ["exact", "random"])
def test_layernorm_dense(clipmi, gpu, cls, W):
    """f32 -> f32 and f32 -> bf16, every M: the per-element bound; the constant row is beta; in place and the older hook give
    the same bits."""
    L = clipmi._lib.lib()
    for M in rx.LN_M:
        c = rx.ln_case(cls, M, W)
        x, gamma, beta = _dev(c, gpu)
        for out_bf16 in (0, 1):
            what = f"layernorm {cls} M={M} W={W} {'bf16' if out_bf16 else 'f32'}"
            out = rx.ln_dense(clipmi, gpu, x, gamma, beta, out_bf16)
            rx.assert_ln_bound(out, c, out_bf16, what)
            if cls == "exact" and M >= 3:
                want = c["beta"].to(out.dtype)
                assert torch.equal(rx.bits(out[1].cpu()), rx.bits(want)), f"{what}: the constant row is not beta"
            old = torch.full_like(out, NAN)
            clipmi._lib.check(L.clipmi_dbg_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), old.data_ptr(), M, W, out_bf16, None), what)
            assert torch.equal(rx.bits(old), rx.bits(out)), f"{what}: clipmi_dbg_layernorm differs"
            if not out_bf16:
                inplace = torch.full((M + 1, W), NAN, device=gpu)
                inplace[:M] = x
                clipmi._lib.check(rx.ln_forms(clipmi, M, W, gamma, beta, x=inplace, out=inplace), what)
                assert torch.isnan(inplace[M]).all() and torch.equal(rx.bits(inplace[:M]), rx.bits(out)), f"{what}: in place differs"


def test_layernorm_refusals(clipmi, gpu):
    x = torch.zeros(4, 2048, device=gpu)
    w = torch.ones(2048, device=gpu)
    x3 = torch.zeros(4, 3 * 2048, dtype=torch.uint8, device=gpu)
    part = torch.zeros(4, 8, 2, device=gpu)
    out = torch.full((4, 2048), NAN, device=gpu)
    for W in (6, 1028, 2):
        assert rx.ln_forms(clipmi, 4, W, w, w, x=x, out=out) == rx.EINVAL and "layernorm: W=" in clipmi._lib.last_error()
    for W in (260, 128, 1020):
        assert rx.ln_forms(clipmi, 4, W, w, w, x=x, out=out, out_x3=x3, out_part=part) == rx.EINVAL
        assert "split output" in clipmi._lib.last_error()
    assert rx.ln_forms(clipmi, 4, 256, w, w, x=x, out=out, out_x3=x3) == rx.EINVAL                  # split output without partials
    assert rx.ln_forms(clipmi, 4, 256, w, w, x=x, x3=x3, out=out) == rx.EINVAL                      # two sources
    assert rx.ln_forms(clipmi, 4, 256, w, w, out=out) == rx.EINVAL                                  # none
    assert rx.ln_forms(clipmi, 4, 256, w, w, x=x, out8=x3) == rx.EINVAL                             # e4m3 without scales
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- gather and stride ----------------------------------------------------------------------------------------------------------------
def _gather_plan(n, R):
    """n data rows (n >= 2) sit at `pos` among R source rows; -> (pos, pick): output row i is data row pick[i]. The index list
    has repeats, runs downwards, and includes source row 0 and the last source row."""
    g = torch.Generator(device="cpu"); g.manual_seed(n * 31 + R)
    pos = torch.cat([torch.tensor([0]), (torch.randperm(R - 2, generator=g)[:n - 2] + 1).sort().values, torch.tensor([R - 1])])
    pick = torch.cat([torch.arange(n - 1, -1, -1), torch.tensor([n - 1, n - 1, 0, 0]), torch.randint(0, n, (n // 2,), generator=g)])
    return pos, pick


def _check_rows(clipmi, gpu, W, gamma, beta, dense, pick, what, src=None, src3=None, rowidx=None, row_step=1):
    """One gathered / strided launch per output type; output row i must have the bits of dense[out type][pick[i]]."""
    M = pick.numel()
    for out_bf16 in (0, 1):
        out = torch.full((M + 1, W), NAN, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=gpu)
        clipmi._lib.check(rx.ln_forms(clipmi, M, W, gamma, beta, x=src, x3=src3, rowidx=rowidx, row_step=row_step, out=out, out_bf16=out_bf16), what)
        torch.cuda.synchronize()
        assert torch.isnan(out[M]).all(), f"{what}: wrote past row M"
        want = dense[out_bf16][pick.to(gpu)]
        bad = (rx.bits(out[:M]) != rx.bits(want)).any(1)
        assert not bad.any(), f"{what} {'bf16' if out_bf16 else 'f32'}: {int(bad.sum())} of {M} rows differ from the dense form's, first {int(bad.nonzero()[0])}"


def _sources(cls, n, W, R, pos, gpu, split):
    """-> (src, src3, dense): R source rows, NaN but for the case's n rows at `pos`; dense[out_bf16] = the dense form's rows"""
    if split:
        rows = rx.split_case_rows(cls, n, W).to(gpu)
        src3 = rx.nan_split_rows(R, W, gpu)
        src3[pos.to(gpu)] = rows
        return None, src3, rows
    rows = rx.ln_case(cls, n, W)["x"].to(gpu)
    src = torch.full((R, W), NAN, device=gpu)
    src[pos.to(gpu)] = rows
    return src, None, rows


def _dense_of(clipmi, gpu, rows, gamma, beta, split):
    return [rx.ln_dense(clipmi, gpu, None if split else rows, gamma, beta, o, x3=rows if split else None) for o in (0, 1)]


@pytest.mark.parametrize("W,split", [(W, 0) for W in rx.LN_W] + [(W, 1) for W in rx.LN_W_256])
def test_layernorm_gathered_rows(clipmi, gpu, W, split):
    """rowidx, as the text head reads the EOT rows (run_head: f32 or split residual rows). 5 data rows among 23, 11 output rows;
    1001 data rows among 1500 at two widths."""
    for cls, n, R in [("exact", 5, 23), ("random", 5, 23)] + ([("exact", 1001, 1500)] if W in (260, 768) else []):
        c = rx.ln_case(cls, n, W)
        _, gamma, beta = _dev(c, gpu)
        pos, pick = _gather_plan(n, R)
        assert pick.numel() > n and 0 in pos[pick] and R - 1 in pos[pick] and (pos[pick][1:] < pos[pick][:-1]).any()
        src, src3, rows = _sources(cls, n, W, R, pos, gpu, split)
        dense = _dense_of(clipmi, gpu, rows, gamma, beta, split)
        rowidx = pos[pick].to(torch.int32).to(gpu)
        _check_rows(clipmi, gpu, W, gamma, beta, dense, pick, f"layernorm gather {cls} n={n} W={W} split={split}", src, src3, rowidx)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("step", [1, 50, 77, 577])
def test_layernorm_strided_rows(clipmi, gpu, step, split):
    """row_step, as the vision head reads the class-token rows L apart."""
    for W in (rx.LN_W_256 if split else rx.LN_W):
        for cls, n in [("exact", 5), ("random", 4), ("random", 1)] + ([("exact", 1001)] if step == 50 and W == 768 else []):
            c = rx.ln_case(cls, n, W)
            _, gamma, beta = _dev(c, gpu)
            pos = torch.arange(n) * step
            src, src3, rows = _sources(cls, n, W, (n - 1) * step + 1, pos, gpu, split)
            dense = _dense_of(clipmi, gpu, rows, gamma, beta, split)
            _check_rows(clipmi, gpu, W, gamma, beta, dense, torch.arange(n), f"layernorm stride {step} {cls} n={n} W={W} split={split}",
                        src, src3, None, step)


# ---- split input ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", rx.LN_W_256)
def test_layernorm_split_input(clipmi, gpu, W):
    """x3 rows with random remainder bytes -> f32: the bits of the f32-input form on the joined values, and within the random
    class's bound of a float64 LayerNorm of them (a dropped or shifted remainder byte is off by up to 2^-8 |x|: thousands of
    times the bound)."""
    for M in rx.LN_M:
        c = rx.ln_case("random", M, W)
        _, gamma, beta = _dev(c, gpu)
        x3 = rx.split_case_rows("random", M, W)
        joined = rx.join(x3, W)
        assert torch.isfinite(joined).all() and not torch.equal(joined, c["x"].to(torch.bfloat16).float())
        ref, mean, rstd = rx.ln64(joined, c["gamma"], c["beta"])
        cj = dict(cls="random", ref=ref, unit=2.0 ** -23 * ((joined.double().abs() + mean.abs()) * rstd * c["gamma"].double().abs() + c["beta"].double().abs()))
        what = f"layernorm split input M={M} W={W}"
        got = rx.ln_dense(clipmi, gpu, None, gamma, beta, 0, x3=x3.to(gpu))
        via_f32 = rx.ln_dense(clipmi, gpu, joined.to(gpu), gamma, beta, 0)
        assert torch.equal(rx.bits(got), rx.bits(via_f32)), f"{what}: differs from the f32-input form on the joined values"
        rx.assert_ln_bound(got, cj, 0, what)


# ---- FP8 output -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", rx.LN_W_256)
@pytest.mark.parametrize("cls", ["beta0", "random"])
def test_layernorm_fp8_output(clipmi, gpu, cls, W):
    """out8 / scale8 against torch's row quantiser of the bf16 form's rows (which are held to the bound here too); the bf16
    buffer is not written. beta0: a row of zeros (scale 1, bytes 0) and a row of magnitude 1e-16."""
    for M in rx.LN_M:
        c = rx.ln_case(cls, M, W)
        x, gamma, beta = _dev(c, gpu)
        what = f"layernorm fp8 {cls} M={M} W={W}"
        rows = rx.ln_dense(clipmi, gpu, x, gamma, beta, 1)
        rx.assert_ln_bound(rows, c, 1, what + " (bf16 rows)")
        want8, want_s = rx.quant_rows(rows.cpu())
        out = torch.full((M + 1, W), NAN, dtype=torch.bfloat16, device=gpu)
        out8 = torch.full((M + 1, W), GUARD, dtype=torch.uint8, device=gpu)
        sc = torch.full((M + 1,), NAN, device=gpu)
        clipmi._lib.check(rx.ln_forms(clipmi, M, W, gamma, beta, x=x, out=out, out_bf16=1, out8=out8, scale8=sc), what)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), f"{what}: the bf16 buffer was written"
        assert (out8[M] == GUARD).all() and torch.isnan(sc[M]), f"{what}: wrote past row M"
        assert torch.equal(rx.bits(sc[:M].cpu()), rx.bits(want_s)), f"{what}: scales"
        rx.assert_e4m3_equal(out8[:M].cpu(), want8, what)
        if cls == "beta0" and M >= 3:
            assert sc[1].item() == 1.0 and not (out8[1] & 0x7f).any(), f"{what}: the row of zeros"
        if cls == "beta0" and M >= 4:
            assert 0 < sc[3].item() < 1e-17 and (out8[3] & 0x7f).any(), f"{what}: the tiny row"


# ---- split output -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", rx.LN_W_256)
@pytest.mark.parametrize("cls", ["exact", "random"])
def test_layernorm_split_output(clipmi, gpu, cls, W):
    """out_x3 / out_part: the bytes clipmi_dbg_split_stats makes of the f32 form's rows; the f32 buffer is not written."""
    L = clipmi._lib.lib()
    for M in rx.LN_M:
        c = rx.ln_case(cls, M, W)
        x, gamma, beta = _dev(c, gpu)
        what = f"layernorm split output {cls} M={M} W={W}"
        rows = rx.ln_dense(clipmi, gpu, x, gamma, beta, 0).contiguous()
        want3 = torch.full((M + 1, 3 * W), GUARD, dtype=torch.uint8, device=gpu)
        want_part = torch.full((M + 1, W // 256, 2), NAN, device=gpu)
        clipmi._lib.check(L.clipmi_dbg_split_stats(rows.data_ptr(), 0, want3.data_ptr(), want_part.data_ptr(), M, W, None), what)
        out = torch.full((M + 1, W), NAN, device=gpu)
        x3 = torch.full((M + 1, 3 * W), GUARD, dtype=torch.uint8, device=gpu)
        part = torch.full((M + 1, W // 256, 2), NAN, device=gpu)
        clipmi._lib.check(rx.ln_forms(clipmi, M, W, gamma, beta, x=x, out=out, out_x3=x3, out_part=part), what)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), f"{what}: the f32 buffer was written"
        assert (x3[M] == GUARD).all() and torch.isnan(part[M]).all() and (want3[M] == GUARD).all(), f"{what}: wrote past row M"
        # (split_stats itself: the hi halves are the bf16 of the rows, the join is within 2^-15 - test_kernels_gpu.py::test_split_stats)
        assert torch.equal(want3[:M, :2 * W].view(torch.bfloat16), rows.to(torch.bfloat16))
        assert torch.equal(x3[:M, :2 * W], want3[:M, :2 * W]), f"{what}: hi halves"
        assert torch.equal(x3[:M, 2 * W:], want3[:M, 2 * W:]), f"{what}: remainder bytes"
        assert torch.equal(rx.bits(part[:M]), rx.bits(want_part[:M])), f"{what}: partials"


# ---- gather_rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_", [1, 50])
@pytest.mark.parametrize("B", [1, 5, 257])
def test_gather_rows(clipmi, gpu, B, L_):
    """dst[b] = src[b L]: f32 rows (4 W bytes) and split rows (3 W bytes), W = 256 and 768; every other source row is filled with
    another byte pattern, the row behind the last destination row stays untouched."""
    L = clipmi._lib.lib()
    for rb in (4 * 256, 3 * 256, 4 * 768, 3 * 768):
        g = torch.Generator(device="cpu"); g.manual_seed(B * 7 + L_ + rb)
        rows = torch.randint(0, 256, (B, rb), generator=g).to(torch.uint8).to(gpu)
        assert ge.count_distinct(rows.view(torch.float64).cpu()) == B
        src = torch.full(((B - 1) * L_ + 1, rb), 0x3C, dtype=torch.uint8, device=gpu)
        src[::L_] = rows
        dst = torch.full((B + 1, rb), GUARD, dtype=torch.uint8, device=gpu)
        clipmi._lib.check(L.clipmi_dbg_gather_rows(src.data_ptr(), dst.data_ptr(), B, L_, rb, None), "gather_rows")
        torch.cuda.synchronize()
        assert (dst[B] == GUARD).all(), f"gather_rows B={B} L={L_} {rb} bytes: wrote past row B"
        assert torch.equal(dst[:B], rows), f"gather_rows B={B} L={L_} {rb} bytes"
    for rb in (24, 1000, 3 * 252):
        assert L.clipmi_dbg_gather_rows(src.data_ptr(), dst.data_ptr(), 1, 1, rb, None) == rx.EINVAL
        assert "gather_rows" in clipmi._lib.last_error()
    torch.cuda.synchronize()
    assert (dst[B] == GUARD).all()


# ---- split_stats on integers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", rx.LN_W_256)
@pytest.mark.parametrize("M", [1, 5, 1001])
def test_split_stats_integer_rows(clipmi, gpu, M, W):
    """Without add, on integers in [-8, 8] plus the per-row offset: the hi halves are the integers, every remainder byte is 128, the
    statistics are the exact sums."""
    L = clipmi._lib.lib()
    c = ge.redraw(lambda seed: torch.randint(-8, 9, (M, W), generator=torch.Generator().manual_seed(seed)).double() + ge.row_offset(M),
                  M * 3 + W, lambda x: ge.count_distinct(x) == M and (M == 1 or ge.count_distinct(x.t()) == W))
    want3 = ge.split_rows(c, gpu)
    want_part, _ = ge.exact_stats(c)
    x = c.float().to(gpu)
    x3 = torch.full((M + 1, 3 * W), GUARD, dtype=torch.uint8, device=gpu)
    part = torch.full((M + 1, W // 256, 2), NAN, device=gpu)
    clipmi._lib.check(L.clipmi_dbg_split_stats(x.data_ptr(), 0, x3.data_ptr(), part.data_ptr(), M, W, None), "split_stats")
    torch.cuda.synchronize()
    assert (x3[M] == GUARD).all() and torch.isnan(part[M]).all(), "wrote past row M"
    assert torch.equal(x3[:M, :2 * W].view(torch.bfloat16).double(), c.to(gpu)), "hi halves"
    assert (x3[:M, 2 * W:] == 128).all() and torch.equal(x3, want3), "remainder bytes"
    assert torch.equal(part[:M].cpu(), want_part), "statistics"


# ---- the FP8 quantisers at the edges of their step loops --------------------------------------------------------------------------------
def _quant_input(M, K, seed):
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-6, 7, (M, K // 8), generator=g).float()).repeat_interleave(8, dim=1))
    x = x.to(torch.bfloat16)
    x[0, K - 1] = 300.0                    # the row's largest magnitude in the last value of a partly active step
    if M > 1:
        x[1] = 0
        x[2, :K - 8] = 0                   # only the last lane's values
        x[3, K - 8:] = 0
    return x


@pytest.mark.parametrize("K", [8, 504, 512, 520, 3072])
@pytest.mark.parametrize("M", [1, 5])
def test_quantize_rows_fp8_step_edges(clipmi, gpu, M, K):
    L = clipmi._lib.lib()
    x = _quant_input(M, K, M + K)
    want8, want_s = rx.quant_rows(x)
    xd = x.to(gpu)
    out = torch.full((M + 1, K), GUARD, dtype=torch.uint8, device=gpu)
    sc = torch.full((M + 1,), NAN, device=gpu)
    clipmi._lib.check(L.clipmi_dbg_quantize_rows_fp8(xd.data_ptr(), out.data_ptr(), sc.data_ptr(), M, K, None), "quantize_rows_fp8")
    torch.cuda.synchronize()
    assert (out[M] == GUARD).all() and torch.isnan(sc[M]), "wrote past row M"
    assert torch.equal(rx.bits(sc[:M].cpu()), rx.bits(want_s)), f"M={M} K={K}: scales"
    rx.assert_e4m3_equal(out[:M].cpu(), want8, f"quantize_rows_fp8 M={M} K={K}")
    for bad in (K + 4, 4, 0):
        assert L.clipmi_dbg_quantize_rows_fp8(xd.data_ptr(), out.data_ptr(), sc.data_ptr(), M, bad, None) == rx.EINVAL


@pytest.mark.parametrize("K", [32, 480, 512, 544, 3072])
@pytest.mark.parametrize("M", [1, 5])
def test_quantize_rows_fp8mx_step_edges(clipmi, gpu, M, K):
    L = clipmi._lib.lib()
    x = _quant_input(M, K, M + K + 1)
    want8, want_sb = rx.quant_mx(x)
    assert K == 32 or want_sb[0].unique().numel() > 1             # scale bytes differ along a row
    xd = x.to(gpu)
    out = torch.full((M + 1, K), GUARD, dtype=torch.uint8, device=gpu)
    sb = torch.full((M + 1, K // 32), GUARD, dtype=torch.uint8, device=gpu)
    clipmi._lib.check(L.clipmi_dbg_quantize_rows_fp8mx(xd.data_ptr(), out.data_ptr(), sb.data_ptr(), M, K, None), "quantize_rows_fp8mx")
    torch.cuda.synchronize()
    assert (out[M] == GUARD).all() and (sb[M] == GUARD).all(), "wrote past row M"
    assert torch.equal(sb[:M].cpu(), want_sb), f"M={M} K={K}: scale bytes"
    rx.assert_e4m3_equal(out[:M].cpu(), want8, f"quantize_rows_fp8mx M={M} K={K}")
    for bad in (K + 8, K + 16, 16, 0):
        assert L.clipmi_dbg_quantize_rows_fp8mx(xd.data_ptr(), out.data_ptr(), sb.data_ptr(), M, bad, None) == rx.EINVAL
