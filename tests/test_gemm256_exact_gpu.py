"""-m gpu: the non-persistent 256-tile GEMM (gemm256.hpp: one schedule and epilogue, expanded for bf16, FP8 and FP8 with
block-scaled A) on EXACT data, for the forms that no other test pins bit for bit: the f32 epilogues, the plain FP8 MFMA
form and block-scaled A. (The bf16-out forms of gemm256 and the MX form of gemm256f8 are also pinned against the persistent
kernel in test_kernels_gpu.py / test_fp8_gpu.py; QuickGELU is not exact and stays there.)

A is dense in {-1, 0, 1}, W 5 % dense in {-1, 1}, bias and residual are small integers, the FP8 row / channel / block
scales are powers of two in 2^-2 .. 2^2 (the e4m3 bytes hold the integers divided by them): every product, partial sum,
scaling and add is exact in f32 and every result an integer that bf16 holds, so the output must EQUAL torch's - a stale
or early LDS read anywhere in the DMA pipeline shows as a wrong integer. Shapes: an M-edge tile with four K-tiles (both A halves, both LDS buffers reused) and the
smallest K each form accepts (two K-tiles: the steady-state loop body runs once).

The persistent FP8 kernel (gemm256p_bf16_nt_kernel<EPI, true>: w_scale in LDS, each tile's 256 a_scale values by LDS-DMA) runs on
the same recipe at the default form (sel = 0) from more than one round of 256 tiles on, with the float64 product computed on the
device: test_gemm_fp8_exact_at_persistent_shapes. clipmi_dbg_gemm_fp8_plan says which kernel a case runs on, and the test pins
its answer: the persistent kernel has the pure-store epilogues 0 and 1 only (EPI_MASK_FP8_256P - its residual form does not fit
256 registers), so epilogues 2 and 3 of these shapes run on gemm256f8 at 129 row tiles, and 32768 x 512 - exactly 256 tiles, one
round - stays on gemm256f8 for every epilogue: the threshold between the two kernels. Its store pass for QuickGELU rows as e4m3
with MX block scales (GemmArgs::out_bscale) is held to torch's restatement of the MX quantiser on the bf16 rows the same launch
writes without it: test_gemm_fp8_persistent_mx_store."""
import ctypes as C
import functools

import pytest
import torch

import gemm_exact as ge
import row_exact as rx

pytestmark = pytest.mark.gpu

BOUND = 256          # |result| stays below it: integers that bf16 holds exactly (asserted, as test_gemm256p_race_screen does)


@functools.lru_cache(maxsize=None)
def _case(form, M, N, K):
    """Operands of one (form, shape) and the exact products, computed once in f64 on the CPU and shared by its epilogues."""
    g = torch.Generator(device="cpu"); g.manual_seed(M * 5 + N + K + {"bf16": 0, "fp8": 1, "bsa": 2}[form])
    a = torch.randint(-1, 2, (M, K), generator=g).float()
    w = (torch.rand(N, K, generator=g) < 0.05).float() * (torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1)
    c = dict(a=a, w=w, bias=torch.randint(-3, 4, (N,), generator=g).float(), res=torch.randint(-3, 4, (M, N), generator=g).float())
    # the stored FP8 operands are the integers divided by their power-of-two scales (exact in e4m3), so every form
    # computes the same integer matrix a w^T through differently scaled, still exact, partial sums
    pow2 = lambda *shape: torch.randint(-2, 3, shape, generator=g)          # noqa: E731
    if form == "fp8":
        c["sa"] = torch.exp2(pow2(M).float())
        c["a"] = a / c["sa"][:, None]
    if form == "bsa":
        e = pow2(M, K // 32)
        c["sb"] = torch.full(((M + 255) // 256 * 256, K // 32), 127, dtype=torch.uint8)          # rows padded to the tile
        c["sb"][:M] = (e + 127).to(torch.uint8)
        c["a"] = a / torch.exp2(e.float()).repeat_interleave(32, dim=1)
    if form != "bf16":
        c["sw"] = torch.exp2(pow2(N).float())
        c["w"] = w / c["sw"][:, None]
    c["acc"] = a.double() @ w.double().t()
    return c


def _run(clipmi, gpu, form, sel, M, N, K, epi):
    L = clipmi._lib.lib()
    c = _case(form, M, N, K)
    ref = c["acc"] + c["bias"].double() + (c["res"].double() if epi == 2 else 0)
    peak = ref.abs().max().item()
    print(f"{form} sel={sel} M={M} N={N} K={K} epi={epi}: max |result| {peak}")
    assert peak <= BOUND and torch.equal(ref.float().double(), ref)
    ref = ref.float().to(torch.bfloat16) if epi == 0 else ref.float()
    out = torch.full((M + 1, N), float("nan"), dtype=ref.dtype, device=gpu)          # +1 guard row
    if epi == 2:
        out[:M] = c["res"].to(gpu)
    bias = c["bias"].to(gpu)
    if form == "bf16":
        a, w = c["a"].to(torch.bfloat16).to(gpu), c["w"].to(torch.bfloat16).to(gpu)
        rc = L.clipmi_dbg_gemm_bf16(a.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, epi | (sel << 8), None)
    else:
        a8 = c["a"].to(torch.float8_e4m3fn).view(torch.uint8).to(gpu)
        w8 = c["w"].to(torch.float8_e4m3fn).view(torch.uint8).to(gpu)
        sw = c["sw"].to(gpu)
        if form == "fp8":
            sa = c["sa"].to(gpu)
            rc = L.clipmi_dbg_gemm_fp8(a8.data_ptr(), w8.data_ptr(), sa.data_ptr(), sw.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                       M, N, K, epi | (sel << 8), None)
        else:
            sb = c["sb"].to(gpu)
            rc = L.clipmi_dbg_gemm_fp8_bsa(a8.data_ptr(), w8.data_ptr(), sb.data_ptr(), sw.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                           M, N, K, epi, None)
    clipmi._lib.check(rc, f"gemm256 {form}")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.isnan(got[M]).all(), "wrote past row M"
    bad = got[:M] != ref
    assert not bad.any(), f"{form} sel={sel} M={M} N={N} K={K} epi={epi}: {bad.sum().item()} of {bad.numel()} differ, " \
                          f"max |diff| {(got[:M].double() - ref.double()).abs().max().item()}"


@pytest.mark.parametrize("M,N,K", [(300, 512, 256), (257, 256, 128)])
@pytest.mark.parametrize("epi", [0, 2, 3])
def test_gemm256_bf16_exact(clipmi, gpu, M, N, K, epi):
    """gemm256_bf16_nt_kernel, forced with algo 2."""
    _run(clipmi, gpu, "bf16", 2, M, N, K, epi)


@pytest.mark.parametrize("M,N,K", [(300, 512, 512), (257, 256, 256)])
@pytest.mark.parametrize("epi", [0, 2, 3])
@pytest.mark.parametrize("mx", [0, 2])
def test_gemm256f8_exact(clipmi, gpu, M, N, K, epi, mx):
    """gemm256f8_nt_kernel: mx = 0 the plain FP8 MFMA (bit 8 of the hook's epi), mx = 2 the scaled MFMA with unit block
    scales kept on the non-persistent kernel (bit 9)."""
    _run(clipmi, gpu, "fp8", 1 if mx == 0 else 2, M, N, K, epi)


@pytest.mark.parametrize("epi", [2, 3])
def test_gemm256f8_block_scaled_a_exact(clipmi, gpu, epi):
    """gemm256f8_nt_kernel<., true, true>: the e8m0 block scales reach the scaled MFMA as its per-lane scale operand."""
    _run(clipmi, gpu, "bsa", 0, 300, 512, 512, epi)


# ---- the persistent FP8 kernel ---------------------------------------------------------------------------------------------------
GK_256P, GK_F8 = 2, 4            # GemmKernel of csrc/gemm_plan.hpp
P_SHAPES = [(32768, 512, 256), (32769, 512, 256), (32769, 512, 512), (4353, 3840, 256)]      # 3840: the widest N the kernel takes
# the kernel each (shape, epilogue) runs on at the default form: see the module docstring
P_KERNEL = {(s, e): GK_256P if e == 0 and s != P_SHAPES[0] else GK_F8 for s in P_SHAPES for e in (0, 2, 3)}


def _fp8_plan(clipmi, M, N, K, epi, out_bs=0):
    """clipmi_dbg_gemm_fp8_plan at mx = 1 -> (return code, number of parts, kernel of part 0, rows of part 0, query)"""
    out = (C.c_int32 * ge.N_PLAN)()
    rc = clipmi._lib.lib().clipmi_dbg_gemm_fp8_plan(M, N, K, epi, 1, 0, out_bs, out, ge.N_PLAN)
    return rc, out[0], out[2], out[1], out[22]


@functools.lru_cache(maxsize=1)
def _p_case(M, N, K, gpu):
    """The recipe of _case at the persistent kernel's sizes, operands and float64 references on the device; redrawn until
    neither reference has two equal rows or columns."""
    def make(seed):
        g = torch.Generator(device="cpu"); g.manual_seed(seed)
        a = torch.randint(-1, 2, (M, K), generator=g).float()
        w = (torch.rand(N, K, generator=g) < 0.05).float() * (torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1)
        bias = torch.randint(-3, 4, (N,), generator=g).float().to(gpu)
        res = torch.randint(-3, 4, (M, N), generator=g).float().to(gpu)
        sa = torch.exp2(torch.randint(-2, 3, (M,), generator=g).float())             # per row: a neighbour's a_scale is off by a power of two
        sw = torch.exp2(torch.randint(-2, 3, (N,), generator=g).float())
        a8, w8 = (a / sa[:, None]).to(torch.float8_e4m3fn), (w / sw[:, None]).to(torch.float8_e4m3fn)
        assert torch.equal(a8.float() * sa[:, None], a) and torch.equal(w8.float() * sw[:, None], w)
        ref = a.to(gpu).double() @ w.to(gpu).double().t() + bias.double()
        return dict(a8=a8.view(torch.uint8).to(gpu), w8=w8.view(torch.uint8).to(gpu), sa=sa.to(gpu), sw=sw.to(gpu), bias=bias, res=res,
                    ref=ref, ref2=ref + res.double())
    return ge.redraw(make, M * 5 + N + K + 3, lambda c: ge.is_distinct(c["ref"]) and ge.is_distinct(c["ref2"]))


@pytest.mark.parametrize("M,N,K", P_SHAPES)
def test_gemm_fp8_exact_at_persistent_shapes(clipmi, gpu, M, N, K):
    """Epilogues 0, 2 and 3 of the default FP8 form equal float64; the plan is one part on the kernel P_KERNEL names."""
    L = clipmi._lib.lib()
    c = _p_case(M, N, K, gpu)
    for epi in (0, 2, 3):
        what = f"fp8 M={M} N={N} K={K} epi={epi}"
        rc, nparts, kernel, rows, _ = _fp8_plan(clipmi, M, N, K, epi)
        assert (rc, nparts, kernel, rows) == (0, 1, P_KERNEL[(M, N, K), epi], M), f"{what}: plan {(rc, nparts, kernel, rows)}"
        ref = c["ref2"] if epi == 2 else c["ref"]
        ge.assert_exact_reference(ref, what)
        ref = ref.float().to(torch.bfloat16) if epi == 0 else ref.float()
        out = torch.full((M + 1, N), float("nan"), dtype=ref.dtype, device=gpu)          # +1 guard row
        if epi == 2:
            out[:M] = c["res"]
        rc = L.clipmi_dbg_gemm_fp8(c["a8"].data_ptr(), c["w8"].data_ptr(), c["sa"].data_ptr(), c["sw"].data_ptr(), c["bias"].data_ptr(),
                                   out.data_ptr(), M, N, K, epi, None)
        clipmi._lib.check(rc, what)
        torch.cuda.synchronize()
        assert torch.isnan(out[M]).all(), f"{what}: wrote past row M"
        bad = out[:M] != ref
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} differ, max |diff| {(out[:M].double() - ref.double()).abs().max().item()}, " \
                              f"first at (row, column) {tuple(bad.nonzero()[0].tolist())}"


@functools.lru_cache(maxsize=1)
def _mx_case(M, N, K, gpu):
    """QuickGELU rows whose magnitudes differ by 32-column block: the channel scales are 2^e, e spread over -6 .. 6 per block (the
    e4m3 weights stay +-1), the bias integers times 2^e; one block has zero weights and zero bias."""
    g = torch.Generator(device="cpu"); g.manual_seed(M + N + K + 4)
    nb = N // 32
    a = torch.randint(-1, 2, (M, K), generator=g).float()
    w = (torch.rand(N, K, generator=g) < 0.05).float() * (torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1)
    e = ((torch.arange(nb) * 5) % 13 - 6)[torch.randperm(nb, generator=g)].float()
    zero = nb // 2 + 1
    sw = torch.exp2(e).repeat_interleave(32)
    bias = torch.randint(-3, 4, (N,), generator=g).float() * sw
    w[32 * zero:32 * zero + 32] = 0
    bias[32 * zero:32 * zero + 32] = 0
    sa = torch.exp2(torch.randint(-2, 3, (M,), generator=g).float())
    a8 = (a / sa[:, None]).to(torch.float8_e4m3fn)
    assert torch.equal(a8.float() * sa[:, None], a) and e.unique().numel() == min(nb, 13)
    pre = (a.to(gpu).double() @ w.to(gpu).double().t()) * sw.to(gpu).double() + bias.to(gpu).double()      # exact in f32 too
    assert torch.equal(pre.float().double(), pre)
    return dict(pre=pre, a8=a8.view(torch.uint8).to(gpu), w8=w.to(torch.float8_e4m3fn).view(torch.uint8).to(gpu), sa=sa.to(gpu), sw=sw.to(gpu),
                bias=bias.to(gpu), zero=zero)


def _launch_mx(clipmi, c, out, bscale, M, N, K, epi=1):
    return clipmi._lib.lib().clipmi_dbg_gemm_fp8_mxout(c["a8"].data_ptr(), c["w8"].data_ptr(), c["sa"].data_ptr(), c["sw"].data_ptr(),
                                                       c["bias"].data_ptr(), out.data_ptr(), None if bscale is None else bscale.data_ptr(),
                                                       M, N, K, epi, None)


@pytest.mark.parametrize("M,N,K", [(32769, 512, 256), (4353, 3840, 256)])
def test_gemm_fp8_persistent_mx_store(clipmi, gpu, M, N, K):
    """Epilogue 1 with block-scale output: e4m3 rows N bytes apart + scale bytes, equal (up to +-0) to torch's MX quantiser of
    the bf16 rows the same launch writes without block-scale output; a guard row behind row M in both. Those bf16 rows are
    held to the float64 QuickGELU of the exact argument."""
    c = _mx_case(M, N, K, gpu)
    what = f"fp8 MX store M={M} N={N} K={K}"
    for out_bs in (0, 1):
        rc, nparts, kernel, rows, query = _fp8_plan(clipmi, M, N, K, 1, out_bs)
        assert (rc, nparts, kernel, rows, query) == (0, 1, GK_256P, M, 1), f"{what}: plan {(rc, nparts, kernel, rows, query)}"
    rows = torch.full((M + 1, N), float("nan"), dtype=torch.bfloat16, device=gpu)
    clipmi._lib.check(_launch_mx(clipmi, c, rows, None, M, N, K), what)
    out8 = torch.full((M + 1, N), rx.GUARD_BYTE, dtype=torch.uint8, device=gpu)
    sb = torch.full((M + 1, N // 32), rx.GUARD_BYTE, dtype=torch.uint8, device=gpu)
    clipmi._lib.check(_launch_mx(clipmi, c, out8, sb, M, N, K), what)
    torch.cuda.synchronize()
    assert torch.isnan(rows[M]).all() and (out8[M] == rx.GUARD_BYTE).all() and (sb[M] == rx.GUARD_BYTE).all(), f"{what}: wrote past row M"
    # the bf16 rows themselves against float64: the argument is exact, and where |x| <= 32 quick_gelu4 is within 2^-16 |ref| plus
    # the bf16 store's 2^-8 |ref| (gemm_exact.run_plain_qgelu); beyond, the rounding of the exponent's argument grows with |x|
    ref = ge.qgelu64(c["pre"])
    near = c["pre"].abs() <= 32
    err, tol = (rows[:M].double() - ref).abs(), (2.0 ** -8 + 2.0 ** -16) * ref.abs()
    assert torch.isfinite(rows[:M].float()).all() and near.float().mean().item() > 0.25
    assert (err <= tol)[near].all(), f"{what}: bf16 rows, worst err / bound {(err / tol.clamp_min(1e-300))[near].max().item()}"
    print(f"{what}: bf16 rows at |x| <= 32, worst err / bound {(err / tol.clamp_min(1e-300))[near].max().item():.3f}")
    want8, want_sb = rx.quant_mx(rows[:M].cpu())
    assert want_sb[0].unique().numel() >= 6 and (want_sb[:, c["zero"]] == 127).all(), f"{what}: the data"
    assert (want_sb != rx.GUARD_BYTE).all()
    assert torch.equal(sb[:M].cpu(), want_sb), f"{what}: {int((sb[:M].cpu() != want_sb).sum())} scale bytes differ"
    rx.assert_e4m3_equal(out8[:M].cpu(), want8, what)


def test_gemm_fp8_mx_store_refused_off_the_persistent_kernel(clipmi, gpu):
    """Block-scale output exists for the persistent QuickGELU form only: the hook refuses where the plan does, and writes nothing."""
    for (M, N, K), epi in [((300, 512, 256), 1), ((32768, 512, 256), 1), ((32769, 512, 256), 0)]:
        rc, _, _, _, query = _fp8_plan(clipmi, M, N, K, epi, 1)
        assert rc == rx.EINVAL and "block-scale output" in clipmi._lib.last_error()
        assert query == (1 if M == 32769 else 0)
        a8 = torch.zeros(M, K, dtype=torch.uint8, device=gpu)
        w8 = torch.zeros(N, K, dtype=torch.uint8, device=gpu)
        c = dict(a8=a8, w8=w8, sa=torch.ones(M, device=gpu), sw=torch.ones(N, device=gpu), bias=torch.zeros(N, device=gpu))
        out8 = torch.full((M + 1, 2 * N), rx.GUARD_BYTE, dtype=torch.uint8, device=gpu)
        sb = torch.full((M + 1, N // 32), rx.GUARD_BYTE, dtype=torch.uint8, device=gpu)
        assert _launch_mx(clipmi, c, out8, sb, M, N, K, epi) == rx.EINVAL and "block-scale output" in clipmi._lib.last_error()
        torch.cuda.synchronize()
        assert (out8 == rx.GUARD_BYTE).all() and (sb == rx.GUARD_BYTE).all()
