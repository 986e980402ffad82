"""-m gpu: the non-persistent 256-tile GEMM (gemm256.hpp: one schedule and epilogue, expanded for bf16, FP8 and FP8 with
block-scaled A) on EXACT data, for the forms that no other test pins bit for bit: the f32 epilogues, the plain FP8 MFMA
form and block-scaled A. (The bf16-out forms of gemm256 and the MX form of gemm256f8 are also pinned against the persistent
kernel in test_kernels_gpu.py / test_fp8_gpu.py; QuickGELU is not exact and stays there.)

A is dense in {-1, 0, 1}, W 5 % dense in {-1, 1}, bias and residual are small integers, the FP8 row / channel / block
scales are powers of two in 2^-2 .. 2^2 (the e4m3 bytes hold the integers divided by them): every product, partial sum,
scaling and add is exact in f32 and every result an integer that bf16 holds, so the output must EQUAL torch's - a stale
or early LDS read anywhere in the DMA pipeline shows as a wrong integer. Shapes: an M-edge tile with four K-tiles (both A halves, both LDS buffers reused) and the
smallest K each form accepts (two K-tiles: the steady-state loop body runs once)."""
import functools

import pytest
import torch

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
