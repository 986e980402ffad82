// gemm.hip — instantiation and launch of the bf16 NT GEMM (see gemm.hpp). Which kernel a GEMM runs on: gemm_plan.hpp.
#include "gemm256p.hpp"
#include "gemm_skinny.hpp"
#include "gemm256f8.hpp"
#include <hip/hip_ext.h>
#include <cstdlib>
#include <type_traits>

namespace clipmi {

static_assert(plan_chip::NUM_CU == NUM_CU && plan_chip::LDS_BYTES == LDS_BYTES && plan_chip::G256_LDS == G256_LDS &&
              plan_chip::G256P_MAX_N == G256P_MAX_N, "gemm_plan.hpp restates these for host-only builds");

static const GemmKnobs& knobs() {        // development switches for A/B runs on one box
    static const GemmKnobs kn{(int)dev_knob("CLIPMI_GEMM_PERSIST", 1), (int)dev_knob("CLIPMI_GEMM_SPLIT", 40),
                              (int)dev_knob("CLIPMI_GEMM_SKINNY", 1), (int)dev_knob("CLIPMI_GEMM_GRID", NUM_CU)};
    return kn;
}

// f(std::integral_constant<int, EPI>) for the runtime `epi`, instantiated for the epilogues in MASK (EPI_MASK_*) only; the plans refuse the others
template <unsigned MASK, int E = 0, typename F>
static int with_epi(int epi, F&& f) {
    if constexpr (E <= EPI_BIAS_RESID_LN8) {
        if constexpr (epi_in(MASK, E))
            if (epi == E) return f(std::integral_constant<int, E>{});
        return with_epi<MASK, E + 1>(epi, f);
    }
    return set_err(CLIPMI_EINVAL, "gemm: epilogue %d is not built for this kernel", epi);
}

// probe: nullptr, or the measurement probe that wants this launch (its events take the dispatch's own begin / end stamps)
template <typename Kernel>
static void launch_probed(Kernel kernel, dim3 grid, dim3 block, int lds, hipStream_t st, GemmProbe* probe, int epi, int kernel_kind,
                          int K, const GemmArgs& g) {
    const int i = probe ? probe->begin(epi, kernel_kind, st, K) : 0;
    if (probe) hipExtLaunchKernelGGL(kernel, grid, block, lds, st, probe->ev[2 * i], probe->ev[2 * i + 1], 0, g);
    else hipLaunchKernelGGL(kernel, grid, block, lds, st, g);
}

// LDS opt-in (hipFuncSetAttribute) is remembered per (kernel, device): a second device in the same thread gets its own
static bool lds_opted(int* slots) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) return false;
    if (slots[dev]) return true;
    slots[dev] = 1;
    return false;
}

// The 512-thread kernels (gemm256.hpp, gemm256p.hpp, gemm256f8.hpp). KERNEL keys the LDS opt-in slots: `lds_max` is opted in
// once per instantiation and device, `lds` is this launch's. opt_err / name: the texts of a failed opt-in and of a failed launch.
template <auto KERNEL>
static int launch_g256(const GemmArgs& g, int grid, hipStream_t st, int lds_max, int lds, const char* opt_err, const char* name,
                       GemmProbe* probe = nullptr, int epi = 0, int kernel_kind = GK_256) {
    static thread_local int opted[64];
    if (!lds_opted(opted) &&
        hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) != hipSuccess)
        return set_err(CLIPMI_EHIP, opt_err, lds_max);
    launch_probed(KERNEL, dim3(grid), dim3(512), lds, st, probe, epi, kernel_kind, g.K, g);
    CLIPMI_CHECK_LAUNCH(name);
    return 0;
}
static int grid256(const GemmArgs& g) { return (g.N / 256) * ((g.M + 255) / 256); }      // one workgroup per tile

// skinny kernel (gemm_skinny.hpp): M <= 128 rows, one wave per 16 columns x 16 rows
template <int EPI>
static int launch_skinny(const GemmArgs& g, hipStream_t st) {
    const int nstrips = g.N / 16, mtiles = (g.M + 15) / 16;
    const int waves = nstrips * mtiles <= 4 * NUM_CU ? 1 : 4;       // one wave per workgroup until every CU has four
    const dim3 grid((nstrips + waves - 1) / waves, mtiles);
    if (g.K > 512) hipLaunchKernelGGL((gemm_skinny_kernel<EPI, 32>), grid, dim3(waves * 64), 0, st, g);
    else hipLaunchKernelGGL((gemm_skinny_kernel<EPI, 16>), grid, dim3(waves * 64), 0, st, g);
    CLIPMI_CHECK_LAUNCH("gemm_skinny_kernel");
    return 0;
}

// one part of a plan, on the kernel and with the epilogue the plan names
static int launch_part(const GemmArgs& g, const GemmPart& part, hipStream_t st, GemmProbe* probe) {
    switch (part.kernel) {
        case GK_SKINNY:
            return with_epi<EPI_MASK_SKINNY>(part.epi, [&](auto e) { return launch_skinny<decltype(e)::value>(g, st); });
        case GK_128:
            return with_epi<EPI_MASK_128>(part.epi, [&](auto e) {
                constexpr int EPI = decltype(e)::value;
                launch_probed(gemm_bf16_nt_kernel<EPI>, dim3((g.N / GEMM_BN) * ((g.M + GEMM_BM - 1) / GEMM_BM)), dim3(256), GEMM_LDS_BYTES, st, probe, EPI, GK_128, g.K, g);
                CLIPMI_CHECK_LAUNCH("gemm_bf16_nt_kernel");
                return 0;
            });
        case GK_256:
            return with_epi<EPI_MASK_256>(part.epi, [&](auto e) {
                constexpr int EPI = decltype(e)::value;
                return launch_g256<gemm256_bf16_nt_kernel<EPI>>(g, grid256(g), st, G256_LDS, G256_LDS, "hipFuncSetAttribute(gemm256, %d B LDS)",
                                                                "gemm256_bf16_nt_kernel", probe, EPI);
            });
        default:            // GK_256P: persistent, role-split (gemm256p.hpp), pure-store epilogues only
            return with_epi<EPI_MASK_256P>(part.epi, [&](auto e) {
                constexpr int EPI = decltype(e)::value;
                return launch_g256<gemm256p_bf16_nt_kernel<EPI, false>>(g, part.grid, st, LDS_BYTES, part.lds, "hipFuncSetAttribute(gemm256p, %d B LDS)",
                                                                        "gemm256p_bf16_nt_kernel", probe, EPI, GK_256P);
            });
    }
}

// the arguments of `rows` rows of g from row `row0` on: a part of a split GEMM (every kernel's rows are independent)
static GemmArgs gemm_rows(const GemmArgs& g, int epi, int row0, int rows) {
    GemmArgs b = g;
    b.M = rows;
    b.A = g.A + (size_t)row0 * gemm_lda(g);
    const size_t oe = (size_t)row0 * g.N;
    if (epi == EPI_BIAS_RESID_LN_F32) {
        b.x3 = static_cast<char*>(g.x3) + (size_t)row0 * resid_row_bytes(g.N); b.tmp_f32 = g.tmp_f32 + oe;
        b.ln_part = g.ln_part + (size_t)row0 * (g.N / 256) * 2;
    } else {
        b.out = static_cast<char*>(g.out) + oe * (epi_is_bf16_out(epi) ? 2 : 4);
    }
    if (b.ln_part_in) b.ln_part_in = g.ln_part_in + (size_t)row0 * (g.K / 256) * 2;
    return b;
}

bool gemm_resid_writes_leaves(int M, int N, int K) {
    const GemmPlan p = gemm_plan(M, N, K, EPI_BIAS_RESID_LN_F32, 0, true, false, 0, knobs());
    return !p.err && p.nparts == 1 && p.part[0].leaves;
}

// algo: gemm_plan's. EPI_BIAS_RESID_LN_F32 updates the split rows x3 and their statistics partials: the persistent kernel's storers do it
// on their way out, every other kernel writes acc + bias as f32 into g.tmp_f32 and split_stats_kernel (add) does the rest. Same bits.
int launch_gemm_algo(const GemmArgs& g, int epi, int algo, hipStream_t st, GemmProbe* probe) {
    if (epi_is_ln(epi) && ((!g.ln_part_in && !g.ln_leaf_in) || !g.colsum || !g.bias))
        return set_err(CLIPMI_EINVAL, "gemm: LN-folded epilogue %d needs ln_part_in, colsum, bias and K %% 256 == 0, K <= 1024", epi);
    if (epi == EPI_BIAS_RESID_LN_F32 && (!g.x3 || !g.ln_part || !g.tmp_f32 || ((size_t)g.x3 & 15) != 0))
        return set_err(CLIPMI_EINVAL, "gemm: EPI_BIAS_RESID_LN_F32 needs x3 (16-byte aligned), ln_part, tmp_f32 and N %% 256 == 0, N <= 1024");
    if (g.lda_bytes && (g.lda_bytes % 16 != 0 || g.lda_bytes < 2u * (unsigned)g.K))
        return set_err(CLIPMI_EINVAL, "gemm: lda_bytes %u (need a multiple of 16, >= 2 K)", g.lda_bytes);
    const GemmPlan plan = gemm_plan(g.M, g.N, g.K, epi, algo, g.ln_leaf != nullptr, g.ln_leaf_in != nullptr, g.dbg, knobs());
    if (plan.err) return set_err(plan.err, "%s", plan.msg);
    if (!g.A || !g.W || (!g.out && epi != EPI_BIAS_RESID_LN_F32)) return set_err(CLIPMI_EINVAL, "gemm: bad arguments");
    for (int i = 0, row0 = 0; i < plan.nparts; row0 += plan.part[i++].rows) {
        const GemmPart& part = plan.part[i];
        GemmArgs a = plan.nparts > 1 ? gemm_rows(g, epi, row0, part.rows) : g;
        if (part.scratch) a.out = a.tmp_f32;
        // (the probe brackets the GEMM launch itself: a scratch part's is an EPI_F32 launch standing in for the residual epilogue)
        if (int rc = launch_part(a, part, st, probe && probe->wants(epi) ? probe : nullptr)) return rc;
        if (part.scratch)
            if (int rc = launch_split_stats(a.tmp_f32, true, a.x3, a.ln_part, a.M, a.N, st)) return rc;
    }
    return 0;
}

// mx, and what runs: gemm_fp8_plan
int launch_gemm_fp8(const GemmArgs& g, int epi, hipStream_t st, int mx) {
    if (!g.A || !g.W || !g.out || (!g.a_scale && !g.a_bscale) || !g.w_scale) return set_err(CLIPMI_EINVAL, "gemm_fp8: NULL pointer");
    const bool bsa_epi = g.a_bscale && epi_in(EPI_MASK_FP8_BSA, epi);        // (epilogues 5, 6, 8: the development library's)
    if (bsa_epi && epi == EPI_BIAS_RESID_LN8 && (!g.x8 || !g.x8_bs || !g.ln_part))
        return set_err(CLIPMI_EINVAL, "gemm_fp8: EPI_BIAS_RESID_LN8 needs x8, x8_bs, ln_part and N <= 1024");
    if (bsa_epi && epi_is_ln(epi) && (!g.ln_part_in || !g.colsum || !g.bias))
        return set_err(CLIPMI_EINVAL, "gemm_fp8: LN-folded epilogue %d needs ln_part_in, colsum, bias, K %% 256 == 0, K <= 1024", epi);
    const GemmPlan plan = gemm_fp8_plan(g.M, g.N, g.K, epi, mx, g.a_bscale != nullptr, g.out_bscale != nullptr, g.dbg, knobs());
    if (plan.err) return set_err(plan.err, "%s", plan.msg);
    const GemmPart& part = plan.part[0];
    switch (part.kernel) {
        case GK_256P:       // more than one round of tiles: the persistent role-split kernel on FP8 operands
            return with_epi<EPI_MASK_FP8_256P>(epi, [&](auto e) {
                return launch_g256<gemm256p_bf16_nt_kernel<decltype(e)::value, true>>(g, part.grid, st, LDS_BYTES, part.lds, "hipFuncSetAttribute(gemm256p, %d B LDS)",
                                                                                      "gemm256p_bf16_nt_kernel");
            });
        case GK_F8_BSA:     // block-scaled A: the tile's 256 x K/32 scale bytes sit behind the K-tile buffers, 160 KiB of LDS at the largest K
            return with_epi<EPI_MASK_FP8_BSA>(epi, [&](auto e) {
                return launch_g256<gemm256f8_nt_kernel<decltype(e)::value, true, true>>(
                    g, grid256(g), st, G256_LDS + 256 * (plan_chip::FP8_BSA_MAX_K / 32), G256_LDS + 256 * (g.K / 32),
                    "hipFuncSetAttribute(gemm256f8 block-scaled)", "gemm256f8_nt_kernel(block-scaled A)");
            });
    }
    return with_epi<EPI_MASK_FP8>(epi, [&](auto e) {
        constexpr int EPI = decltype(e)::value;
        const char *opt_err = "hipFuncSetAttribute(gemm256f8, %d B LDS)", *name = "gemm256f8_nt_kernel";
        return mx ? launch_g256<gemm256f8_nt_kernel<EPI, true>>(g, grid256(g), st, G256_LDS, G256_LDS, opt_err, name)
                  : launch_g256<gemm256f8_nt_kernel<EPI, false>>(g, grid256(g), st, G256_LDS, G256_LDS, opt_err, name);
    });
}

// true when launch_gemm_fp8(.., EPI_BIAS_QGELU_BF16, ..) of this shape runs on the persistent kernel, whose store pass can
// emit e4m3 + MX block scales (GemmArgs::out_bscale) instead of bf16
bool gemm_fp8_emits_mx(int M, int N, int K) {
    const GemmPlan p = gemm_fp8_plan(M, N, K, EPI_BIAS_QGELU_BF16, 1, false, false, 0, knobs());
    return !p.err && p.part[0].kernel == GK_256P;
}

}  // namespace clipmi

using namespace clipmi;

// the operands every test hook below passes
static GemmArgs hook_args(const void* a, const void* w, const float* bias, void* out, int M, int N, int K) {
    GemmArgs g{};
    g.A = static_cast<const unsigned short*>(a); g.W = static_cast<const unsigned short*>(w); g.bias = bias; g.out = out;
    g.M = M; g.N = N; g.K = K;
    return g;
}

extern "C" int clipmi_dbg_gemm_bf16(const void* a_dev, const void* w_dev, const float* bias_dev, void* out_dev, int M,
                                    int N, int K, int epi, void* stream) {
    const int algo = (epi >> 8) & 7;      // test hook: bits 8-10 force a kernel (see gemm_plan)
    epi &= 0xff;
    if (epi < 0 || epi > 3) return set_err(CLIPMI_EINVAL, "dbg_gemm: epi %d", epi);
    GemmArgs g = hook_args(a_dev, w_dev, bias_dev, out_dev, M, N, K);
    static const int dbg_env = (int)dev_knob("CLIPMI_GEMM_DBG", 0);
    g.dbg = dbg_env;
    if (g.dbg & 12) { g.pos = bias_dev; g.bias = nullptr; }     // stamps land in the caller's "bias" buffer (>= 4 KiB)
    return launch_gemm_algo(g, epi, algo, as_stream(stream));
}

// Test hooks of the LN-folded layers (clipmi.h). `epi` = 5 or 6, bits 8-9 force a kernel as in clipmi_dbg_gemm_bf16.
extern "C" int clipmi_dbg_gemm_ln(const void* x3_dev, const void* wg_dev, const float* cb_dev, const float* colsum_dev,
                                  const float* part_dev, void* out_dev, int M, int N, int K, int epi, void* stream) {
    const int algo = (epi >> 8) & 3;
    epi &= 0xff;
    if (!epi_is_ln(epi)) return set_err(CLIPMI_EINVAL, "dbg_gemm_ln: epi %d", epi);
    GemmArgs g = hook_args(x3_dev, wg_dev, cb_dev, out_dev, M, N, K);       // the hi halves of the split rows are the A operand
    g.lda_bytes = (unsigned)resid_row_bytes(K); g.colsum = colsum_dev; g.ln_part_in = part_dev;
    return launch_gemm_algo(g, epi, algo, as_stream(stream));
}

// One prompt / one image (M <= 128, the skinny kernels): the residual producer that writes statistics leaves leaf_dev [M][N / 4][2]
// and the LN-folded consumer reading them; together the bits of clipmi_dbg_gemm_resid_ln + clipmi_dbg_gemm_ln.
extern "C" int clipmi_dbg_gemm_resid_ln_leaf(const void* a_dev, const void* w_dev, const float* bias_dev, void* x3_dev, float* leaf_dev,
                                             int M, int N, int K, void* stream) {
    if (!leaf_dev || !gemm_resid_writes_leaves(M, N, K))
        return set_err(CLIPMI_EINVAL, "dbg_gemm_resid_ln_leaf: M <= %d, N %% 256 == 0, N <= 1024, K %% 32 == 0", SKINNY_MAX_M);
    GemmArgs g = hook_args(a_dev, w_dev, bias_dev, nullptr, M, N, K);
    g.x3 = x3_dev; g.ln_leaf = leaf_dev;
    g.ln_part = leaf_dev; g.tmp_f32 = leaf_dev;          // unused on this path (the argument check wants them non-null)
    return launch_gemm_algo(g, EPI_BIAS_RESID_LN_F32, 0, as_stream(stream));
}

extern "C" int clipmi_dbg_gemm_ln_leaf(const void* x3_dev, const void* wg_dev, const float* cb_dev, const float* colsum_dev,
                                       const float* leaf_dev, void* out_dev, int M, int N, int K, int epi, void* stream) {
    if (!epi_is_ln(epi)) return set_err(CLIPMI_EINVAL, "dbg_gemm_ln_leaf: epi %d", epi);
    GemmArgs g = hook_args(x3_dev, wg_dev, cb_dev, out_dev, M, N, K);
    g.lda_bytes = (unsigned)resid_row_bytes(K); g.colsum = colsum_dev; g.ln_leaf_in = leaf_dev;
    return launch_gemm_algo(g, epi, 0, as_stream(stream));
}

// x3 (split residual rows, updated in place) += a @ w^T + bias; part = statistics partials of the new rows; tmp_dev: f32 [M][N]
// scratch. algo as in clipmi_dbg_gemm_bf16 (3 = the persistent kernel's fused store pass; 1 / 2 = GEMM into tmp + split_stats_kernel).
extern "C" int clipmi_dbg_gemm_resid_ln(const void* a_dev, const void* w_dev, const float* bias_dev, void* x3_dev,
                                        float* part_dev, float* tmp_dev, int M, int N, int K, int algo, void* stream) {
    GemmArgs g = hook_args(a_dev, w_dev, bias_dev, nullptr, M, N, K);
    g.x3 = x3_dev; g.ln_part = part_dev; g.tmp_f32 = tmp_dev;
    static const int dbg_env = (int)dev_knob("CLIPMI_GEMM_DBG", 0);
    g.dbg = dbg_env;
    return launch_gemm_algo(g, EPI_BIAS_RESID_LN_F32, algo & 7, as_stream(stream));
}

extern "C" int clipmi_dbg_gemm_fp8_bsa(const void* a8_dev, const void* w8_dev, const void* a_bscale_dev, const float* w_scale_dev,
                                       const float* bias_dev, void* out_dev, int M, int N, int K, int epi, void* stream) {
    GemmArgs g = hook_args(a8_dev, w8_dev, bias_dev, out_dev, M, N, K);
    g.a_bscale = static_cast<const unsigned char*>(a_bscale_dev); g.w_scale = w_scale_dev;
    return launch_gemm_fp8(g, epi, as_stream(stream), 1);
}

extern "C" int clipmi_dbg_gemm_fp8(const void* a8_dev, const void* w8_dev, const float* a_scale_dev, const float* w_scale_dev,
                                   const float* bias_dev, void* out_dev, int M, int N, int K, int epi, void* stream) {
    // test hook: bit 8 selects the plain (non-scaled) FP8 MFMA form, bit 9 keeps the MX form on the non-persistent kernel
    const int mx = (epi >> 8) & 1 ? 0 : ((epi >> 9) & 1 ? 2 : 1);
    epi &= 0xff;
    if (epi < 0 || epi > 3) return set_err(CLIPMI_EINVAL, "dbg_gemm_fp8: epi %d", epi);
    GemmArgs g = hook_args(a8_dev, w8_dev, bias_dev, out_dev, M, N, K);
    g.a_scale = a_scale_dev; g.w_scale = w_scale_dev;
    return launch_gemm_fp8(g, epi, as_stream(stream), mx);
}

// clipmi_dbg_gemm_fp8's default form (mx = 1) with GemmArgs::out_bscale: where the plan runs the persistent QuickGELU kernel the rows
// leave as e4m3, N bytes apart in out_dev, + MX scale bytes; every other shape or epilogue with out_bscale_dev set is refused
extern "C" int clipmi_dbg_gemm_fp8_mxout(const void* a8_dev, const void* w8_dev, const float* a_scale_dev, const float* w_scale_dev,
                                         const float* bias_dev, void* out_dev, void* out_bscale_dev, int M, int N, int K, int epi,
                                         void* stream) {
    if (epi < 0 || epi > 3) return set_err(CLIPMI_EINVAL, "dbg_gemm_fp8_mxout: epi %d", epi);
    GemmArgs g = hook_args(a8_dev, w8_dev, bias_dev, out_dev, M, N, K);
    g.a_scale = a_scale_dev; g.w_scale = w_scale_dev; g.out_bscale = static_cast<unsigned char*>(out_bscale_dev);
    return launch_gemm_fp8(g, epi, as_stream(stream), 1);
}

// The plans alone, host only. out[0] = nparts, then (rows, kernel, epi, scratch, leaves, grid, lds) per part, out[22] = `query`: what
// gemm_resid_writes_leaves / gemm_fp8_emits_mx answer for the shape; unused entries 0. A refusal: the return value + clipmi_last_error().
static int plan_out(const GemmPlan& p, bool query, int32_t* out, int n_out) {
    if (!out || n_out < 1) return set_err(CLIPMI_EINVAL, "dbg_gemm_plan: no output array");
    for (int i = 0; i < n_out; ++i) out[i] = i == 22 && query;
    if (p.err) return set_err(p.err, "%s", p.msg);
    out[0] = p.nparts;
    for (int i = 0; i < p.nparts; ++i) {
        const GemmPart& q = p.part[i];
        const int32_t f[7] = {q.rows, q.kernel, q.epi, q.scratch, q.leaves, q.grid, q.lds};
        for (int j = 0; j < 7 && 1 + 7 * i + j < n_out; ++j) out[1 + 7 * i + j] = f[j];
    }
    return 0;
}

extern "C" int clipmi_dbg_gemm_plan(int M, int N, int K, int epi, int algo, int ln_leaf, int ln_leaf_in, int dbg, int32_t* out, int n_out) {
    return plan_out(gemm_plan(M, N, K, epi, algo, ln_leaf != 0, ln_leaf_in != 0, dbg, knobs()), gemm_resid_writes_leaves(M, N, K), out, n_out);
}

extern "C" int clipmi_dbg_gemm_fp8_plan(int M, int N, int K, int epi, int mx, int a_bscale, int out_bscale, int32_t* out, int n_out) {
    return plan_out(gemm_fp8_plan(M, N, K, epi, mx, a_bscale != 0, out_bscale != 0, 0, knobs()), gemm_fp8_emits_mx(M, N, K), out, n_out);
}
