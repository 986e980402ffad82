// gemm_plan.hpp — which kernel a GEMM runs on, as pure host functions of its shape. No HIP in here: gemm.hip
// launches what these say, encode.hip asks them where producer and consumer must agree on a buffer's format, tests/test_gemm_plan.py pins them.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include "../../include/clipmi.h"

namespace clipmi {

enum Epilogue {
    EPI_BIAS_BF16 = 0,        // out bf16 [M][N] = acc + bias
    EPI_BIAS_QGELU_BF16 = 1,  // out bf16 = quick_gelu(acc + bias)
    EPI_BIAS_RESID_F32 = 2,   // out f32 [M][N] += acc + bias        (residual stream, in place)
    EPI_F32 = 3,              // out f32 = acc (+ bias if given)
    EPI_PATCH_F32 = 4,        // out f32 [b*L + 1 + p][n] = acc + pos[1 + p][n],  m = b*np + p
    // LayerNorm folded into the GEMM that consumes it ("LN-folded" linear layers, see ln_fold in gemm.hpp):
    EPI_LN_BIAS_BF16 = 5,        // out bf16 = rstd[m] * (acc - mean[m] * colsum[n]) + bias[n]
    EPI_LN_BIAS_QGELU_BF16 = 6,  // out bf16 = quick_gelu(the same)
    EPI_BIAS_RESID_LN_F32 = 7,   // split residual: x3 (hi | lo rows) += acc + bias, + row-statistics partials of the new rows
    EPI_BIAS_RESID_LN8 = 8       // FP8 towers with folded LayerNorms: out f32 [M][N] += acc + bias, and the new rows also leave as e4m3
                                 // with MX block scales (x8, x8_bs: A of the next LN-folded FP8 GEMM) + statistics partials (ln_part)
};
constexpr bool epi_is_ln(int e) { return e == EPI_LN_BIAS_BF16 || e == EPI_LN_BIAS_QGELU_BF16; }
constexpr bool epi_is_qgelu(int e) { return e == EPI_BIAS_QGELU_BF16 || e == EPI_LN_BIAS_QGELU_BF16; }
constexpr bool epi_is_bf16_out(int e) { return e == EPI_BIAS_BF16 || e == EPI_BIAS_QGELU_BF16 || epi_is_ln(e); }

// The epilogues each kernel family instantiates, bit e = Epilogue e (with_epi in gemm.hip instantiates these, the plan refuses the rest)
constexpr unsigned EPI_MASK_128 = 0x7f, EPI_MASK_256 = 0x7f;     // everything but the split-residual producers
constexpr unsigned EPI_MASK_256P = 0xe7, EPI_MASK_SKINNY = 0xff; // persistent: the pure-store epilogues 0, 1, 2, 5, 6, 7
constexpr unsigned EPI_MASK_FP8 = 0x0f;                          // gemm256f8, row-scaled A; of these on the persistent kernel:
constexpr unsigned EPI_MASK_FP8_256P = 0x03;                     // (its residual form does not fit 256 registers)
#ifdef CLIPMI_DEV
constexpr unsigned EPI_MASK_FP8_BSA = 0x16c;                     // gemm256f8, block-scaled A: 2, 3 + the folded-LayerNorm FP8 tower's 5, 6, 8
#else
constexpr unsigned EPI_MASK_FP8_BSA = 0x00c;
#endif
constexpr bool epi_in(unsigned mask, int e) { return e >= 0 && e < 32 && ((mask >> e) & 1u) != 0; }

namespace plan_chip {       // (gemm.hip ties these to the kernels' own constants with static_asserts)
constexpr int NUM_CU = 256, LDS_BYTES = 160 * 1024, G256_LDS = 128 * 1024, G256P_MAX_N = 8192, FP8_BSA_MAX_K = 4096;
}
constexpr int SKINNY_MAX_M = 128;       // rows up to which the skinny kernels (gemm_skinny.hpp) take a GEMM

// LDS of the persistent kernel beyond the two K-tile buffers: bias[N]; FP8: w_scale[N] + the tile's 256 a_scale values
// (1 KiB); LN consumer: the tile's 256 colsum values (1 KiB) + K/256 statistics pairs per row (+ 8 B where the 4-pair read
// of the last row runs past them)
constexpr int g256p_lds(int epi, bool fp8, int N, int K, int dbg) {
    const int nseg = K >> 8;
    return plan_chip::G256_LDS + N * 4 * (fp8 ? 2 : 1) +
           (fp8 ? 1024 : epi_is_ln(epi) ? 1024 + 256 * nseg * 8 + (nseg < 4 ? 8 : 0) : 0) + ((dbg & 12) ? 8192 + 2048 : 0);
}

// Development knobs (CLIPMI_GEMM_*; read once through dev_knob in gemm.hip, these defaults in the product library)
struct GemmKnobs {
    int persist = 1;                   // PERSIST: 0 keeps every GEMM off the persistent kernel, 2 keeps the pre-round-5 rule
    int split = 40;                    // SPLIT=<pct>: split off the last round when it is less than pct % full (0: never)
    int skinny = 1;                    // SKINNY=0: no skinny kernel
    int grid = plan_chip::NUM_CU;      // GRID: fewer workgroups than CUs for the persistent kernel
};

enum GemmKernel { GK_128 = 0, GK_256 = 1, GK_256P = 2, GK_SKINNY = 3, GK_F8 = 4, GK_F8_BSA = 5 };     // 0-2 are GemmProbe::kernel_of's

// One launch of a plan: `rows` rows of the GEMM, in order. epi is the epilogue the kernel is instantiated with.
struct GemmPart {
    int rows, kernel, epi;
    bool scratch;        // EPI_BIAS_RESID_LN_F32 off the persistent kernel: an EPI_F32 launch into the f32 scratch rows + split_stats (add)
    bool leaves;         // the skinny residual producer updates the split rows itself and writes statistics leaves
    int grid, lds;       // GK_256P only
};
struct GemmPlan {
    int err = 0;         // a refusal: CLIPMI_E* and msg (written by refuse only)
    int nparts = 0;      // > 1: a split GEMM: part[0].rows = rows_main, every part but the last on the persistent kernel
    GemmPart part[3];
    char msg[224];
    GemmPlan& refuse(int code, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
        va_list ap; va_start(ap, fmt); vsnprintf(msg, sizeof(msg), fmt, ap); va_end(ap);
        err = code; return *this;
    }
    GemmPlan& add(int rows, int kernel, int epi, bool scratch = false, bool leaves = false, int grid = 0, int lds = 0) {
        part[nparts++] = GemmPart{rows, kernel, epi, scratch, leaves, grid, lds}; return *this;
    }
};

inline long long tiles256(int M, int N) { return (long long)(N / 256) * (((long long)M + 255) / 256); }
inline int g256p_grid(long long tiles, const GemmKnobs& kn) { return (int)(tiles < kn.grid ? tiles : kn.grid); }

// algo: 0 = choose by shape, 1 = force the 128x128 kernel, 2 = force the 256x256 kernel, 3 = force the persistent 256x256
// kernel. leaf / leaf_in: GemmArgs::ln_leaf / ln_leaf_in are set; dbg: GemmArgs::dbg (bits 2-3 cost the persistent kernel LDS).
inline GemmPlan gemm_plan(int M, int N, int K, int epi, int algo, bool leaf, bool leaf_in, int dbg, const GemmKnobs& kn = GemmKnobs()) {
    GemmPlan p;
    if (epi_is_ln(epi) && (K % 256 != 0 || K > 1024))
        return p.refuse(CLIPMI_EINVAL, "gemm: LN-folded epilogue %d needs ln_part_in, colsum, bias and K %% 256 == 0, K <= 1024", epi);
    if (epi == EPI_BIAS_RESID_LN_F32 && (N % 256 != 0 || N > 1024))
        return p.refuse(CLIPMI_EINVAL, "gemm: EPI_BIAS_RESID_LN_F32 needs x3 (16-byte aligned), ln_part, tmp_f32 and N %% 256 == 0, N <= 1024");
    if (algo == 5)
        return p.refuse(CLIPMI_EUNSUPPORTED, "algo 5 (W-direct gemm256, DESIGN 4.4h) was removed: measured 33-40 %% slower in round 4, commit 9acf8e2 last carried it");
#ifndef CLIPMI_DEV
    if (algo == 4) return p.refuse(CLIPMI_EUNSUPPORTED, "algo %d exists in the development build only (libclipmi_dev.so)", algo);
#else
    if (algo == 4) return p.refuse(CLIPMI_EUNSUPPORTED, "algo 4 (gemm2w, DESIGN 4.4g) was removed in round 5: measured slower in round 3, its sources are in the history");
#endif
    const bool ok256 = N % 256 == 0 && K % 64 == 0 && K >= 128;
    if (algo == 2 && !ok256) return p.refuse(CLIPMI_EINVAL, "gemm256: N=%d K=%d (need N %% 256 == 0, K %% 64 == 0, K >= 128)", N, K);
    const bool ok256p = ok256 && K % 128 == 0 && N <= plan_chip::G256P_MAX_N && epi_in(EPI_MASK_256P, epi) && K <= (1 << 20) &&
                        g256p_lds(epi, false, N, K, dbg) <= plan_chip::LDS_BYTES;
    if (algo == 3 && !ok256p)
        return p.refuse(CLIPMI_EINVAL, "gemm256p: M=%d N=%d K=%d epi=%d (need N %% 256 == 0, K %% 128 == 0, a store-only epilogue "
                        "and bias/colsum rows that fit LDS)", M, N, K, epi);
    const int lds_p = ok256p ? g256p_lds(epi, false, N, K, dbg) : 0;
    // by shape: the 256x256 pipeline wins when its tiles fill the 256 CUs in whole rounds (r01 on MI355X,
    // M=25600: N=2304/3072 -> 781/841 TF vs 702/685; N=768 -> 300 tiles = 1.17 rounds, 408/769 vs 521/904)
    bool use256 = algo == 2 || algo == 3, use256p = algo == 3;
    while (algo == 0 && ok256 && M >= 1024) {
        const long long tiles = tiles256(M, N);
        const long long rounds = (tiles + plan_chip::NUM_CU - 1) / plan_chip::NUM_CU;
        // calibrated with tools/gemm_rule.py: the 256x256 kernel wins from ~0.74-0.78 fill of its rounds
        // (earlier for long K, where its mainloop advantage outweighs the idle CUs of the last round)
        const long long pct = K >= 2048 ? 72 : 78;
        use256 = tiles * 100 >= rounds * plan_chip::NUM_CU * pct;
        // more than one round of tiles: the persistent kernel overlaps each tile's write-out with the next tile's K-loop (the
        // split-residual producer also at <= one round: its fused store pass saves the split_stats pass; PERSIST=2: the old rule)
        use256p = use256 && ok256p && kn.persist != 0 && (tiles > plan_chip::NUM_CU || (epi == EPI_BIAS_RESID_LN_F32 && kn.persist != 2));
        // A ragged last round (M = 25600 at N = 768: 300 tiles = 1.17 rounds; 78 k images/s at B = 512 against 102 k at 435 / 870):
        // the rows that fill WHOLE rounds of 256 x 256 tiles go to the persistent kernel, the remaining row tiles to whatever the
        // rule picks for them alone (128 x 128 tiles: a quarter of a big tile's time per round), instead of the whole GEMM falling
        // back. Same bits either way (every kernel's rows are independent). Not for the patch GEMM (its epilogue maps the absolute row).
        if (!(ok256p && kn.persist != 0 && tiles > plan_chip::NUM_CU && epi != EPI_PATCH_F32 && (tiles % plan_chip::NUM_CU) != 0 &&
              (tiles % plan_chip::NUM_CU) * 100 < (long long)plan_chip::NUM_CU * kn.split))
            break;
        const long long main_tiles = (tiles / plan_chip::NUM_CU) * plan_chip::NUM_CU;                      // whole rounds
        const long long rows_main = main_tiles / (N / 256) * 256;                    // < M: the last round was ragged
        // (at most two splits: the rows left over hold fewer than 0.4 x 256 + N / 256 tiles, part[] has room for any knob)
        if (rows_main < 256 || rows_main >= M || p.nparts == 2) break;
        p.add((int)rows_main, GK_256P, epi, false, false, g256p_grid(tiles256((int)rows_main, N), kn), lds_p);
        M -= (int)rows_main;
        use256 = use256p = false;        // the rest is planned on its own
    }
    if (M < 1) return p.refuse(CLIPMI_EINVAL, "gemm: bad arguments");
    const char* leaf_in_err = "gemm: ln_leaf_in is read by the skinny LN-folded consumers only (M <= %d)";
    if (leaf_in && p.nparts) return p.refuse(CLIPMI_EINVAL, leaf_in_err, SKINNY_MAX_M);     // (the persistent parts are no skinny consumers)
    // a handful of rows (one prompt, one image): the skinny kernel, whatever the epilogue
    const bool skinny = algo == 0 && kn.skinny != 0 && M <= SKINNY_MAX_M && N % 16 == 0 && K % 32 == 0 && K >= 32;
    // with a leaf buffer its residual producer updates the split rows itself and leaves statistics leaves (no scratch, no split_stats)
    const bool leaves = skinny && epi == EPI_BIAS_RESID_LN_F32 && leaf;
    if (!(skinny && (epi != EPI_BIAS_RESID_LN_F32 || leaves)) && leaf_in)
        return p.refuse(CLIPMI_EINVAL, leaf_in_err, SKINNY_MAX_M);
    // EPI_BIAS_RESID_LN_F32 off the persistent kernel: acc + bias as f32 into the scratch rows, then split_stats
    const bool scratch = epi == EPI_BIAS_RESID_LN_F32 && !use256p && !leaves;
    const int ran = scratch ? (int)EPI_F32 : epi;
    const int kernel = skinny ? GK_SKINNY : use256p ? GK_256P : use256 ? GK_256 : GK_128;
    if (kernel == GK_SKINNY && !epi_in(EPI_MASK_SKINNY, ran)) return p.refuse(CLIPMI_EINVAL, "gemm_skinny: epilogue %d", ran);
    if (kernel == GK_128 && (N < 1 || K < 1 || N % 128 != 0 || K % 64 != 0))
        return p.refuse(CLIPMI_EINVAL, "gemm: M=%d N=%d K=%d (need N %% 128 == 0, K %% 64 == 0)", M, N, K);
    if ((kernel == GK_128 || kernel == GK_256) && !epi_in(kernel == GK_128 ? EPI_MASK_128 : EPI_MASK_256, ran))
        return p.refuse(CLIPMI_EINVAL, "gemm: unknown epilogue %d", ran);
    return kernel == GK_256P ? p.add(M, kernel, ran, false, false, g256p_grid(tiles256(M, N), kn), lds_p)
                             : p.add(M, kernel, ran, scratch, leaves);
}

// launch_gemm_fp8 (e4m3 operands). mx: 1 = the block-scaled MFMA form with unit scales (twice the rate), 0 = plain FP8 MFMA, 2 = the
// MX form kept off the persistent kernel (tests). bsa / out_bs: GemmArgs::a_bscale / out_bscale are set; dbg: as in gemm_plan.
inline GemmPlan gemm_fp8_plan(int M, int N, int K, int epi, int mx, bool bsa, bool out_bs, int dbg = 0, const GemmKnobs& kn = GemmKnobs()) {
    GemmPlan p;
    if (M < 1 || N % 256 != 0 || K % 128 != 0 || K < 256)
        return p.refuse(CLIPMI_EINVAL, "gemm_fp8: M=%d N=%d K=%d (need N %% 256 == 0, K %% 128 == 0, K >= 256)", M, N, K);
    if (bsa) {            // MX activations: per-32-block e8m0 scales instead of a row scale
        if (K > plan_chip::FP8_BSA_MAX_K) return p.refuse(CLIPMI_EINVAL, "gemm_fp8: block-scaled A needs K <= %d", plan_chip::FP8_BSA_MAX_K);
        if (!epi_in(EPI_MASK_FP8_BSA, epi)) return p.refuse(CLIPMI_EINVAL, "gemm_fp8: block-scaled A with epilogue %d", epi);
        // (development library, DESIGN 4.4c: the FP8 tower with folded LayerNorms - its residual producer and LN-folded consumers)
        if (epi == EPI_BIAS_RESID_LN8 && N > 1024)
            return p.refuse(CLIPMI_EINVAL, "gemm_fp8: EPI_BIAS_RESID_LN8 needs x8, x8_bs, ln_part and N <= 1024");
        if (epi_is_ln(epi) && (K % 256 != 0 || K > 1024))
            return p.refuse(CLIPMI_EINVAL, "gemm_fp8: LN-folded epilogue %d needs ln_part_in, colsum, bias, K %% 256 == 0, K <= 1024", epi);
        if (epi_is_ln(epi) && out_bs && epi != EPI_LN_BIAS_QGELU_BF16)
            return p.refuse(CLIPMI_EINVAL, "gemm_fp8: e4m3 + block-scale output exists for the QuickGELU forms only");
        return p.add(M, GK_F8_BSA, epi);
    }
    // more than one round of tiles: the persistent role-split kernel on FP8 operands (mx = 2 keeps gemm256f8 for tests)
    const long long tiles = tiles256(M, N);
    const bool persist = mx == 1 && tiles > plan_chip::NUM_CU && K % 256 == 0 && N <= 3840 && kn.persist != 0 && epi_in(EPI_MASK_FP8_256P, epi);
    if (out_bs && !(persist && epi == EPI_BIAS_QGELU_BF16))
        return p.refuse(CLIPMI_EINVAL, "gemm_fp8: e4m3 + block-scale output exists for the persistent QuickGELU form only");
    if (persist) {
        const int lds = g256p_lds(epi, true, N, K, dbg);
        if (lds > plan_chip::LDS_BYTES) return p.refuse(CLIPMI_EUNSUPPORTED, "gemm256p: %d B of LDS for N=%d", lds, N);
        return p.add(M, GK_256P, epi, false, false, g256p_grid(tiles, kn), lds);
    }
    if (!epi_in(EPI_MASK_FP8, epi)) return p.refuse(CLIPMI_EINVAL, "gemm_fp8: epilogue %d", epi);
    return p.add(M, GK_F8, epi);
}

}  // namespace clipmi
