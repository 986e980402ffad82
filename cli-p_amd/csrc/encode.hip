// encode.hip — clipmi_encode_image / clipmi_encode_text: the two towers as kernel sequences on
// one stream. Replaces model.encode_image (reference build-index.py:49-50) and
// model.encode_text + normalize (query-index.py:108, 13-17). Op order follows SURVEY.md §2.1.
//
// Activation layout in HBM (all row-major, token row t = b*L + l):
//   ln_fold towers (bf16 weights, W % 256 == 0: every real CLIP tower; gemm.hpp "LN-folded linear layers"):
//     x3   [B*L][3 W bytes]    the residual stream, split (gemm.hpp split_make): a row is W bf16 hi = bf16(x) then W u8
//                              remainders (3 bytes per element since round 5); the hi halves are the A operand of the
//                              LN-folded qkv / c_fc GEMMs (row pitch 3 W), 12-24 residual adds keep ~2^-17 relative
//     ln_part f32 [B*L][W/256][2]  row statistics of x as per-256-column (sum, sum of squares)
//     x    f32  [B*L][W]       embedding-stage output only (and scratch of non-persistent residual GEMMs)
//   other towers (FP8 weights, toy widths):
//     x    f32  [B*L][W]       residual stream;  h also receives the LayerNorm outputs
//   h    bf16 [B*L][W]     attention output (GEMM A operand)
//   big  bf16 [B*L][4W]    qkv ([..][3W]) and, later in the layer, the MLP hidden ([..][4W])
//   patches bf16 [B*np][patch_k] (vision), pooled bf16 [B][W]
#include "vit_kernels.hpp"

namespace clipmi {
namespace {

struct Ws {
    unsigned short* patches;
    float* x;
    unsigned short* h;
    unsigned short* big;
    unsigned short* pooled;
    int* rowidx;
    unsigned char* a8;        // weight_format 1: the current GEMM's A operand as e4m3 [B*L][<= 4W]
    float* a_scale;           //                  and its row scales [B*L]
    unsigned char* a_bs;      //                  or (A produced by attention / QuickGELU) its MX block scales, rows padded to 256
    unsigned char* x8;        // weight_format 1 + ln_fold: the residual rows as e4m3 [B*L][W] (A operand of the LN-folded qkv / c_fc GEMMs)
    unsigned char* x8_bs;     //                            and their MX block scales, rows padded to 256
    void* x3;                 // ln_fold: the residual stream kept split, rows of [W bf16 hi | W u8 lo]; the hi halves are
                              //          also the A operand of the LN-folded qkv / c_fc GEMMs
    float* ln_part;           //          row statistics of x as per-256-column (sum, sum of squares) [B*L][W/256][2]
    float* ln_leaf;           //          <= 128 rows (one prompt, one image): the statistics as per-4-column leaves [B*L][W/4][2]
    // vision towers with bf16 weights: the class-token rows of the last block's tail (run_layers), compact
    void* x3c;                // ln_fold: the B class-token rows of x3, [B][3 W bytes]
    float* partc;             //          their statistics partials [B][W/256][2]
    float* leafc;             //          B <= 128: or their statistics leaves [B][W/4][2]
    float* xc;                // no ln_fold: the B class-token rows of x, f32 [B][W]
};

size_t carve(const clipmi_tower* t, int B, void* base, size_t cap, Ws* out) {
    Arena ar(base ? base : reinterpret_cast<void*>(256), cap);
    const size_t rows = (size_t)B * t->tokens;
    const int W = t->width;
    Ws w{};
    if (t->kind == 0) w.patches = ar.take<unsigned short>((size_t)B * (t->tokens - 1) * t->patch_k);
    w.x = ar.take<float>(rows * W);
    w.h = ar.take<unsigned short>(rows * W);
    w.big = ar.take<unsigned short>(rows * 4 * W);
    w.pooled = ar.take<unsigned short>((size_t)B * W);
    w.rowidx = ar.take<int>((size_t)B);
    if (t->weight_format == 1) {
        w.a8 = ar.take<unsigned char>(rows * 4 * W);
        w.a_scale = ar.take<float>(rows);
        w.a_bs = ar.take<unsigned char>((rows + 255) / 256 * 256 * (size_t)(4 * W / 32));
    }
    if (t->ln_fold && t->weight_format == 1) {
        // FP8 tower with folded LayerNorms: the residual stays f32 (w.x); its e4m3 image + statistics travel beside it
        w.x8 = ar.take<unsigned char>(rows * W);
        w.x8_bs = ar.take<unsigned char>((rows + 255) / 256 * 256 * (size_t)(W / 32));
        w.ln_part = ar.take<float>(rows * 2 * (W / 256));
    } else if (t->ln_fold) {
        w.x3 = ar.take<unsigned char>(rows * resid_row_bytes(W));
        w.ln_part = ar.take<float>(rows * 2 * (W / 256));
        if (rows <= (size_t)SKINNY_MAX_M) w.ln_leaf = ar.take<float>(rows * 2 * (W / 4));
    }
    if (t->kind == 0 && t->weight_format == 0) {
        if (t->ln_fold) {
            w.x3c = ar.take<unsigned char>((size_t)B * resid_row_bytes(W));
            w.partc = ar.take<float>((size_t)B * 2 * (W / 256));
            if (B <= SKINNY_MAX_M) w.leafc = ar.take<float>((size_t)B * 2 * (W / 4));
        } else {
            w.xc = ar.take<float>((size_t)B * W);
        }
    }
    if (out) *out = w;
    return ar.off + 256;
}

int check_tower(const clipmi_tower* t, int kind, const char* who) {
    if (!t) return set_err(CLIPMI_EINVAL, "%s: NULL tower", who);
    if (t->abi_version != CLIPMI_ABI_VERSION)
        return set_err(CLIPMI_EINVAL, "%s: tower ABI %d != %d", who, t->abi_version, CLIPMI_ABI_VERSION);
    if (t->kind != kind) return set_err(CLIPMI_EINVAL, "%s: tower kind %d", who, t->kind);
    if (t->width % 128 != 0 || t->heads * 64 != t->width || t->mlp != 4 * t->width || t->embed % 128 != 0 ||
        t->width > 1024 || t->layers < 1)
        return set_err(CLIPMI_EUNSUPPORTED,
                       "%s: width=%d heads=%d mlp=%d embed=%d (need width %% 128 == 0 <= 1024, head dim 64, embed %% 128 == 0)",
                       who, t->width, t->heads, t->mlp, t->embed);
    if (t->weight_format != 0 && t->weight_format != 1)
        return set_err(CLIPMI_EINVAL, "%s: weight_format %d", who, t->weight_format);
    if (t->weight_format == 1 && t->width % 256 != 0)
        return set_err(CLIPMI_EUNSUPPORTED, "%s: fp8 weights need width %% 256 == 0 (width %d)", who, t->width);
    if (t->ln_fold != 0 && (t->ln_fold != 1 || t->width % 256 != 0))
        return set_err(CLIPMI_EINVAL, "%s: ln_fold %d needs width %% 256 == 0 (width %d)", who, t->ln_fold, t->width);
#ifndef CLIPMI_DEV
    if (t->ln_fold != 0 && t->weight_format != 0)
        return set_err(CLIPMI_EUNSUPPORTED, "%s: folded LayerNorms on FP8 weights exist in the development library only", who);
#endif
    if (t->tokens > 80 && kind == 1)
        return set_err(CLIPMI_EUNSUPPORTED, "%s: %d tokens (causal attention covers <= 80)", who, t->tokens);
    return 0;
}

template <typename T>
const T* at(const void* blob, uint64_t off) {
    return reinterpret_cast<const T*>(static_cast<const char*>(blob) + off);
}

// The pruned tail of a vision tower (bf16 weights). encode_image reads only the class-token row of every image behind the
// last block, and everything behind that block's attention is row-wise: out_proj, the residual adds, the LayerNorm
// statistics, c_fc + QuickGELU and c_proj run over the B class-token rows instead of all B * L (ViT-B/32: 49 of 50 rows of
// three of the twelve blocks' four GEMMs were computed to be thrown away). A row's bits depend neither on the batch size
// nor on the kernel that computes it (gemm.hip), so the embeddings are the ones the full block gives.
// At every batch size. With one or two ViT-B/32 images (all token rows on the skinny kernels) the tail is four launches in
// place of three, and it still measured faster per call there; the CLIPMI_ENCODE_TAIL = 0 / 2 numbers are in DESIGN 4.7a.
// CLIPMI_ENCODE_TAIL (development library): 0 = the last block over all rows; 1 = the product's rule and 2 = the tail at every
// batch size, which are the same thing today.
bool encode_tail() {
    static const int mode = (int)dev_knob("CLIPMI_ENCODE_TAIL", 1);
    return mode != 0;
}

// dst[b][:] = src[b * L][:], rows of row_bytes bytes (a multiple of 16): the class-token rows of the residual stream
int launch_gather_rows(const void* src, void* dst, int B, int L, size_t row_bytes, hipStream_t st) {
    if (row_bytes % 16 != 0) return set_err(CLIPMI_EINVAL, "gather_rows: %zu bytes per row", row_bytes);
    const int row16 = (int)(row_bytes / 16);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(((long long)B * row16 + 255) / 256)), dim3(256), 0, st,
                       static_cast<const uint4*>(src), static_cast<uint4*>(dst), B, L, row16);
    CLIPMI_CHECK_LAUNCH("gather_rows_kernel");
    return 0;
}

// One layer's tensors in the weight blob (clipmi_tower lo_*), typed; qkv_b / fc_b are the folded cb rows in LN-folded towers
struct LayerW {
    const unsigned short *qkv_w, *out_w, *fc_w, *proj_w;
    const float *qkv_b, *out_b, *fc_b, *proj_b, *qkv_colsum, *fc_colsum, *qkv_s, *out_s, *fc_s, *proj_s, *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    LayerW(const clipmi_tower* t, const void* blob, int l) {
        const uint64_t lb = t->off_layers + (uint64_t)l * t->layer_stride;
        auto f = [&](uint64_t lo) { return at<float>(blob, lb + lo); };
        auto h = [&](uint64_t lo) { return at<unsigned short>(blob, lb + lo); };
        qkv_w = h(t->lo_qkv_w); out_w = h(t->lo_out_w); fc_w = h(t->lo_fc_w); proj_w = h(t->lo_proj_w);
        qkv_b = f(t->ln_fold ? t->lo_qkv_cb : t->lo_qkv_b); fc_b = f(t->ln_fold ? t->lo_fc_cb : t->lo_fc_b);
        out_b = f(t->lo_out_b); proj_b = f(t->lo_proj_b); qkv_colsum = f(t->lo_qkv_colsum); fc_colsum = f(t->lo_fc_colsum);
        qkv_s = f(t->lo_qkv_s); out_s = f(t->lo_out_s); fc_s = f(t->lo_fc_s); proj_s = f(t->lo_proj_s);          // FP8 weight scales
        ln1_w = f(t->lo_ln1_w); ln1_b = f(t->lo_ln1_b); ln2_w = f(t->lo_ln2_w); ln2_b = f(t->lo_ln2_b);
    }
};

// the fields every linear layer sets; what a form adds (statistics, scales, the split residual) the form sets itself
GemmArgs linear(const void* A, size_t lda_bytes, const unsigned short* W, const float* bias, int M, int N, int K, void* out) {
    GemmArgs g{};
    g.A = static_cast<const unsigned short*>(A); g.lda_bytes = (unsigned)lda_bytes; g.W = W; g.bias = bias;
    g.M = M; g.N = N; g.K = K; g.out = out;
    return g;
}

// where the blocks left the residual rows: f32 x or split x3 (the tower's form), one per image every row_step rows (L, or 1 behind a tail)
struct Resid { const float* x; const void* x3; long long row_step; };

// what every block form works on; tail: the last block runs its tail on the class-token rows (vision towers, bf16 weights)
struct Blocks {
    const clipmi_tower* t; const void* blob; const Ws& w; int B, causal; hipStream_t st; GemmProbe* probe; bool tail; int W, L, M, last;
};

// plain blocks, the pruned tail (see tail_ln): the class-token rows of the f32 residual move to w.xc, ln_2 writes its B rows to the
// head of w.h once out_proj has read the attention rows there
int tail_plain(const Blocks& c, const LayerW& lw, Resid& r) {
    const Ws& w = c.w; const int B = c.B, W = c.W;
    if (int rc = launch_gather_rows(w.x, w.xc, B, c.L, (size_t)W * 4, c.st)) return rc;
    if (int rc = launch_gemm_algo(linear(w.h, (size_t)c.L * W * 2, lw.out_w, lw.out_b, B, W, W, w.xc), EPI_BIAS_RESID_F32, 0, c.st, nullptr)) return rc;
    LnArgs ln2{w.xc, lw.ln2_w, lw.ln2_b, w.h, nullptr, 1, B, W, 1};
    if (int rc = launch_layernorm(ln2, c.st)) return rc;
    if (int rc = launch_gemm_algo(linear(w.h, 0, lw.fc_w, lw.fc_b, B, 4 * W, W, w.big), EPI_BIAS_QGELU_BF16, 0, c.st, nullptr)) return rc;
    r = Resid{w.xc, nullptr, 1};
    return launch_gemm_algo(linear(w.big, 0, lw.proj_w, lw.proj_b, B, W, 4 * W, w.xc), EPI_BIAS_RESID_F32, 0, c.st, nullptr);
}

int blocks_plain(const Blocks& c, Resid& r) {
    const Ws& w = c.w; const int W = c.W, M = c.M;
    for (int l = 0; l <= c.last; ++l) {
        const LayerW lw(c.t, c.blob, l);
        LnArgs ln{w.x, lw.ln1_w, lw.ln1_b, w.h, nullptr, 1, M, W, 1};
        if (int rc = launch_layernorm(ln, c.st)) return rc;
        if (int rc = launch_gemm_algo(linear(w.h, 0, lw.qkv_w, lw.qkv_b, M, 3 * W, W, w.big), EPI_BIAS_BF16, 0, c.st, c.probe)) return rc;
        if (int rc = launch_attention(w.big, w.h, c.B, c.L, c.t->heads, c.causal, ATTN_DEFAULT, c.st)) return rc;
        if (c.tail && l == c.last) return tail_plain(c, lw, r);
        if (int rc = launch_gemm_algo(linear(w.h, 0, lw.out_w, lw.out_b, M, W, W, w.x), EPI_BIAS_RESID_F32, 0, c.st, c.probe)) return rc;
        ln.w = lw.ln2_w; ln.b = lw.ln2_b;
        if (int rc = launch_layernorm(ln, c.st)) return rc;
        if (int rc = launch_gemm_algo(linear(w.h, 0, lw.fc_w, lw.fc_b, M, 4 * W, W, w.big), EPI_BIAS_QGELU_BF16, 0, c.st, c.probe)) return rc;
        if (int rc = launch_gemm_algo(linear(w.big, 0, lw.proj_w, lw.proj_b, M, W, 4 * W, w.x), EPI_BIAS_RESID_F32, 0, c.st, c.probe)) return rc;
    }
    return 0;
}

// LN-folded blocks, the pruned tail: K and V of every token were needed, from here on only the class-token rows are. Their residual
// rows move to w.x3c (not in place: row b would land on rows another workgroup still reads), out_proj reads its A rows L apart in w.h,
// c_fc / c_proj use the head of w.big. No probe: bench.py's per-kernel times stay averages over one shape. B <= 128: leaves of their own.
int tail_ln(const Blocks& c, const LayerW& lw, Resid& r) {
    const Ws& w = c.w; const int B = c.B, W = c.W;
    float* const leaf = w.leafc && gemm_resid_writes_leaves(B, W, W) && gemm_resid_writes_leaves(B, W, 4 * W) ? w.leafc : nullptr;
    if (int rc = launch_attention(w.big, w.h, B, c.L, c.t->heads, c.causal, ATTN_DEFAULT, c.st)) return rc;
    if (int rc = launch_gather_rows(w.x3, w.x3c, B, c.L, resid_row_bytes(W), c.st)) return rc;
    GemmArgs out = linear(w.h, (size_t)c.L * W * 2, lw.out_w, lw.out_b, B, W, W, nullptr);
    out.x3 = w.x3c; out.ln_part = w.partc; out.ln_leaf = leaf; out.tmp_f32 = w.x;
    if (int rc = launch_gemm_algo(out, EPI_BIAS_RESID_LN_F32, 0, c.st, nullptr)) return rc;
    GemmArgs fc = linear(w.x3c, resid_row_bytes(W), lw.fc_w, lw.fc_b, B, 4 * W, W, w.big);
    fc.colsum = lw.fc_colsum; fc.ln_part_in = w.partc; fc.ln_leaf_in = leaf;
    if (int rc = launch_gemm_algo(fc, EPI_LN_BIAS_QGELU_BF16, 0, c.st, nullptr)) return rc;
    GemmArgs proj = linear(w.big, 0, lw.proj_w, lw.proj_b, B, W, 4 * W, nullptr);
    proj.x3 = w.x3c; proj.ln_part = w.partc; proj.ln_leaf = leaf; proj.tmp_f32 = w.x;
    r = Resid{nullptr, w.x3c, 1};
    return launch_gemm_algo(proj, EPI_BIAS_RESID_LN_F32, 0, c.st, nullptr);
}

// LN-folded blocks (gemm.hpp): ln_1 / ln_2 never run as passes of their own, the residual stream lives split in w.x3 with its row
// statistics in w.ln_part (the caller left the embedded rows so); w.x (f32) is only the scratch of residual GEMMs off the persistent kernel
int blocks_ln(const Blocks& c, Resid& r) {
    const Ws& w = c.w; const int W = c.W, M = c.M;
    // One prompt / one image (M <= 128: the skinny kernels, ~90 dependent launches of ~4 us): the residual GEMMs update the split rows
    // themselves and hand the statistics on as leaves. leaf_in: w.ln_leaf, not w.ln_part, describes w.x3 - from the first residual GEMM on.
    float* const leaf = w.ln_leaf && gemm_resid_writes_leaves(M, W, W) && gemm_resid_writes_leaves(M, W, 4 * W) ? w.ln_leaf : nullptr;
    const float* leaf_in = nullptr;
    for (int l = 0; l <= c.last; ++l) {
        const LayerW lw(c.t, c.blob, l);
        GemmArgs qkv = linear(w.x3, resid_row_bytes(W), lw.qkv_w, lw.qkv_b, M, 3 * W, W, w.big);
        qkv.colsum = lw.qkv_colsum; qkv.ln_part_in = w.ln_part; qkv.ln_leaf_in = leaf_in;
        if (int rc = launch_gemm_algo(qkv, EPI_LN_BIAS_BF16, 0, c.st, c.probe)) return rc;
        if (c.tail && l == c.last) return tail_ln(c, lw, r);
        // (bench probe, mode 2: attention's own end stamp, so that out_proj gets a completion-to-completion time too)
        hipEvent_t* aev = nullptr;
        if (c.probe && c.probe->mode == 2 && c.probe->n < GemmProbe::MAX) aev = &c.probe->ev[2 * c.probe->begin(GemmProbe::EPI_ATTENTION, 2, c.st, 0)];
        if (int rc = launch_attention(w.big, w.h, c.B, c.L, c.t->heads, c.causal, ATTN_DEFAULT, c.st, nullptr, nullptr, nullptr, aev)) return rc;
        GemmArgs out = linear(w.h, 0, lw.out_w, lw.out_b, M, W, W, nullptr);
        out.x3 = w.x3; out.ln_part = w.ln_part; out.ln_leaf = leaf; out.tmp_f32 = w.x;
        if (int rc = launch_gemm_algo(out, EPI_BIAS_RESID_LN_F32, 0, c.st, c.probe)) return rc;
        leaf_in = leaf;
        GemmArgs fc = linear(w.x3, resid_row_bytes(W), lw.fc_w, lw.fc_b, M, 4 * W, W, w.big);
        fc.colsum = lw.fc_colsum; fc.ln_part_in = w.ln_part; fc.ln_leaf_in = leaf_in;
        if (int rc = launch_gemm_algo(fc, EPI_LN_BIAS_QGELU_BF16, 0, c.st, c.probe)) return rc;
        GemmArgs proj = linear(w.big, 0, lw.proj_w, lw.proj_b, M, W, 4 * W, nullptr);
        proj.x3 = w.x3; proj.ln_part = w.ln_part; proj.ln_leaf = leaf; proj.tmp_f32 = w.x;
        if (int rc = launch_gemm_algo(proj, EPI_BIAS_RESID_LN_F32, 0, c.st, c.probe)) return rc;
    }
    return 0;
}

// The two steps both FP8 forms share: attention's output and the QuickGELU rows travel as e4m3 with MX block scales, written by the
// producer itself where it has the fused form (attention52x4; the persistent QuickGELU GEMM), else by quantize_rows_fp8mx_kernel over
// the producer's bf16 rows: the same bytes either way.
bool fp8_fuse_off() { static const bool off = dev_knob("CLIPMI_FP8_FUSE", 1) == 0; return off; }   // A/B aid (development build)
// attention -> e4m3 rows w.a8 + block scales w.a_bs
int attention_fp8(const Blocks& c, const Ws& w) {
    bool fused = false;
    if (int rc = launch_attention(w.big, w.h, c.B, c.L, c.t->heads, c.causal, ATTN_DEFAULT, c.st, fp8_fuse_off() ? nullptr : w.a8, w.a_bs, &fused)) return rc;
    return fused ? 0 : launch_quantize_rows_fp8mx(w.h, w.a8, w.a_bs, c.M, c.W, c.st);
}
// c_fc (`fc`, into w.big) -> e4m3 QuickGELU rows *h8 + block scales w.a_bs; mx_out: the GEMM writes them itself, into the bf16 buffer's bytes
int fc_fp8(const Blocks& c, const Ws& w, GemmArgs fc, int epi, bool mx_out, const unsigned char** h8) {
    if (mx_out) fc.out_bscale = w.a_bs;
    *h8 = mx_out ? reinterpret_cast<const unsigned char*>(w.big) : w.a8;
    if (int rc = launch_gemm_fp8(fc, epi, c.st)) return rc;
    return mx_out ? 0 : launch_quantize_rows_fp8mx(w.big, w.a8, w.a_bs, c.M, 4 * c.W, c.st);
}

// FP8 blocks (weight_format 1, BASELINE.json configs[4]): the four linear layers run on the FP8 matrix cores - weights are e4m3 with one
// scale per output channel, LayerNorm writes its rows as e4m3 with a row scale, gemm256f8 applies both scales in its epilogue
int blocks_fp8(const Blocks& c) {
    const Ws& w = c.w; const int W = c.W, M = c.M;
    const bool fc_mx = !fp8_fuse_off() && gemm_fp8_emits_mx(M, 4 * W, W);
    for (int l = 0; l <= c.last; ++l) {
        const LayerW lw(c.t, c.blob, l);
        LnArgs ln{w.x, lw.ln1_w, lw.ln1_b, w.h, nullptr, 1, M, W, 1};
        ln.out8 = w.a8; ln.scale8 = w.a_scale;
        if (int rc = launch_layernorm(ln, c.st)) return rc;
        GemmArgs qkv = linear(w.a8, 0, lw.qkv_w, lw.qkv_b, M, 3 * W, W, w.big);
        qkv.a_scale = w.a_scale; qkv.w_scale = lw.qkv_s;
        if (int rc = launch_gemm_fp8(qkv, EPI_BIAS_BF16, c.st)) return rc;
        if (int rc = attention_fp8(c, w)) return rc;
        GemmArgs out = linear(w.a8, 0, lw.out_w, lw.out_b, M, W, W, w.x);
        out.a_bscale = w.a_bs; out.w_scale = lw.out_s;
        if (int rc = launch_gemm_fp8(out, EPI_BIAS_RESID_F32, c.st)) return rc;
        ln.w = lw.ln2_w; ln.b = lw.ln2_b;
        if (int rc = launch_layernorm(ln, c.st)) return rc;
        GemmArgs fc = linear(w.a8, 0, lw.fc_w, lw.fc_b, M, 4 * W, W, w.big);
        fc.a_scale = w.a_scale; fc.w_scale = lw.fc_s;
        const unsigned char* h8;
        if (int rc = fc_fp8(c, w, fc, EPI_BIAS_QGELU_BF16, fc_mx, &h8)) return rc;
        GemmArgs proj = linear(h8, 0, lw.proj_w, lw.proj_b, M, W, 4 * W, w.x);
        proj.a_bscale = w.a_bs; proj.w_scale = lw.proj_s;
        if (int rc = launch_gemm_fp8(proj, EPI_BIAS_RESID_F32, c.st)) return rc;
    }
    return 0;
}

#ifdef CLIPMI_DEV
// FP8 blocks with folded LayerNorms (development library: parity-green and measured SLOWER than the LayerNorm-pass tower above,
// DESIGN 4.4c). The residual stream stays f32 in w.x; every producer of residual rows (the embedding stage through
// rows_mx_stats_kernel, then the residual GEMMs' store passes: EPI_BIAS_RESID_LN8) also leaves them as e4m3 with MX block scales
// (w.x8 / w.x8_bs) and statistics partials (w.ln_part); qkv / c_fc take THOSE as A, with the LN-folded epilogue. No LayerNorm pass.
int blocks_ln_fp8(const Blocks& c) {
    const Ws& w = c.w; const int W = c.W, M = c.M;
    for (int l = 0; l <= c.last; ++l) {
        const LayerW lw(c.t, c.blob, l);
        GemmArgs qkv = linear(w.x8, 0, lw.qkv_w, lw.qkv_b, M, 3 * W, W, w.big);
        qkv.a_bscale = w.x8_bs; qkv.w_scale = lw.qkv_s; qkv.colsum = lw.qkv_colsum; qkv.ln_part_in = w.ln_part;
        if (int rc = launch_gemm_fp8(qkv, EPI_LN_BIAS_BF16, c.st)) return rc;
        if (int rc = attention_fp8(c, w)) return rc;
        GemmArgs out = linear(w.a8, 0, lw.out_w, lw.out_b, M, W, W, w.x);
        out.a_bscale = w.a_bs; out.w_scale = lw.out_s; out.x8 = w.x8; out.x8_bs = w.x8_bs; out.ln_part = w.ln_part;
        if (int rc = launch_gemm_fp8(out, EPI_BIAS_RESID_LN8, c.st)) return rc;
        GemmArgs fc = linear(w.x8, 0, lw.fc_w, lw.fc_b, M, 4 * W, W, w.big);
        fc.a_bscale = w.x8_bs; fc.w_scale = lw.fc_s; fc.colsum = lw.fc_colsum; fc.ln_part_in = w.ln_part;
        const unsigned char* h8;
        if (int rc = fc_fp8(c, w, fc, EPI_LN_BIAS_QGELU_BF16, !fp8_fuse_off(), &h8)) return rc;
        GemmArgs proj = linear(h8, 0, lw.proj_w, lw.proj_b, M, W, 4 * W, w.x);
        proj.a_bscale = w.a_bs; proj.w_scale = lw.proj_s; proj.x8 = w.x8; proj.x8_bs = w.x8_bs; proj.ln_part = w.ln_part;
        if (int rc = launch_gemm_fp8(proj, EPI_BIAS_RESID_LN8, c.st)) return rc;
    }
    return 0;
}
#endif

// the 12 (or 24) residual attention blocks shared by both towers, in the tower's form; *r: where they leave the residual rows
int run_layers(const clipmi_tower* t, const void* blob, const Ws& w, int B, int causal, hipStream_t st, GemmProbe* probe, Resid* r) {
    const bool fp8 = t->weight_format == 1;
    const bool tail = !causal && !fp8 && (t->ln_fold ? w.x3c != nullptr : w.xc != nullptr) && encode_tail();
    const Blocks c{t, blob, w, B, causal, st, probe, tail, t->width, t->tokens, B * t->tokens, t->layers - 1};
    *r = Resid{w.x, w.x3, t->tokens};
#ifdef CLIPMI_DEV
    if (t->ln_fold && fp8) return blocks_ln_fp8(c);
#endif
    if (t->ln_fold) return blocks_ln(c, *r);
    return fp8 ? blocks_fp8(c) : blocks_plain(c, *r);
}

// rows r (with rowidx: gathered by index, the text tower's EOT rows) -> final LayerNorm -> projection [E][W] -> f32 [B][E] (-> L2 normalise)
int run_head(const clipmi_tower* t, const void* blob, const Ws& w, const Resid& r, int B, const int* rowidx, float* out, int normalize, hipStream_t st) {
    const bool split = t->ln_fold && t->weight_format == 0;      // bf16 LN-folded towers keep the residual as (hi, lo)
    LnArgs ln{split ? nullptr : r.x, at<float>(blob, t->off_ln_post_w), at<float>(blob, t->off_ln_post_b), w.pooled, rowidx,
              r.row_step, B, t->width, 1};
    ln.x3 = r.x3;                          // split: the residual stream is rows of (hi | lo)
    if (int rc = launch_layernorm(ln, st)) return rc;
    if (int rc = launch_gemm_algo(linear(w.pooled, 0, at<unsigned short>(blob, t->off_out_proj), nullptr, B, t->embed, t->width, out), EPI_F32, 0, st)) return rc;
    return normalize ? clipmi_l2_normalize_rows(out, B, t->embed, st) : 0;
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" size_t clipmi_encode_image_workspace_bytes(const clipmi_tower* t, int B) {
    if (check_tower(t, 0, "encode_image")) return 0;
    if (B < 1) { set_err(CLIPMI_EINVAL, "encode_image: B=%d", B); return 0; }
    return carve(t, B, nullptr, ~(size_t)0, nullptr);
}

// The embedding front end of the vision tower, everything in front of the first block: patches -> patch GEMM (+ positional
// rows, EPI_PATCH_F32; `algo` as in launch_gemm_algo, 0 in the product) -> class-token rows -> ln_pre (skipped when
// !with_ln_pre: the test hook's view of the rows in front of it). Shared by clipmi_encode_image and clipmi_dbg_embed_image.
static int embed_image(const clipmi_tower* t, const void* blob_dev, const void* pixels_dev, int pix_dtype, int B, const Ws& w,
                       int algo, bool with_ln_pre, hipStream_t st) {
    const int W = t->width, L = t->tokens;
    const int grid = t->res / t->patch, np = grid * grid;
    PatchArgs pa{pixels_dev, w.patches, pix_dtype, B, t->res, t->patch, grid, np, t->patch_k};
    if (int rc = launch_patchify(pa, st)) return rc;
    GemmArgs g{};
    g.A = w.patches; g.W = at<unsigned short>(blob_dev, t->off_patch_w); g.bias = nullptr; g.out = w.x;
    g.M = B * np; g.N = W; g.K = t->patch_k; g.pos = at<float>(blob_dev, t->off_pos); g.np = np; g.L = L;
    if (int rc = launch_gemm_algo(g, EPI_PATCH_F32, algo, st)) return rc;
    hipLaunchKernelGGL(cls_rows_kernel, dim3((unsigned)(((long long)B * W + 255) / 256)), dim3(256), 0, st, w.x,
                       at<float>(blob_dev, t->off_cls), at<float>(blob_dev, t->off_pos), B, L, W);
    CLIPMI_CHECK_LAUNCH("cls_rows_kernel");
    if (!with_ln_pre) return 0;
    LnArgs ln{w.x, at<float>(blob_dev, t->off_ln_pre_w), at<float>(blob_dev, t->off_ln_pre_b), w.x, nullptr, 1, B * L, W, 0};
    const bool fold8 = t->ln_fold && t->weight_format == 1;
    if (t->ln_fold && !fold8) { ln.out_x3 = w.x3; ln.out_part = w.ln_part; }     // straight into the split residual
    return launch_layernorm(ln, st);       // ln_pre (ln_fold 0 / FP8: in place, each wave owns its row)
}

// arguments of clipmi_encode_image and of its test hook (`who` names the entry point in the message)
static int check_image_args(const clipmi_tower* t, const void* blob_dev, const void* pixels_dev, int pix_dtype, int B,
                            bool have_out, const void* ws_dev, size_t ws_bytes, const char* who) {
    if (int rc = check_tower(t, 0, who)) return rc;
    if (!blob_dev || !pixels_dev || !have_out || !ws_dev) return set_err(CLIPMI_EINVAL, "%s: NULL pointer", who);
    if (B < 1) return set_err(CLIPMI_EINVAL, "%s: B=%d", who, B);
    if (pix_dtype != CLIPMI_F32 && pix_dtype != CLIPMI_BF16 && pix_dtype != CLIPMI_U8)
        return set_err(CLIPMI_EINVAL, "%s: pix_dtype %d", who, pix_dtype);
    const int grid = t->res / t->patch, np = grid * grid;
    if (np + 1 != t->tokens || t->patch_k % 64 != 0 || t->patch_k < 3 * t->patch * t->patch)
        return set_err(CLIPMI_EINVAL, "%s: inconsistent tower (res %d patch %d tokens %d patch_k %d)", who, t->res,
                       t->patch, t->tokens, t->patch_k);
    const size_t need = clipmi_encode_image_workspace_bytes(t, B);
    if (ws_bytes < need) return set_err(CLIPMI_EWORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, need);
    return 0;
}

static int encode_image_impl(const clipmi_tower* t, const void* blob_dev, const void* pixels_dev, int pix_dtype,
                             int B, float* out_dev, int normalize, void* ws_dev, size_t ws_bytes, void* stream, GemmProbe* probe) {
    if (int rc = check_image_args(t, blob_dev, pixels_dev, pix_dtype, B, out_dev != nullptr, ws_dev, ws_bytes, "encode_image")) return rc;
    Ws w;
    carve(t, B, ws_dev, ws_bytes, &w);
    hipStream_t st = as_stream(stream);
    if (int rc = embed_image(t, blob_dev, pixels_dev, pix_dtype, B, w, 0, true, st)) return rc;
#ifdef CLIPMI_DEV
    if (t->ln_fold && t->weight_format == 1)     // FP8 tower with folded LayerNorms: the embedded rows' e4m3 image + statistics for the first qkv GEMM
        if (int rc = launch_rows_mx_stats(w.x, w.x8, w.x8_bs, w.ln_part, B * t->tokens, t->width, st)) return rc;
#endif
    Resid r;
    if (int rc = run_layers(t, blob_dev, w, B, 0, st, probe, &r)) return rc;
    return run_head(t, blob_dev, w, r, B, nullptr, out_dev, normalize, st);
}

extern "C" int clipmi_encode_image(const clipmi_tower* t, const void* blob_dev, const void* pixels_dev, int pix_dtype,
                                   int B, float* out_dev, int normalize, void* ws_dev, size_t ws_bytes, void* stream) {
    return encode_image_impl(t, blob_dev, pixels_dev, pix_dtype, B, out_dev, normalize, ws_dev, ws_bytes, stream, nullptr);
}

extern "C" size_t clipmi_encode_text_workspace_bytes(const clipmi_tower* t, int Q) {
    if (check_tower(t, 1, "encode_text")) return 0;
    if (Q < 1) { set_err(CLIPMI_EINVAL, "encode_text: Q=%d", Q); return 0; }
    return carve(t, Q, nullptr, ~(size_t)0, nullptr);
}

// The embedding front end of the text tower: token + positional embedding, the EOT rows and, for LN-folded towers, the split
// rows with their statistics - in one launch where the fused kernel exists. Shared by clipmi_encode_text and
// clipmi_dbg_embed_text.
static int embed_text(const clipmi_tower* t, const void* blob_dev, const int32_t* ids_dev, int Q, const Ws& w, hipStream_t st) {
    const int W = t->width, L = t->tokens;
    const long long n4 = (long long)Q * L * (W / 4);
    const bool fold8_ = t->ln_fold && t->weight_format == 1;
    if (t->ln_fold && !fold8_ && W % 256 == 0 && W <= 1024) {
        // LN-folded tower: embedding, split rows + statistics and the EOT rows in one launch (the bits of the three kernels below)
        hipLaunchKernelGGL(text_embed_split_kernel, dim3((unsigned)((Q * L + 3) / 4 + 1)), dim3(256), 0, st, ids_dev,
                           at<float>(blob_dev, t->off_tok_emb), at<float>(blob_dev, t->off_pos), w.x3, w.ln_part, w.rowidx, Q, L, W,
                           t->vocab);
        CLIPMI_CHECK_LAUNCH("text_embed_split_kernel");
        return 0;
    }
    hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, w.x, ids_dev,
                       at<float>(blob_dev, t->off_tok_emb), at<float>(blob_dev, t->off_pos), Q, L, W, t->vocab);
    CLIPMI_CHECK_LAUNCH("text_embed_kernel");
    hipLaunchKernelGGL(eot_rows_kernel, dim3((Q + 63) / 64), dim3(64), 0, st, ids_dev, w.rowidx, Q, L);
    CLIPMI_CHECK_LAUNCH("eot_rows_kernel");
#ifdef CLIPMI_DEV
    if (t->ln_fold && t->weight_format == 1) {
        if (int rc = launch_rows_mx_stats(w.x, w.x8, w.x8_bs, w.ln_part, Q * L, W, st)) return rc;
    } else
#endif
    if (t->ln_fold) {
        if (int rc = launch_split_stats(w.x, false, w.x3, w.ln_part, Q * L, W, st)) return rc;
    }
    return 0;
}

// arguments of clipmi_encode_text and of its test hook (`who` names the entry point in the message)
static int check_text_args(const clipmi_tower* t, const void* blob_dev, const int32_t* ids_dev, int Q, bool have_out, const void* ws_dev,
                           size_t ws_bytes, const char* who) {
    if (int rc = check_tower(t, 1, who)) return rc;
    if (!blob_dev || !ids_dev || !have_out || !ws_dev) return set_err(CLIPMI_EINVAL, "%s: NULL pointer", who);
    if (Q < 1) return set_err(CLIPMI_EINVAL, "%s: Q=%d", who, Q);
    const size_t need = clipmi_encode_text_workspace_bytes(t, Q);
    if (ws_bytes < need) return set_err(CLIPMI_EWORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, need);
    return 0;
}

extern "C" int clipmi_encode_text(const clipmi_tower* t, const void* blob_dev, const int32_t* ids_dev, int Q,
                                  float* out_dev, int normalize, void* ws_dev, size_t ws_bytes, void* stream) {
    if (int rc = check_text_args(t, blob_dev, ids_dev, Q, out_dev != nullptr, ws_dev, ws_bytes, "encode_text")) return rc;
    Ws w;
    carve(t, Q, ws_dev, ws_bytes, &w);
    hipStream_t st = as_stream(stream);
    if (int rc = embed_text(t, blob_dev, ids_dev, Q, w, st)) return rc;
    Resid r;
    if (int rc = run_layers(t, blob_dev, w, Q, 1, st, nullptr, &r)) return rc;
    r.row_step = 1;          // the head gathers the EOT rows by index
    return run_head(t, blob_dev, w, r, Q, w.rowidx, out_dev, normalize, st);
}

// Test hooks of the embedding front ends: the product's own launch sequence (embed_image / embed_text above) in the tower's
// ordinary workspace, then copies of what it left there, on the same stream. Every output pointer is optional.
static int copy_out(void* dst, const void* src, size_t bytes, hipStream_t st, const char* who) {
    if (!dst) return 0;
    if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return set_err(CLIPMI_EHIP, "%s: hipMemcpyAsync", who);
    return 0;
}

extern "C" int clipmi_dbg_embed_image(const clipmi_tower* t, const void* blob_dev, const void* pixels_dev, int pix_dtype, int B,
                                      int algo, int with_ln_pre, void* patches_out_dev, float* rows_out_dev, void* x3_out_dev,
                                      float* part_out_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    const char* who = "dbg_embed_image";
    if (int rc = check_image_args(t, blob_dev, pixels_dev, pix_dtype, B, true, ws_dev, ws_bytes, who)) return rc;
    const int W = t->width, L = t->tokens, np = L - 1;
    if (algo < 0 || algo > 2) return set_err(CLIPMI_EINVAL, "%s: algo %d (0 = by shape, 1 = 128 x 128, 2 = 256 x 256)", who, algo);
    if (algo == 2 && (W % 256 != 0 || t->patch_k < 128))
        return set_err(CLIPMI_EINVAL, "%s: algo 2 needs width %% 256 == 0 and patch_k >= 128 (width %d, patch_k %d)", who, W, t->patch_k);
    // the form the rows have behind ln_pre: split rows + partials (bf16 LN-folded towers) or f32 rows
    const bool split = with_ln_pre && t->ln_fold && t->weight_format == 0;
    if (split ? rows_out_dev != nullptr : (x3_out_dev != nullptr || part_out_dev != nullptr))
        return set_err(CLIPMI_EINVAL, "%s: this tower's rows are %s here", who, split ? "split rows + partials" : "f32 rows");
    Ws w;
    carve(t, B, ws_dev, ws_bytes, &w);
    hipStream_t st = as_stream(stream);
    if (int rc = embed_image(t, blob_dev, pixels_dev, pix_dtype, B, w, algo, with_ln_pre != 0, st)) return rc;
    const size_t rows = (size_t)B * L;
    if (int rc = copy_out(patches_out_dev, w.patches, (size_t)B * np * t->patch_k * 2, st, who)) return rc;
    if (int rc = copy_out(rows_out_dev, w.x, rows * W * 4, st, who)) return rc;
    if (int rc = copy_out(x3_out_dev, w.x3, rows * resid_row_bytes(W), st, who)) return rc;
    return copy_out(part_out_dev, w.ln_part, rows * 2 * (W / 256) * 4, st, who);
}

extern "C" int clipmi_dbg_embed_text(const clipmi_tower* t, const void* blob_dev, const int32_t* ids_dev, int Q, float* rows_out_dev,
                                     void* x3_out_dev, float* part_out_dev, int32_t* rowidx_out_dev, void* ws_dev, size_t ws_bytes,
                                     void* stream) {
    const char* who = "dbg_embed_text";
    if (int rc = check_text_args(t, blob_dev, ids_dev, Q, true, ws_dev, ws_bytes, who)) return rc;
    const bool split = t->ln_fold && t->weight_format == 0;
    if (split ? rows_out_dev != nullptr : (x3_out_dev != nullptr || part_out_dev != nullptr))
        return set_err(CLIPMI_EINVAL, "%s: this tower's rows are %s", who, split ? "split rows + partials" : "f32 rows");
    Ws w;
    carve(t, Q, ws_dev, ws_bytes, &w);
    hipStream_t st = as_stream(stream);
    if (int rc = embed_text(t, blob_dev, ids_dev, Q, w, st)) return rc;
    const int W = t->width;
    const size_t rows = (size_t)Q * t->tokens;
    if (int rc = copy_out(rows_out_dev, w.x, rows * W * 4, st, who)) return rc;
    if (int rc = copy_out(x3_out_dev, w.x3, rows * resid_row_bytes(W), st, who)) return rc;
    if (int rc = copy_out(part_out_dev, w.ln_part, rows * 2 * (W / 256) * 4, st, who)) return rc;
    return copy_out(rowidx_out_dev, w.rowidx, (size_t)Q * 4, st, who);
}

// launch_gather_rows as the pruned tail calls it: dst[b][:] = src[b * L][:], rows of row_bytes bytes
extern "C" int clipmi_dbg_gather_rows(const void* src_dev, void* dst_dev, int B, int L, size_t row_bytes, void* stream) {
    if (!src_dev || !dst_dev || B < 1 || L < 1 || row_bytes < 16) return set_err(CLIPMI_EINVAL, "dbg_gather_rows: bad arguments");
    return launch_gather_rows(src_dev, dst_dev, B, L, row_bytes, as_stream(stream));
}

// Measurement hook (bench.py roofline): clipmi_encode_image `reps` times per estimator with HIP events around the launches
// of the GEMM whose epilogue is `probe_epi` (1 = MLP c_fc + QuickGELU) on `stream`; synchronises. Three estimators of that
// kernel's in-situ duration, each from its own `reps` forward passes (ms[0..2], averages over the timed launches):
//   ms[0] begin -> end events of hipExtLaunchKernel. The begin event is stamped when the dispatch packet is PROCESSED, which in
//         a back-to-back stream is before the previous kernel has drained: it reads long (14 % for the 200-us c_fc launch).
//   ms[1] a plain event record in front of the launch (completes with everything before it) -> the launch's end event:
//         kernel + the boundary to the previous kernel + the event packet.
//   ms[2] end event of the previous GEMM launch -> end event of this one, used where that previous launch is the kernel
//         directly in front in the stream (LN-folded tower: out_proj -> c_fc): completion to completion = the kernel + ONE
//         kernel boundary (~1.5 us), the closest to the profiler's dispatch duration; 0 when not applicable.
// kernel_kind / epi_ran: which kernel and epilogue the timed launches really were (0 gemm_bf16_nt_kernel, 1 gemm256_..., 2
// gemm256p_...; the EPI_* number).
static int encode_probe(const clipmi_tower* t, const void* blob_dev, const void* pixels_dev, int pix_dtype, int B, float* out_dev,
                        void* ws_dev, size_t ws_bytes, void* stream, int probe_epi, int reps, int nmodes, float* ms, int* launches,
                        int* kernel_kind, int* epi_ran) {
    if (!ms || reps < 1) return set_err(CLIPMI_EINVAL, "dbg_encode_image_probe_ms: bad arguments");
    // probe_epi bits 8..: only launches with this K (out_proj and c_proj share the residual epilogue and differ in K); 0 = any
    const int k_filter = probe_epi >> 8;
    probe_epi &= 0xff;
    GemmProbe p;             // lives on this call's stack: the library keeps no mutable state (clipmi.h)
    for (int i = 0; i < 2 * GemmProbe::MAX; ++i)
        if (hipEventCreate(&p.ev[i]) != hipSuccess) return set_err(CLIPMI_EHIP, "hipEventCreate");
    for (int i = 0; i < GemmProbe::MAX; ++i)
        if (hipEventCreate(&p.pre[i]) != hipSuccess) return set_err(CLIPMI_EHIP, "hipEventCreate");
    int rc = 0;
    for (int mode = 0; mode < nmodes && rc == 0; ++mode) {
        double total = 0.0;
        int count = 0;
        for (int r = 0; r < reps && rc == 0; ++r) {
            p.epi = probe_epi; p.n = 0; p.mode = mode;
            rc = encode_image_impl(t, blob_dev, pixels_dev, pix_dtype, B, out_dev, 1, ws_dev, ws_bytes, stream, &p);
            if (rc) break;
            if (hipStreamSynchronize(as_stream(stream)) != hipSuccess) { rc = set_err(CLIPMI_EHIP, "hipStreamSynchronize"); break; }
            for (int i = 0; i < p.n; ++i) {
                if (GemmProbe::base_of(p.epi_of[i]) != probe_epi || (k_filter && p.k_of[i] != k_filter)) continue;
                float v = 0.f;
                if (mode == 0) (void)hipEventElapsedTime(&v, p.ev[2 * i], p.ev[2 * i + 1]);
                else if (mode == 1) (void)hipEventElapsedTime(&v, p.pre[i], p.ev[2 * i + 1]);
                else {
                    // the launch in front must carry its own end stamp with NO kernel between them: the residual producer in front
                    // of qkv / c_fc, c_fc in front of c_proj, attention (probed in this mode) in front of out_proj
                    if (i == 0 || p.kernel_of[i - 1] != 2 ||
                        (p.epi_of[i - 1] != EPI_BIAS_RESID_LN_F32 && p.epi_of[i - 1] != EPI_LN_BIAS_QGELU_BF16 &&
                         p.epi_of[i - 1] != GemmProbe::EPI_ATTENTION)) continue;
                    (void)hipEventElapsedTime(&v, p.ev[2 * (i - 1) + 1], p.ev[2 * i + 1]);
                }
                total += v;
                ++count;
                if (kernel_kind) *kernel_kind = p.kernel_of[i];
                if (epi_ran) *epi_ran = p.epi_of[i];
            }
        }
        if (rc == 0 && count == 0 && mode == 0) rc = set_err(CLIPMI_EINVAL, "dbg_encode_image_probe_ms: no launch matched epi %d", probe_epi);
        if (rc == 0) { ms[mode] = count ? (float)(total / count) : 0.f; if (launches && mode == 0) *launches = count; }
    }
    for (int i = 0; i < 2 * GemmProbe::MAX; ++i) (void)hipEventDestroy(p.ev[i]);
    for (int i = 0; i < GemmProbe::MAX; ++i) (void)hipEventDestroy(p.pre[i]);
    return rc;
}

extern "C" int clipmi_dbg_encode_image_probe_ms(const clipmi_tower* t, const void* blob_dev, const void* pixels_dev,
                                                int pix_dtype, int B, float* out_dev, void* ws_dev, size_t ws_bytes,
                                                void* stream, int probe_epi, int reps, float* kernel_ms, int* launches) {
    return encode_probe(t, blob_dev, pixels_dev, pix_dtype, B, out_dev, ws_dev, ws_bytes, stream, probe_epi, reps, 1, kernel_ms,
                        launches, nullptr, nullptr);
}

extern "C" int clipmi_dbg_encode_image_probe3_ms(const clipmi_tower* t, const void* blob_dev, const void* pixels_dev,
                                                 int pix_dtype, int B, float* out_dev, void* ws_dev, size_t ws_bytes,
                                                 void* stream, int probe_epi, int reps, float* ms3, int* launches,
                                                 int* kernel_kind, int* epi_ran) {
    return encode_probe(t, blob_dev, pixels_dev, pix_dtype, B, out_dev, ws_dev, ws_bytes, stream, probe_epi, reps, 3, ms3,
                        launches, kernel_kind, epi_ran);
}
