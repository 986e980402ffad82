/*
 * clipmi.h — C ABI of libclipmi.so, the MI355X (gfx950) CLIP index-and-search hot path.
 *
 * The reference (ps-auxw/CLI-P) has no FFI of its own: its "interface" for this path is the
 * set of Python calls its two scripts make on third-party objects. Each entry
 * point below names the reference call site it stands in for, as `file:line` under the
 * reference tree. The Python mirror of those call shapes lives in `cli-p_amd/`; the binding a
 * maintainer would add to the reference scripts is shown in INTEGRATION.md.
 *
 * Contract for every entry point:
 *   - plain C types only; every `*_dev` pointer is a DEVICE (HBM) pointer owned by the caller;
 *   - the library never allocates, frees or synchronises: all work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream) and is graph-capturable;
 *   - scratch memory is a caller-owned workspace whose size the matching *_workspace_bytes()
 *     function returns (0 from that function = unsupported arguments, see clipmi_last_error);
 *   - what a workspace, scratch rows and every output hold on entry is arbitrary - a call reads nothing of them that it has
 *     not written itself, so one workspace may serve calls of any size one after the other without being cleared -, and
 *     `status_dev[i]` is written for every image of the call, 0 included (tests/ws_cases.py has the table, region by region);
 *   - return value 0 = enqueued; non-zero = a CLIPMI_E* code, nothing was enqueued (or, for
 *     CLIPMI_EHIP, a launch failed); the message is in clipmi_last_error() (thread-local);
 *   - re-entrant: no global mutable state apart from that thread-local error string.
 */
#ifndef CLIPMI_H
#define CLIPMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLIPMI_ABI_VERSION 8

enum {
    CLIPMI_OK = 0,
    CLIPMI_EINVAL = 1,   /* bad argument (shape, dtype, NULL pointer, K out of range ...) */
    CLIPMI_EWORKSPACE = 2, /* workspace too small */
    CLIPMI_EHIP = 3,     /* a HIP call failed */
    CLIPMI_EUNSUPPORTED = 4
};

/* element types of buffers crossing the ABI */
enum {
    CLIPMI_F32 = 0,
    CLIPMI_BF16 = 1,
    CLIPMI_U8 = 2,
    CLIPMI_F16 = 3   /* IEEE binary16, little-endian; as clipmi_topk_ip's / clipmi_topk_ip_rows' db_dtype: [N][E] row-major,
                        row pitch 2 E bytes (an addition to ABI 8 in the sense of the PNG note below: one newly accepted
                        argument value and two new entry points, nothing existing changes, CLIPMI_ABI_VERSION stays 8) */
};

/*
 * One transformer tower (vision or text) as a POD view into ONE packed device blob.
 * Produced on the host by the packer (cli-p_amd/weights.py) from tensors with OpenAI CLIP
 * state-dict names (SURVEY.md §8b "weight-file contract"); replaces the model object that
 * `clip.load("ViT-B/32", device=device, jit=False)` returns (build-index.py:18,
 * query-index.py:21). All offsets are bytes from the blob base, 256-byte aligned.
 * GEMM weights are bf16, row-major [out_features][in_features] (PyTorch Linear layout, so the
 * contraction index is contiguous for both operands); LayerNorm parameters, biases and
 * embeddings are f32.
 */
typedef struct clipmi_tower {
    int32_t abi_version;   /* CLIPMI_ABI_VERSION */
    int32_t kind;          /* 0 = vision, 1 = text */
    int32_t width;         /* W: 768 (ViT-B/32 vision), 512 (text) */
    int32_t layers;
    int32_t heads;         /* W / 64 */
    int32_t mlp;           /* 4 W */
    int32_t embed;         /* E: 512 */
    int32_t tokens;        /* L: 50 for ViT-B/32 (49 patches + CLS); 77 for text */
    /* vision only */
    int32_t patch;         /* P: 32 */
    int32_t res;           /* R: 224 */
    int32_t patch_k;       /* 3*P*P rounded up to a multiple of 64 (zero-padded columns) */
    /* text only */
    int32_t vocab;         /* 49408 */

    uint64_t blob_bytes;

    /* vision: conv1.weight as bf16 [W][patch_k]; class_embedding f32 [W];
       positional_embedding f32 [L][W]; ln_pre f32 */
    uint64_t off_patch_w, off_cls, off_pos, off_ln_pre_w, off_ln_pre_b;
    /* text: token_embedding.weight f32 [vocab][W]; positional_embedding uses off_pos */
    uint64_t off_tok_emb;

    /* per layer l: base = off_layers + l * layer_stride, then the intra-layer offsets */
    uint64_t off_layers, layer_stride;
    uint64_t lo_ln1_w, lo_ln1_b;      /* f32 [W] */
    uint64_t lo_qkv_w, lo_qkv_b;      /* attn.in_proj_weight bf16 [3W][W], in_proj_bias f32 [3W] */
    uint64_t lo_out_w, lo_out_b;      /* attn.out_proj bf16 [W][W], f32 [W] */
    uint64_t lo_ln2_w, lo_ln2_b;
    uint64_t lo_fc_w, lo_fc_b;        /* mlp.c_fc bf16 [4W][W], f32 [4W] */
    uint64_t lo_proj_w, lo_proj_b;    /* mlp.c_proj bf16 [W][4W], f32 [W] */

    /* vision: ln_post + visual.proj stored TRANSPOSED as bf16 [E][W];
       text: ln_final + text_projection stored TRANSPOSED as bf16 [E][W] */
    uint64_t off_ln_post_w, off_ln_post_b, off_out_proj;

    /* ABI 2. weight_format 0: the four linear layers of every block are bf16 (above). weight_format 1
       (BASELINE.json configs[4], FP8 matrix cores): lo_qkv_w / lo_out_w / lo_fc_w / lo_proj_w point at OCP e4m3
       bytes [out_features][in_features] and lo_*_s at f32 [out_features] per-output-channel scales
       (weight = scale * e4m3 value). Activations travel as e4m3 with MX block scales (one e8m0 scale 2^(e-7) per 32
       consecutive values of a row, written by the producing kernel: attention, the QuickGELU GEMM) or, where a producer
       sees whole rows (LayerNorm), with one f32 scale per row. Needs width % 256 == 0. */
    int32_t weight_format, ln_fold;
    uint64_t lo_qkv_s, lo_out_s, lo_fc_s, lo_proj_s;

    /* ABI 3. ln_fold = 1 (weight_format 0, width % 256 == 0): ln_1 / ln_2 are folded into the GEMMs that consume
       them. With mean / rstd the row statistics of the residual row x,
           LayerNorm(x; g, b) W^T + bias = rstd * (x Wg^T - mean * colsum) + cb,
       Wg = W diag(g) (lo_qkv_w / lo_fc_w then hold Wg, rounded to bf16 once), colsum[n] = sum_k Wg[n][k],
       cb[n] = sum_k b[k] W[n][k] + bias[n] (W = the bf16-rounded plain weights; sums in float64, stored f32 [3W] / [4W]).
       The residual stream is kept split x = hi + lo (two bf16 arrays); hi is the GEMM operand, the residual GEMM's
       store pass updates hi / lo and the statistics, and no stand-alone LayerNorm pass over the stream remains. */
    uint64_t lo_qkv_colsum, lo_qkv_cb, lo_fc_colsum, lo_fc_cb;
} clipmi_tower;

/* ---- a3/a4: model.encode_image(image) and the row L2-normalise that follows it ----------
 * Replaces build-index.py:49 (`model.encode_image(image)`) and, with normalize != 0,
 * build-index.py:50 (`image_features / image_features.norm(dim=-1, keepdim=True)`).
 *   pixels_dev : [B][3][R][R], NCHW. CLIPMI_F32 / CLIPMI_BF16 = already normalised (the output
 *                of the reference `transform`, build-index.py:48); CLIPMI_U8 = raw 0..255 RGB,
 *                the /255, -mean, /std of CLIP's transform is fused into the patch kernel.
 *   out_dev    : f32 [B][E] (the layout build-index.py:51 serialises: 2048 B per row for E=512)
 */
size_t clipmi_encode_image_workspace_bytes(const clipmi_tower* t, int B);
int clipmi_encode_image(const clipmi_tower* t, const void* blob_dev,
                        const void* pixels_dev, int pix_dtype, int B,
                        float* out_dev, int normalize,
                        void* ws_dev, size_t ws_bytes, void* stream);

/* ---- a9/a10: model.encode_text(texts) + normalize() -------------------------------------
 * Replaces query-index.py:108 (`model.encode_text(texts)`; `normalize`, query-index.py:13-17,
 * when normalize != 0 — per ROW here; identical to the reference for its Q = 1).
 *   ids_dev : int32 [Q][L] token ids as produced by clip.tokenize (query-index.py:107);
 *             the pooled row is the first argmax of each row (the EOT token).
 *   out_dev : f32 [Q][E]
 */
size_t clipmi_encode_text_workspace_bytes(const clipmi_tower* t, int Q);
int clipmi_encode_text(const clipmi_tower* t, const void* blob_dev,
                       const int32_t* ids_dev, int Q,
                       float* out_dev, int normalize,
                       void* ws_dev, size_t ws_bytes, void* stream);

/* ---- a12: index.search(features, k + offset + 1) ----------------------------------------
 * Replaces query-index.py:111 (`D, I = index.search(features, K)`), as EXACT flat inner-product
 * search over this rank's shard of the packed matrix that build-index.py:68-107 assembles.
 *   db_dev     : [N][E] row-major (E in {512, 768}), CLIPMI_F32, or CLIPMI_F16: binary16 rows of pitch 2 E bytes, as
 *                clipmi_rows_to_f16 writes them (half the bytes per pass). Every other db_dtype is
 *                CLIPMI_EUNSUPPORTED. With CLIPMI_F16 everything below holds word for word ON THE ROWS' VALUES CONVERTED TO
 *                F32, which is exact (subnormals included; +-inf and NaN components as in f32 rows): the same fmaf chain, the
 *                same plan and workspace (clipmi_topk_ip_workspace_bytes has no dtype argument), the same ordering and pads.
 *   q_dev      : f32 [Q][E]
 *   out_score  : f32 [Q][K] descending; out_id: int64 [Q][K] = id_base + row; ties broken by
 *                ascending id; slots beyond min(K, N) hold score -FLT_MAX and id -1
 *   Scores are bit-exact f32: for each (row, query) one fmaf chain in the fixed order
 *   documented in DESIGN.md ("score order") and restated in oracle/topk_oracle.c.
 *   K range: 1 <= K <= 8128 at E = 512, 1 <= K <= 7104 at E = 768, whatever N and Q (one query's K + 16 candidate
 *   slots and as many of scratch must fit in LDS beside the query image, which is wider at 768). A larger K is
 *   CLIPMI_EINVAL and a workspace size of 0; the coarse and wide entry points below accept the same range.
 *   clipmi_merge_topk takes R * K <= 13609 (one LDS pass): eight shards merge on the device up to K = 1701.
 */
size_t clipmi_topk_ip_workspace_bytes(int64_t N, int E, int Q, int K);
int clipmi_topk_ip(const void* db_dev, int db_dtype, int64_t N, int E,
                   const float* q_dev, int Q, int K, int64_t id_base,
                   float* out_score_dev, int64_t* out_id_dev,
                   void* ws_dev, size_t ws_bytes, void* stream);

/* ---- a12 over a chosen subset of the rows (an addition to ABI 8 in the sense of the PNG note below: two new entry points,
 * nothing existing changes, CLIPMI_ABI_VERSION stays 8). clipmi_topk_ip_rows is clipmi_topk_ip's result restricted to the
 * rows `rows_dev` names, reading only those rows (M * E * 4 + M * 4 bytes per pass of <= 32 queries instead of N * E * 4).
 *   rows_dev : u32 [M] row numbers of db_dev, strictly ascending. 0 <= M <= N; NULL with M > 0, M < 0 and M > N are
 *              CLIPMI_EINVAL, a db_dtype other than CLIPMI_F32 and CLIPMI_F16 (as in clipmi_topk_ip: M * E * 2 bytes of rows
 *              per pass) is CLIPMI_EUNSUPPORTED - all decided on the host, nothing is launched.
 *              M = 0 fills the outputs with pads and reads nothing.
 *   result   : scores bit-exact (the same MFMA sequence per (row, query): DESIGN.md "score order"), ordered by descending
 *              score, then ascending ROW ID; out_id = id_base + row; slots beyond min(K, M) hold (-FLT_MAX, -1). Non-finite
 *              rows and queries as in clipmi_topk_ip (a NaN score is never selected). E, the K range, asynchrony, "no
 *              allocation, no synchronisation" and workspace independence as there; the workspace is clipmi_topk_ip's for M rows.
 *   safety   : the list is not validated on the device, but whatever it holds the kernels form no address outside
 *              db_dev[0 .. N): an entry >= N is skipped - never addressed, never published, as if it were absent. A
 *              DUPLICATE entry is not checked either: it is a second candidate with the same (score, id), which the
 *              selects' rank counting (distinct keys assumed) may return once, twice or - at a list boundary - in place of
 *              a neighbour; memory-safe, but outside the contract. So is a list that is not ascending: the result is still the
 *              exact top-K of the listed rows (ordering is by row id, not by list position), only the pre-pass then samples
 *              the first list entries rather than the lowest rows. */
size_t clipmi_topk_ip_rows_workspace_bytes(int64_t M, int E, int Q, int K);
int clipmi_topk_ip_rows(const void* db_dev, int db_dtype, int64_t N, int E,
                        const uint32_t* rows_dev, int64_t M,
                        const float* q_dev, int Q, int K, int64_t id_base,
                        float* out_score_dev, int64_t* out_id_dev,
                        void* ws_dev, size_t ws_bytes, void* stream);

/* ---- a12, coarse-then-exact variant: the same exact result (bit-exact scores, same ordering rule) from a
 * bf16 coarse scan of `db_bf16_dev` (the matrix rounded to bf16, [N][E]) that keeps a provable superset,
 * followed by exact f32 re-scoring of the survivors from `db_dev` (DESIGN.md "coarse path"). Half the HBM
 * bytes per pass and 64 queries per pass. `rmax` = an upper bound of the largest row L2 norm of db_dev.
 * E = 512 or 768, N >= 65536 (anything else: CLIPMI_EUNSUPPORTED, a workspace size of 0); if a candidate list overflows,
 * the exact scan runs as a device-side fallback. More than 64 queries are taken as 64-query passes inside the call. */
size_t clipmi_topk_ip_coarse_workspace_bytes(int64_t N, int E, int Q, int K);
int clipmi_topk_ip_coarse(const void* db_dev, const void* db_bf16_dev, int64_t N, int E, float rmax,
                          const float* q_dev, int Q, int K, int64_t id_base,
                          float* out_score_dev, int64_t* out_id_dev,
                          void* ws_dev, size_t ws_bytes, void* stream);

/* ---- a12, int8 coarse copy: the same contract with a quarter of the f32 bytes per pass.
 * clipmi_quantize_rows_i8 builds the copy (E a multiple of 32). Rows are taken in blocks of 32 that share one scale
 * s = (largest |x| of the block) / 127; q_rk = rint(x_rk / s). `out_i8_dev` (clipmi_i8_copy_bytes) holds the blocks as
 * [E / 32][64][16 bytes] - entry (k-step s, lane l) = bytes 32 s + 16 (l >> 5) .. + 15 of row (l & 31) of the block, the
 * register image of v_mfma_i32_32x32x32_i8's row operand, so a scanning wave reads whole contiguous KiB; rows past N in
 * the last block are zero. `meta_dev` (clipmi_i8_meta_bytes) receives meta[r] = (s, a_r) with a_r >= ||x_r - s q_r||_2
 * for N rounded up to 32 rows (+32), followed by one (s, largest a_r) pair per block and one u32 per slot: the row it holds.
 * clipmi_topk_ip_coarse_i8 scans the copy with integer MFMA (exact integer dot products) and keeps every row whose exact
 * score could reach the running K-th best, by |x.y - s t_q D| <= a_r ||y|| + (rmax + amax) ||y - t_q p_q||; survivors are
 * re-scored in exact f32 as above. `amax` >= every a_r, `rmax` >= every row norm. Up to 64 queries are one pass of the
 * copy (v_mfma_i32_16x16x64_i8, HBM-bound); MORE than 64 queries (query-index.py:111 is one call whatever Q) are taken
 * in chunks of <= 1024 as ONE pass each at E = 512 (v_mfma_i32_32x32x32_i8, query tiles of 256 resident in LDS,
 * matrix-bound); at E = 768, where such a tile (192 KiB) does not fit in LDS, as 64-query passes one after the other inside
 * the call (a caller that wants them overlapped enqueues 64-query calls on two streams, as IndexFlatIP does).
 * E = 512 or 768, N >= 65536. Workspace: clipmi_topk_ip_coarse_workspace_bytes. */
/* Build-side helpers of the coarse copies (index load: query-index.py:60-75 reads every vector once and keeps the
 * matrix). clipmi_rows_stats writes stats2_dev[0] = the largest row norm of db (f64 accumulation, rounded up: a valid
 * `rmax`) and stats2_dev[1] = the largest a_r of an int8 copy's meta (`meta_dev` may be NULL: 0). clipmi_rows_to_bf16
 * writes the bf16 copy (round to nearest even) clipmi_topk_ip_coarse scans. E a multiple of 4. Asynchronous on `stream`. */
int clipmi_rows_stats(const float* db_dev, int64_t N, int E, const float* meta_dev, float* stats2_dev, void* stream);
int clipmi_rows_to_bf16(const float* db_dev, int64_t N, int E, void* out_bf16_dev, void* stream);
/* The CLIPMI_F16 matrix of an index kept in fp16 (an addition to ABI 8, see CLIPMI_F16): out_f16_dev[N][E] = db_dev rounded to
 * the nearest binary16, ties to even; finite values of magnitude >= 65520 become +-inf, the sign of zero is kept, NaN stays NaN.
 * counts2_dev is NULL or two u64 the call ADDS to (the caller zeroes them): [0] += elements whose value changed
 * (f32(f16(x)) != x; a NaN that stays NaN is not counted), [1] += finite elements that became infinite. E a multiple of 4.
 * Asynchronous on `stream`. */
int clipmi_rows_to_f16(const float* db_dev, int64_t N, int E, void* out_f16_dev, uint64_t* counts2_dev, void* stream);
size_t clipmi_i8_copy_bytes(int64_t N, int E);
size_t clipmi_i8_meta_bytes(int64_t N);
/* (ABI 4: the two buffer sizes are arguments - a copy or meta buffer smaller than clipmi_i8_copy_bytes / clipmi_i8_meta_bytes
 *  is refused with CLIPMI_EINVAL instead of written past.
 *  ABI 4, `perm_dev`: NULL, or a permutation of 0 .. N-1 (u32 [N]): slot t of the copy then holds row perm[t]. Order the rows by
 *  their largest |component| (clipmi_rows_absmax + any sort) and the 32 rows of a block share a scale that is nearly each
 *  row's own: error norms and with them the re-scored rows per query drop ~12 %. The search is exact for ANY permutation; it
 *  reports row ids - the meta buffer carries the slot -> row table behind the block meta.
 *  `perm_dev` is NOT validated (a check would need a pass and memory of its own): entries >= N become empty slots (memory-safe),
 *  duplicate or missing rows silently drop rows from every coarse search. Build it with clipmi_rows_order_by_absmax below, which
 *  returns a permutation by construction.) */
int clipmi_quantize_rows_i8(const float* db_dev, int64_t N, int E, const uint32_t* perm_dev, void* out_i8_dev, size_t out_i8_bytes,
                            float* meta_dev, size_t meta_bytes, void* stream);
/* out_dev[r] = largest |x_rk| of row r (f32 [N]); E a multiple of 4. Asynchronous on `stream`.
 * NaN components are skipped (the maximum is taken with fmaxf): a row of NaN and finite values gives its largest finite
 * |x|, NaN beside +-inf gives +inf, a row of NaN only gives 0. */
int clipmi_rows_absmax(const float* db_dev, int64_t N, int E, float* out_dev, void* stream);
/* perm_dev[t] (u32 [N]) = the row that belongs in slot t of the int8 copy: the rows ordered by their largest |component|,
 * ascending, equal maxima in row order (a stable radix sort of clipmi_rows_absmax's values on the device; no framework sort is
 * needed to build the sorted copy). `ws_dev`: clipmi_rows_order_workspace_bytes(N) bytes. Asynchronous on `stream`; pass the
 * result to clipmi_quantize_rows_i8 as `perm_dev`. Replaces nothing in the reference (its IVF lists have no such order); the
 * index-load site is query-index.py:29. */
size_t clipmi_rows_order_workspace_bytes(int64_t N);
int clipmi_rows_order_by_absmax(const float* db_dev, int64_t N, int E, uint32_t* perm_dev, void* ws_dev, size_t ws_bytes, void* stream);
int clipmi_topk_ip_coarse_i8(const void* db_dev, const void* db_i8_dev, const float* meta_dev, float amax,
                             int64_t N, int E, float rmax, const float* q_dev, int Q, int K, int64_t id_base,
                             float* out_score_dev, int64_t* out_id_dev,
                             void* ws_dev, size_t ws_bytes, void* stream);
/* ---- ABI 8. The same search with a ONE-PASS wide scan at E = 768 as well - opt-in: clipmi_topk_ip_coarse_i8 and its workspace
 * function keep their behaviour byte for byte. Arguments, contract (asynchronous, no allocation, exact for any data and any row
 * permutation, exact fallback when a list overflows) and results are those of clipmi_topk_ip_coarse_i8.
 * "Any data" includes any magnitude: the norms of the coarse bounds (||y||, ||f_q||, a_r, rmax) are f64 sums of squares rounded
 * up, and a query or database whose largest |component|, rmax or rmax ||y|| lies outside [2^-110, 2^110 (2^120 for the product)]
 * - bf16 copy: below 2^-90 - has no coarse bound: every row is re-scored or the exact fallback answers (DESIGN.md 4.1m;
 * tests/test_topk_magnitude_gpu.py holds all four search entries to the oracle from 2^-126 to 2^100).
 * E = 512, or Q <= 64: it IS that function, and the workspace size is clipmi_topk_ip_coarse_workspace_bytes'.
 * E = 768, Q > 64: chunks of <= 1024 queries, each ONE pass of the copy on `stream` (v_mfma_i32_32x32x32_i8, 24 k-steps, query
 * tiles of 128 = 96 KiB resident in LDS, four-wave workgroups); the workspace is the larger of the 64-query one and the wide
 * pass's for min(Q, 1024) queries. Returns 0 / CLIPMI_EUNSUPPORTED under the conditions of the functions above. */
size_t clipmi_topk_ip_wide_workspace_bytes(int64_t N, int E, int Q, int K);
int clipmi_topk_ip_wide_i8(const void* db_dev, const void* db_i8_dev, const float* meta_dev, float amax,
                           int64_t N, int E, float rmax, const float* q_dev, int Q, int K, int64_t id_base,
                           float* out_score_dev, int64_t* out_id_dev,
                           void* ws_dev, size_t ws_bytes, void* stream);

/* ---- multi-GPU merge of per-shard partial results (no reference counterpart: the reference
 * is single-process). Inputs are R lists per query as gathered by one
 * all-gather: scores f32 [R][Q][K], ids int64 [R][Q][K] (id -1 = empty slot). Same ordering
 * rule (score desc, id asc), so the result equals single-GPU exact top-K.
 */
size_t clipmi_merge_topk_workspace_bytes(int R, int Q, int K);
int clipmi_merge_topk(const float* scores_dev, const int64_t* ids_dev, int R, int Q, int K,
                      float* out_score_dev, int64_t* out_id_dev,
                      void* ws_dev, size_t ws_bytes, void* stream);

/* The same merge over the buffer ONE all-gather yields when every rank contributes a packed record
 * [scores f32 Q*K | pad to 8 B | ids int64 Q*K] of record_bytes (a multiple of 8): rank r's record is at
 * gathered_dev + r * record_bytes. Lets the N>1 search path be: top-k -> one collective -> merge. */
int clipmi_merge_topk_packed(const void* gathered_dev, size_t record_bytes, int R, int Q, int K,
                             float* out_score_dev, int64_t* out_id_dev, void* stream);

/* ---- a4/a10 stand-alone: rows of x[n][E] scaled to unit L2 norm in place (rows with
 * norm < 1e-9 are left unchanged, as query-index.py:13-17 does). */
int clipmi_l2_normalize_rows(float* x_dev, int64_t n, int E, void* stream);

/* ---- a2 on the device: Pillow's bicubic resize (shorter side -> n_px) + centre crop of 8-bit RGB images that were
 * shipped at full size, bit for bit what `transform(image)` computes before its float tail (build-index.py:48; Pillow's
 * two-pass 8-bit resampling with 22-bit integer coefficients). The host supplies, per image, a job record and the integer
 * coefficient blocks of the n_px outputs per axis that survive the crop ([n_px] first tap | [n_px] tap count | [n_px][k]
 * coefficients, int32): cli-p_amd/decode_worker.py computes them with Pillow's own float64 formula.
 * raw_dev: the images, HWC bytes at job.src_off; out_dev: uint8 [.][3][n_px][n_px] (block job.out_index);
 * scratch_dev: the 8-bit intermediate rows, job.tmp_off + nrows*n_px*3 bytes each; max_rows = the largest job.nrows. */
typedef struct clipmi_resize_job {
    int64_t src_off;              /* bytes from raw_dev to the image's first pixel (rows of w*3 bytes) */
    int32_t w, h;                 /* source size */
    int32_t r0, nrows;            /* source rows [r0, r0 + nrows) the output window needs */
    int32_t out_index;
    int32_t need_h, need_v;       /* 0: that axis is not resampled (source size == target size), only cropped */
    int32_t left, top;            /* window origin on an axis that is not resampled */
    int32_t hk, vk;               /* taps per output of the horizontal / vertical coefficient block */
    int64_t hcoef_off, vcoef_off; /* int32 offsets into coef_dev */
    int64_t tmp_off;              /* bytes into scratch_dev */
} clipmi_resize_job;
int clipmi_resize_crop_rgb8(const void* raw_dev, const void* jobs_dev, int njobs, int max_rows, const int32_t* coef_dev,
                            int n_px, void* out_dev, void* scratch_dev, void* stream);

/* ---- `Image.open(tfn)` on the device for baseline JPEG files (build-index.py:47, the decode in front of `transform` at :48;
 * SURVEY.md §8(f) next-1): the bytes Pillow (libjpeg-turbo: Huffman decode, jpeg_idct_islow, fancy upsampling, 16-bit
 * fixed-point YCbCr -> RGB) hands to the transform, bit for bit. The HOST walks the markers (cli-p_amd/jpeg.py) and lets through
 * 8-bit baseline / extended-sequential Huffman files with one interleaved scan, 1 (grey) or 3 (YCbCr) components, luma sampling
 * 1x1, 2x1 or 2x2 with 1x1 chroma, with or without restart intervals; everything else stays with Pillow. Per image one record; the
 * entropy-coded segments travel with the 0xFF00 stuffing removed, each 4-byte aligned and followed by at least 16 zero bytes.
 * tables_dev: the batch's distinct Huffman tables, 288 bytes each (DHT's 16 counts + up to 256 symbols, zero padded to 272,
 * then the table class - 0 DC, 1 AC - and 15 zero bytes).
 * out_dev: per image height rows of width*3 RGB bytes at out_off (grey files replicated, as Image.convert("RGB") does) - the
 * layout clipmi_resize_crop_rgb8 takes. status_dev[i]: 0 decoded; 1 invalid Huffman code; 2 the data ended early or ran
 * over; 3 a marker inside a segment handed over with its stuffing; 4 a block outside the range where libjpeg-turbo's IDCT equals
 * the device's (a dequantised coefficient or pass-1 value beyond int16, an output beyond [-512, 511]) - such a file goes back to Pillow, whose error handling is the reference's. total_blocks = sum of the images' 8x8 blocks
 * (coef_off counts in blocks), max_blocks / max_pixels = the largest image's.
 * Further layouts (an addition to ABI 8 in the sense of the PNG note below: no new entry point, no new struct, a caller that
 * writes 0 into `reserved` gets what it got before, CLIPMI_ABI_VERSION stays 8): the records of this entry and of the progressive
 * one may also name luma sampling 1x2 (4:4:0, libjpeg-turbo's h1v2_fancy_upsample), 4x1 (4:1:1) or 1x4 (replication), and a colour
 * transform of "none" for the three-component files libjpeg takes for RGB-coded - the host lets those through where its caller opts
 * in (jpeg_parse.parse(layouts=True)). A record with other sampling factors, another transform or a size below 1 is reported with
 * status 1 and nothing of it is decoded. Such a record comes back EMPTIED in images_dev: beside `stuffed` and `stream_bytes`, which
 * the device rewrites in any record it unstuffs, a refused record has width, height, stream_bytes, restart_interval, n_intervals,
 * stuffed and reserved set to 0 and ncomp, hs, vs set to 1 (an empty grey image, which gives the later kernels nothing to do). The
 * progressive entry does not write to its records. */
typedef struct clipmi_jpeg_image {
    int64_t stream_off;           /* bytes from streams_dev */
    int64_t coef_off;             /* the image's first block in the workspace's coefficient / sample buffers */
    int64_t out_off;              /* bytes from out_dev */
    int64_t intervals_off;        /* restart intervals: bytes from streams_dev to n_intervals uint32 byte offsets into the segment */
    int32_t stream_bytes;
    int32_t width, height;
    int32_t ncomp;                /* 1 or 3 */
    int32_t hs, vs;               /* luma sampling factors (1,1) (2,1) (2,2), and (1,2) (4,1) (1,4); chroma is 1x1 */
    int32_t dc_tbl[3], ac_tbl[3]; /* per component: index into tables_dev */
    int32_t restart_interval;     /* MCUs per restart interval (DRI), 0 = none */
    int32_t n_intervals;          /* ceil(MCUs / restart_interval); the RSTn markers themselves are removed from the segment */
    int32_t stuffed;              /* 1: the segment still holds the 0xFF00 byte stuffing (no restart intervals then) - the device
                                     removes it IN PLACE and rewrites stream_bytes and this field (0 done, 2 marker inside the scan) */
    int32_t reserved;             /* colour transform: 0 = YCbCr -> RGB as before, 1 = none (components are R, G, B) */
    uint8_t quant[3][64];         /* per component: quantisation steps, natural (row-major) order */
} clipmi_jpeg_image;
int64_t clipmi_jpeg_workspace_bytes(int64_t total_blocks, int ntables);
int clipmi_jpeg_decode_rgb8(void* streams_dev, void* images_dev, int n, const void* tables_dev, int ntables,
                            int64_t total_blocks, int64_t max_blocks, int64_t max_pixels, void* out_dev, int32_t* status_dev,
                            void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- Four-component JPEG files, CMYK as stored and YCCK (an addition to ABI 8 in the sense of the PNG note below: two new entry
 * points - this one and clipmi_resize_crop_cmyk8 - and one new record, nothing existing changes, CLIPMI_ABI_VERSION stays 8).
 * clipmi_jpeg_decode_cmyk8 takes clipmi_jpeg_decode_rgb8's argument list over clipmi_jpeg_image4 records: clipmi_jpeg_image with
 * four table indices of each class, four rows of quantisation steps and the colour transform in `reserved` - 2 = CMYK as stored (a
 * file without an Adobe marker, or with Adobe transform 0), 3 = YCCK (Adobe transform 2). The host lets through, where its caller
 * opts in (jpeg_parse.parse(cmyk=True)), 8-bit baseline / extended-sequential Huffman files with one interleaved scan of four
 * components, components 1-3 sampled 1x1 and component 0 at one of the luma samplings above. Still Pillow's: progressive
 * four-component files, Adobe transform 1, a file whose component 3 is sampled like component 0 (IJG's own YCCK default of
 * 2x2,1x1,1x1,2x2), and anything above the parser's size caps.
 * out_dev: per image, at out_off (4-byte aligned for full store width; any offset works), height rows of width*4 bytes - what
 * np.asarray(Image.open(f)) holds for such a file, mode CMYK. With p0..p3 the four decoded, upsampled samples (components 1-3
 * upsampled as chroma is): transform 2 gives (255-p0, 255-p1, 255-p2, 255-p3); transform 3 gives (R, G, B, 255-p3) with R, G, B
 * the YCbCr -> RGB conversion of (p0, p1, p2) above. The layout clipmi_resize_crop_cmyk8 takes.
 * Workspace: clipmi_jpeg_workspace_bytes(total_blocks, ntables) with an image's blocks counted at hs*vs + 3 per MCU. status_dev:
 * 0-4 as clipmi_jpeg_decode_rgb8. A record with ncomp != 4, other sampling factors, a transform other than 2 / 3 or a size below
 * 1 is reported with status 1, nothing of it is decoded, and it comes back emptied as a refused clipmi_jpeg_image does. The fused
 * entries (clipmi_jpeg_decode_transform_rgb8 ...) do not take four components: ncomp = 4 in their records is status 1. */
typedef struct clipmi_jpeg_image4 {
    int64_t stream_off, coef_off, out_off, intervals_off;     /* as clipmi_jpeg_image */
    int32_t stream_bytes;
    int32_t width, height;
    int32_t ncomp;                /* 4 */
    int32_t hs, vs;               /* sampling factors of component 0; components 1-3 are 1x1 */
    int32_t dc_tbl[4], ac_tbl[4]; /* per component: index into tables_dev */
    int32_t restart_interval, n_intervals, stuffed;           /* as clipmi_jpeg_image */
    int32_t reserved;             /* colour transform: 2 = CMYK as stored, 3 = YCCK */
    uint8_t quant[4][64];         /* per component: quantisation steps, natural (row-major) order */
} clipmi_jpeg_image4;
int clipmi_jpeg_decode_cmyk8(void* streams_dev, void* images_dev, int n, const void* tables_dev, int ntables,
                             int64_t total_blocks, int64_t max_blocks, int64_t max_pixels, void* out_dev, int32_t* status_dev,
                             void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- ABI 7. Progressive JPEG files on the device (SOF2, 8-bit, Huffman): the same bytes as Pillow's `convert("RGB")`, for the
 * files the host parser lets through (cli-p_amd/jpeg_parse.py parse_progressive: grey or YCbCr with luma sampling 1x1, 2x1 or
 * 2x2 and 1x1 chroma, no restart intervals, a scan script libjpeg accepts without a warning and that brings every coefficient of
 * every component to Al = 0 - libjpeg then applies no block smoothing). Per image one record, per scan one record: an image's
 * scans are scans_dev[first_scan .. first_scan + n_scans - 1], in file order (n_scans 1..128). Every scan's entropy-coded
 * segment travels with the 0xFF00 stuffing removed, 4-byte aligned and followed by at least 16 zero bytes. tables_dev: the
 * batch's distinct Huffman tables in the 288-byte form of clipmi_jpeg_decode_rgb8. out_dev, total_blocks, max_blocks,
 * max_pixels: as clipmi_jpeg_decode_rgb8. status_dev[i]: 0 decoded; 1 invalid Huffman code (also: a coefficient behind its
 * band, a refinement value of more than one bit, a record outside the limits above); 2 a scan's data ended early; 3 (not
 * produced: segments arrive unstuffed); 4 a block outside the range where libjpeg-turbo's IDCT equals the device's - as
 * clipmi_jpeg_decode_rgb8, and such a file goes back to Pillow. */
typedef struct clipmi_jpeg_scan {
    int64_t stream_off;           /* bytes from streams_dev */
    int32_t stream_bytes;
    int32_t ncomp;                /* components in the scan, 1..3 (AC scans: 1) */
    int32_t comp[3];              /* frame component indices, increasing */
    int32_t tbl[3];               /* per scan component: index into tables_dev - the DC table of a DC first scan, the AC table of
                                     an AC scan; -1 for a DC refinement (raw bits) */
    int32_t ss, se, ah, al;       /* spectral selection and successive approximation, as in the SOS header */
    int32_t reserved[2];
} clipmi_jpeg_scan;
typedef struct clipmi_jpeg_progressive_image {
    int64_t coef_off;             /* as clipmi_jpeg_image */
    int64_t out_off;
    int32_t width, height;
    int32_t ncomp;                /* 1 or 3 */
    int32_t hs, vs;               /* luma sampling factors (1,1) (2,1) (2,2), and (1,2) (4,1) (1,4); chroma is 1x1 */
    int32_t first_scan;           /* index into scans_dev */
    int32_t n_scans;
    int32_t reserved[5];          /* [0]: colour transform: 0 = YCbCr -> RGB as before, 1 = none (components are R, G, B); [1..4]: 0 */
    uint8_t quant[3][64];         /* per component: quantisation steps, natural (row-major) order */
} clipmi_jpeg_progressive_image;
int64_t clipmi_jpeg_progressive_workspace_bytes(int n, int64_t total_blocks, int ntables);
int clipmi_jpeg_decode_progressive_rgb8(const void* streams_dev, const void* images_dev, int n, const void* scans_dev, int nscans,
                                        const void* tables_dev, int ntables, int64_t total_blocks, int64_t max_blocks,
                                        int64_t max_pixels, void* out_dev, int32_t* status_dev, void* ws_dev, int64_t ws_bytes,
                                        void* stream);

/* ---- Baseline and progressive JPEG files straight to the transform's pixels (a further addition to ABI 8 in the sense of the
 * PNG note below: two new entry points, nothing existing changes). The decode entries above followed by clipmi_resize_crop_rgb8,
 * without the full-size RGB image between them: the colour conversion and the horizontal pass read the decoder's sample planes
 * in the workspace, for the source rows and columns the n_px-wide window needs only, and clipmi_resize_crop_rgb8's vertical pass
 * finishes. The arguments of the decode entries with the transform's in place of out_dev and max_pixels: jobs_dev, max_rows,
 * coef_dev, n_px, out_dev (uint8 [.][3][n_px][n_px], block job.out_index) and scratch_dev as clipmi_resize_crop_rgb8 takes them.
 * Job k belongs to image k; its w and h are the image's; its src_off and the image record's out_off are ignored. Workspace
 * sizes: clipmi_jpeg_workspace_bytes / clipmi_jpeg_progressive_workspace_bytes. status_dev: as the decode entries; a file with a
 * non-zero status leaves unspecified bytes in its block of out_dev and in its scratch rows, and nothing outside them. */
int clipmi_jpeg_decode_transform_rgb8(void* streams_dev, void* images_dev, int n, const void* tables_dev, int ntables,
                                      int64_t total_blocks, int64_t max_blocks, const void* jobs_dev, int max_rows,
                                      const int32_t* coef_dev, int n_px, void* out_dev, void* scratch_dev, int32_t* status_dev,
                                      void* ws_dev, int64_t ws_bytes, void* stream);
int clipmi_jpeg_decode_progressive_transform_rgb8(const void* streams_dev, const void* images_dev, int n, const void* scans_dev,
                                                  int nscans, const void* tables_dev, int ntables, int64_t total_blocks,
                                                  int64_t max_blocks, const void* jobs_dev, int max_rows, const int32_t* coef_dev,
                                                  int n_px, void* out_dev, void* scratch_dev, int32_t* status_dev, void* ws_dev,
                                                  int64_t ws_bytes, void* stream);

/* ---- PNG files on the device (an addition to ABI 8: two new entry points and one new record, nothing existing changes, so
 * CLIPMI_ABI_VERSION stays 8). The same bytes as Pillow's `Image.open(f).convert("RGB")` for the files the host parser lets
 * through (cli-p_amd/png_parse.py: 8-bit grey or RGB, not interlaced, at most 16384 pixels wide, no tRNS, no APNG chunk, and no
 * chunk in front of or behind the image data that makes Pillow refuse the file - the device sees the image data only). Per image one record. stream_off:
 * the IDAT payloads joined, WITHOUT the 2-byte zlib header, the Adler-32 and whatever follows it left in place, 16-byte aligned
 * and followed by at least 16 zero bytes. raw_off: where the image's filtered scanlines (height x (1 + width x channels) bytes)
 * go in the workspace's scanline buffer, a multiple of 16; total_raw_bytes = the sum of the images' scanline sizes, each rounded
 * up to 16, max_raw_bytes = the largest single one. out_dev: per image height rows of width*3 RGB bytes at out_off (grey
 * replicated) - the layout clipmi_resize_crop_rgb8 takes.
 * status_dev[i]: 0 decoded - the DEFLATE data is valid, ends with its final block's end-of-block code having produced exactly
 * the scanlines' bytes, every filter byte is <= 4, and the 4 bytes behind the byte-aligned end of the stream equal the Adler-32
 * of the produced bytes; 1 invalid DEFLATE data (a bad block type, stored length, code set, code or distance) or a record
 * outside the limits above; 2 the stream ended early, produced too little or wants to produce more, or fewer than 4 bytes follow
 * it; 3 a filter byte above 4; 4 the Adler-32 differs. A file with a non-zero status goes back to Pillow, whose error handling
 * is the reference's; its bytes in out_dev are undefined. */
typedef struct clipmi_png_image {
    int64_t stream_off;           /* bytes from streams_dev */
    int64_t raw_off;              /* bytes into the workspace's scanline buffer */
    int64_t out_off;              /* bytes from out_dev */
    int32_t stream_bytes;
    int32_t width, height;
    int32_t channels;             /* 1 (grey) or 3 (RGB) */
    int32_t reserved[2];
} clipmi_png_image;
int64_t clipmi_png_workspace_bytes(int n, int64_t total_raw_bytes);
int clipmi_png_decode_rgb8(const void* streams_dev, const void* images_dev, int n, int64_t total_raw_bytes, int64_t max_raw_bytes,
                           void* out_dev, int32_t* status_dev, void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- Alpha, palette and low-depth PNG files on the device (a further addition to ABI 8 in the sense of the note above: new
 * entry points and one new record, nothing existing changes). clipmi_png_decode_px8 takes the stream layout, the records, the
 * workspace and the arguments of clipmi_png_decode_rgb8 and leaves the file's own-mode pixels, which Pillow's transform
 * resamples before it converts to RGB. A record carries in reserved[0] colour type << 8 | bit depth, in reserved[1] the palette's
 * entry count (colour type 3: 1 .. 1 << depth; otherwise ignored), and in `channels` the samples per pixel (4, 2, 1, 1).
 * Taken: colour type 6 and 4 at depth 8, colour type 3 at depth 1/2/4/8, colour type 0 at depth 1/2/4; a scanline holds
 * ceil(width x channels x depth / 8) bytes behind its filter byte, at most 49152 (the sizes and offsets count these scanlines).
 * out_dev, per image at out_off (a multiple of 16), one of two layouts:
 *   "alpha" (colour types 6 and 4, colour type 0 at depth 2/4): rows of width*4 bytes R G B A; grey + alpha as L L L A, grey at
 *           depth 2 / 4 as v*85 / v*17 three times, then 255 - the layout clipmi_resize_crop_rgba8 takes;
 *   "index" (colour type 3, colour type 0 at depth 1): rows of width bytes, one sample each, the most significant bits of a byte
 *           first, the padding bits at a row's end dropped - the layout clipmi_nearest_crop_p8 takes.
 * status_dev[i]: 0..4 as clipmi_png_decode_rgb8; 5 an "index" image holds a sample >= its entry count (1-bit grey has 2). */
int64_t clipmi_png_px8_workspace_bytes(int n, int64_t total_raw_bytes);
int clipmi_png_decode_px8(const void* streams_dev, const void* images_dev, int n, int64_t total_raw_bytes, int64_t max_raw_bytes,
                          void* out_dev, int32_t* status_dev, void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- Adam7-interlaced PNG files (a further addition to ABI 8 in the sense of the two notes above: no new entry point and no
 * new struct; a caller that leaves `reserved` as it was gets what it got before). Both decode entries take a record of a file
 * written with interlace method 1, for the colour types and depths they take anyway:
 *   clipmi_png_decode_px8:  bit 16 of reserved[0] set (colour type and depth stay in bits 0-15; bits above 16 must be zero);
 *   clipmi_png_decode_rgb8: reserved[0] exactly 1 << 16. Every other value is not looked at, as before.
 * The stream, the filters and the Adler-32 are the same. The scanlines of such a record are those of its up to seven passes
 * one after the other: pass p = 1 .. 7 holds the pixels (x0 + i dx, y0 + j dy) with (x0, y0, dx, dy) = (0,0,8,8) (4,0,8,8)
 * (0,4,4,8) (2,0,4,4) (0,2,2,4) (1,0,2,2) (0,1,1,2), that is pw = ceil((width - x0) / dx) by ph = ceil((height - y0) / dy)
 * pixels, and contributes ph x (1 + ceil(pw x channels x depth / 8)) bytes, or nothing at all where pw or ph is 0. The sizes
 * and offsets (raw_off, total_raw_bytes, max_raw_bytes) count that sum. The output layouts ("rgb", "alpha", "index"), out_off and
 * the status codes 0-5 keep their meaning: the decoded pixels are laid out as those of the same picture stored without
 * interlace, every byte of the image's block of out_dev written once and none outside it. */

/* ---- PNG files of depth 16 (a further addition to ABI 8 in the sense of the notes above: no new entry point and no new struct;
 * every record that was valid before decodes to the same bytes and statuses). clipmi_png_decode_px8 also takes, in
 * reserved[0] = colour type << 8 | bit depth (bit 16: Adam7, as above), three values of depth 16, with `channels` 3, 4, 2:
 *   colour type 2 (RGB):          "rgb" layout - rows of width*3 bytes R G B, what clipmi_png_decode_rgb8 leaves and
 *                                 clipmi_resize_crop_rgb8 takes; the image's block of out_dev holds width x height x 3 bytes;
 *   colour type 6 (RGBA):         "alpha" layout, R G B A;
 *   colour type 4 (grey + alpha): "alpha" layout, L L L A.
 * Each output byte is the high (first) byte of its 16-bit sample, which is what Pillow keeps of such a file; the low bytes are
 * reconstructed with the rest (the filters run byte by byte at the distance of one pixel: 6, 8, 4 bytes) and dropped by the
 * store. A scanline holds width x channels x 2 bytes behind its filter byte, at most 49152: 8192, 6144 and 12288 pixels. The
 * sizes and offsets (raw_off, total_raw_bytes, max_raw_bytes) count these scanlines; status 0-4 as before, never 5.
 * Colour type 0 at depth 16 is not taken (status 1): Pillow resamples it in 16 bits. clipmi_png_decode_rgb8 is unchanged. */

/* The transform for those pixels, bit for bit what Pillow's resize (in the file's mode) + crop + convert("RGB") gives.
 * clipmi_resize_crop_rgba8: arguments and jobs of clipmi_resize_crop_rgb8 with 4 bytes per source and scratch pixel (rows of
 * w*4 bytes; nrows*n_px*4 scratch bytes per job, tmp_off a multiple of 4). A job that resamples an axis premultiplies each
 * pixel as it is loaded (t = c*a + 128; c' = ((t >> 8) + t) >> 8), resamples four channels and un-premultiplies in front of the
 * store (a 0 or 255: c'; else min(255, 255*c' / a)); a job that resamples neither axis crops and drops alpha.
 * clipmi_nearest_crop_p8: "index" rows -> palette colours of the source pixel each output takes. tabs_dev (4-byte aligned)
 * holds, per job, the palette (256 x 3 bytes, pal_off in bytes) and two int32 tables (col_off, row_off: int32 offsets) with the
 * source column of each of the n_px output columns and the source row of each output row, computed by the host with Pillow's
 * float64 accumulation (cli-p_amd/decode_worker.py nearest_window). Both write out_dev as clipmi_resize_crop_rgb8 does. */
typedef struct clipmi_nearest_job {
    int64_t src_off;              /* bytes from raw_dev to the image's first sample (rows of w bytes) */
    int32_t w, h;                 /* source size */
    int32_t out_index;
    int32_t reserved;
    int64_t pal_off;              /* bytes from tabs_dev */
    int64_t col_off, row_off;     /* int32 offsets from tabs_dev */
} clipmi_nearest_job;
int clipmi_resize_crop_rgba8(const void* raw_dev, const void* jobs_dev, int njobs, int max_rows, const int32_t* coef_dev,
                             int n_px, void* out_dev, void* scratch_dev, void* stream);
int clipmi_nearest_crop_p8(const void* raw_dev, const void* jobs_dev, int njobs, const void* tabs_dev, int n_px, void* out_dev,
                           void* stream);
/* clipmi_resize_crop_cmyk8 (with clipmi_jpeg_decode_cmyk8 above): arguments, jobs, 4 bytes per source and scratch pixel and scratch
 * sizing of clipmi_resize_crop_rgba8, for rows of C M Y K bytes. Pillow resamples mode CMYK as four plain bands, so nothing is
 * premultiplied; its convert("RGB") - nk = 255 - K, out_c = clip8(nk - muldiv255(c, nk)) for c in C, M, Y, with muldiv255(a, b):
 * t = a*b + 128, ((t >> 8) + t) >> 8 - is applied in front of the store, also in a job that resamples neither axis. */
int clipmi_resize_crop_cmyk8(const void* raw_dev, const void* jobs_dev, int njobs, int max_rows, const int32_t* coef_dev,
                             int n_px, void* out_dev, void* scratch_dev, void* stream);

/* thread-local message of the last failing call on this thread ("" if none) */
const char* clipmi_last_error(void);
int clipmi_abi_version(void);

/* ---- test/bench hooks: the individual kernels behind encode_*, exported so that parity
 * tests and bench.py can launch and time them one at a time. Not part of the drop-in surface.
 * (clipmi_dbg_embed_image / clipmi_dbg_embed_text are additions to ABI 8 in the sense of the PNG note above: nothing existing
 * changes, CLIPMI_ABI_VERSION stays 8.)
 */
/* C[M][N] = A[M][K](bf16) . W[N][K]^T(bf16) with fused epilogue `epi`:
 *   0: out bf16 = acc + bias        1: out bf16 = quickgelu(acc + bias)
 *   2: out f32 += acc + bias (residual, in place)    3: out f32 = acc (bias may be NULL)
 * `epi` bits 8-10 force a kernel (1 = 128 x 128 tiles, 2 = 256 x 256, 3 = the persistent 256 x 256 kernel). Epilogue 4 (the patch
 * GEMM: row b*np + p goes to row b*L + 1 + p with the positional row 1 + p added) needs a tower's geometry and is refused here; it
 * is tested in its three kernels through clipmi_dbg_embed_image below (tests/test_embed_gpu.py); 5-8 have hooks of their own. */
int clipmi_dbg_gemm_bf16(const void* a_dev, const void* w_dev, const float* bias_dev,
                         void* out_dev, int M, int N, int K, int epi, void* stream);
/* rows of f32 x[M][W] -> LayerNorm(eps 1e-5) -> bf16 (out_bf16 != 0) or f32 */
int clipmi_dbg_layernorm(const float* x_dev, const float* w_dev, const float* b_dev,
                         void* out_dev, int M, int W, int out_bf16, void* stream);
/* qkv bf16 [B*L][3W] -> softmax(q k^T / 8 (+causal)) v -> bf16 [B*L][W], head dim 64 */
int clipmi_dbg_attention(const void* qkv_dev, void* out_dev, int B, int L, int heads,
                         int causal, void* stream);
/* The same attention (no mask) as the FP8 towers launch it, with the fused output stage where the shape's kernel has one
 * (49 <= L <= 52): *fused = 1 and the rows leave as e4m3 [B*L][W] + MX scale bytes [B*L][W / 32] - the bytes
 * clipmi_dbg_quantize_rows_fp8mx makes of clipmi_dbg_attention's rows - and out_bf16_dev is not written; otherwise *fused = 0,
 * bf16 rows in out_bf16_dev and the other two untouched. (An addition to ABI 8 in the sense of the note above: nothing
 * existing changes, CLIPMI_ABI_VERSION stays 8.) */
int clipmi_dbg_attention_fp8mx(const void* qkv_dev, void* out_bf16_dev, void* out_fp8_dev, void* bscale_dev, int B, int L,
                               int heads, int* fused, void* stream);

/* clipmi_topk_ip's launch sequence `reps` times with HIP events around the MAIN scan kernel on
 * `stream`; synchronises; *scan_ms = average duration of that kernel (bench.py roofline). Q <= 16 */
int clipmi_dbg_topk_scan_ms(const void* db_dev, int64_t N, int E, const float* q_dev, int Q, int K,
                            float* out_score_dev, int64_t* out_id_dev, void* ws_dev, size_t ws_bytes,
                            void* stream, int reps, float* scan_ms);

/* The same for clipmi_topk_ip_rows: events around the main list scan (tools/subset_timing.py). Q <= 32, M >= 1. (An addition
 * to ABI 8 in the sense of the note above: nothing existing changes, CLIPMI_ABI_VERSION stays 8.) */
int clipmi_dbg_topk_rows_scan_ms(const void* db_dev, int64_t N, int E, const uint32_t* rows_dev, int64_t M,
                                 const float* q_dev, int Q, int K, float* out_score_dev, int64_t* out_id_dev,
                                 void* ws_dev, size_t ws_bytes, void* stream, int reps, float* scan_ms);

/* Both hooks above in one for a CLIPMI_F16 matrix (tools/f16_timing.py): rows_dev == NULL is the plain scan, otherwise the
 * list form over M >= 1 entries. Q <= 32. (An addition to ABI 8, see CLIPMI_F16.) */
int clipmi_dbg_topk_scan_f16_ms(const void* db_f16_dev, int64_t N, int E, const uint32_t* rows_dev, int64_t M,
                                const float* q_dev, int Q, int K, float* out_score_dev, int64_t* out_id_dev,
                                void* ws_dev, size_t ws_bytes, void* stream, int reps, float* scan_ms);

/* clipmi_topk_ip_coarse `reps` times with HIP events around the bf16 scan kernel (Q <= 64) */
int clipmi_dbg_topk_coarse_scan_ms(const void* db_dev, const void* db_bf16_dev, int64_t N, int E, float rmax,
                                   const float* q_dev, int Q, int K, float* out_score_dev, int64_t* out_id_dev,
                                   void* ws_dev, size_t ws_bytes, void* stream, int reps, float* scan_ms,
                                   long long* survivors /* optional: rows kept by the coarse pass, summed over Q */);

int clipmi_dbg_topk_coarse_i8_scan_ms(const void* db_dev, const void* db_i8_dev, const float* meta_dev, float amax,
                                      int64_t N, int E, float rmax, const float* q_dev, int Q, int K,
                                      float* out_score_dev, int64_t* out_id_dev, void* ws_dev, size_t ws_bytes,
                                      void* stream, int reps, float* scan_ms, long long* survivors);

/* The wide passes of clipmi_topk_ip_wide_i8 (64 < Q; E = 512 or 768; workspace: clipmi_topk_ip_wide_workspace_bytes) `reps`
 * times with HIP events around every wide scan launch; synchronises. Of the last repetition: *scan_ms = the summed duration of
 * the wide scan launches, *survivors = the exactly re-scored (query, row) pairs, *scan_launches = the number of wide scan
 * launches (segments x chunks: the copy is streamed once per chunk), *fallback_armed = 1 if a list overflowed (the exact
 * fallback answered). The last three may be NULL. */
int clipmi_dbg_topk_wide_i8_scan_ms(const void* db_dev, const void* db_i8_dev, const float* meta_dev, float amax,
                                    int64_t N, int E, float rmax, const float* q_dev, int Q, int K,
                                    float* out_score_dev, int64_t* out_id_dev, void* ws_dev, size_t ws_bytes,
                                    void* stream, int reps, float* scan_ms, long long* survivors, int* scan_launches,
                                    int* fallback_armed);

/* the FP8 path's two kernels alone: bf16 [M][K] -> e4m3 [M][K] + f32 row scales; C = a_scale w_scale (A8 W8^T) + epilogue
 * `epi` (0 bias -> bf16, 1 bias + QuickGELU -> bf16, 2 bias + residual into f32 out, 3 f32) */
int clipmi_dbg_quantize_rows_fp8(const void* in_bf16_dev, void* out_fp8_dev, float* scale_dev, int M, int K, void* stream);
int clipmi_dbg_gemm_fp8(const void* a8_dev, const void* w8_dev, const float* a_scale_dev, const float* w_scale_dev,
                        const float* bias_dev, void* out_dev, int M, int N, int K, int epi, void* stream);

/* LN-folded linear layers (tower ABI 3, csrc/gemm.hpp), kernel by kernel:
 * The residual stream is kept SPLIT (3 bytes per element since round 5 / ABI 5): a row of width W is W bf16 values hi = bf16(x)
 * followed by W biased 8-bit remainders u, bits(x') = (bits(hi) << 16) + (u << 8) - 0x8000 - x to 15 mantissa bits; `x3` buffers are [M][3 W] bytes.
 *   split_stats   rows = add ? x + x3 : x (f32 [M][W]) -> x3 = the split rows, part [M][W/256][2]
 *                 = per-256-column (sum, sum of squares)                                           (W % 256 == 0, <= 1024)
 *   gemm_ln       out bf16 = [quick_gelu] (rstd * (hi(x3) wg^T - mean * colsum) + cb), (mean, rstd) from part; epi 5 | 6,
 *                 bits 8-9 force a kernel
 *   gemm_resid_ln x3 += a w^T + bias, part of the new rows; tmp = f32 [M][N] scratch; algo 3 = the persistent
 *                 kernel's fused store pass, else GEMM into tmp + split_stats(add) */
int clipmi_dbg_split_stats(const float* x_dev, int add, void* x3_dev, float* part_dev, int M, int W, void* stream);
int clipmi_dbg_gemm_ln(const void* x3_dev, const void* wg_dev, const float* cb_dev, const float* colsum_dev,
                       const float* part_dev, void* out_dev, int M, int N, int K, int epi, void* stream);
/* MX block scales (round 3): e4m3 activations with one e8m0 scale per 32 consecutive values of a row, 2^(e - 7) with
 * e = floor(log2(largest magnitude of the block)). clipmi_dbg_quantize_rows_fp8mx: bf16 [M][K] -> e4m3 [M][K] + scale
 * bytes [M][K / 32] (K a multiple of 32). clipmi_dbg_gemm_fp8_bsa: out = w_scale[n] * sum_k (scaled A8)[m][k] W8[n][k]
 * + bias (+ out for epi 2; epi 3 = plain f32) on the block-scaled matrix-core instruction; a_bscale_dev holds
 * ceil(M / 256) * 256 rows of K / 32 bytes. */
int clipmi_dbg_quantize_rows_fp8mx(const void* in_bf16_dev, void* out_fp8_dev, void* bscale_dev, int M, int K, void* stream);
int clipmi_dbg_gemm_fp8_bsa(const void* a8_dev, const void* w8_dev, const void* a_bscale_dev, const float* w_scale_dev,
                            const float* bias_dev, void* out_dev, int M, int N, int K, int epi, void* stream);
/* One prompt / one image (M <= 128 rows, csrc/gemm_skinny.hpp, round 5): the residual GEMM updates the split rows in place and writes
 * the statistics LEAVES leaf_dev [M][N / 4][2] ((sum, sum of squares) of every 4-column group) instead of running a split /
 * statistics pass; the LN-folded consumer behind it reads them and runs the canonical reduction tree itself. Bit for bit
 * clipmi_dbg_gemm_resid_ln followed by clipmi_dbg_gemm_ln. */
int clipmi_dbg_gemm_resid_ln_leaf(const void* a_dev, const void* w_dev, const float* bias_dev, void* x3_dev, float* leaf_dev,
                                  int M, int N, int K, void* stream);
int clipmi_dbg_gemm_ln_leaf(const void* x3_dev, const void* wg_dev, const float* cb_dev, const float* colsum_dev,
                            const float* leaf_dev, void* out_dev, int M, int N, int K, int epi, void* stream);
int clipmi_dbg_gemm_resid_ln(const void* a_dev, const void* w_dev, const float* bias_dev, void* x3_dev, float* part_dev,
                             float* tmp_dev, int M, int N, int K, int algo, void* stream);

/* The row kernels in every form the towers launch them (tests/test_rows_exact_gpu.py; additions to ABI 8 in the sense of the
 * note above: nothing existing changes, CLIPMI_ABI_VERSION stays 8).
 * clipmi_dbg_layernorm_forms sets every field of the LayerNorm launcher's arguments one to one. Output row r is made of source
 * row rowidx_dev[r] (int32 [M]) or, without rowidx_dev, r * row_step (1 = dense); the source is f32 rows x_dev [..][W] or split
 * rows x3_dev [..][3 W bytes], exactly one of the two. One output form:
 *   out8_dev + scale8_dev       : e4m3 [M][W] + f32 row scales [M], the bytes clipmi_dbg_quantize_rows_fp8 makes of the bf16 rows
 *                                 (out_dev is not written);
 *   out_x3_dev + out_part_dev   : split rows [M][3 W bytes] + statistics partials [M][W/256][2] (W % 256 == 0), the bytes
 *                                 clipmi_dbg_split_stats makes of the f32 rows (out_dev is not written);
 *   out_dev                     : bf16 (out_bf16 != 0) or f32 [M][W]; out_dev == x_dev (f32, dense) normalises in place.
 * W % 4 == 0, W <= 1024.
 * clipmi_dbg_gather_rows: dst[b][:] = src[b * L][:], b < B, rows of row_bytes bytes (a multiple of 16): the class-token rows of the
 * pruned last block.
 * clipmi_dbg_gemm_fp8_mxout: clipmi_dbg_gemm_fp8 in its default form with one more output: with out_bscale_dev set, a QuickGELU
 * GEMM (epi 1) that runs on the persistent kernel writes its rows as e4m3, N bytes apart, into out_dev and their MX scale bytes
 * [M][N / 32] into out_bscale_dev - the bytes clipmi_dbg_quantize_rows_fp8mx makes of the bf16 rows; any other epilogue or a shape
 * off the persistent kernel is refused (clipmi_dbg_gemm_fp8_plan with out_bscale = 1 says which). out_bscale_dev == NULL: bf16 /
 * f32 rows as clipmi_dbg_gemm_fp8 writes them. */
int clipmi_dbg_layernorm_forms(const float* x_dev, const void* x3_dev, const int32_t* rowidx_dev, int64_t row_step,
                               const float* w_dev, const float* b_dev, void* out_dev, int out_bf16, void* out8_dev,
                               float* scale8_dev, void* out_x3_dev, float* out_part_dev, int M, int W, void* stream);
int clipmi_dbg_gather_rows(const void* src_dev, void* dst_dev, int B, int L, size_t row_bytes, void* stream);
int clipmi_dbg_gemm_fp8_mxout(const void* a8_dev, const void* w8_dev, const float* a_scale_dev, const float* w_scale_dev,
                              const float* bias_dev, void* out_dev, void* out_bscale_dev, int M, int N, int K, int epi,
                              void* stream);

/* Which kernel a GEMM of this shape runs on (csrc/gemm_plan.hpp: the rule the launchers follow), host only - no device is
 * touched, no operand exists. clipmi_dbg_gemm_plan: the bf16 GEMMs; epi = the EPI_* number, algo 0 = by shape, 1 / 2 / 3 force
 * the 128 x 128 / 256 x 256 / persistent 256 x 256 kernel, ln_leaf / ln_leaf_in != 0: the caller passes statistics leaves
 * (M <= 128), dbg: 0. clipmi_dbg_gemm_fp8_plan: the FP8 GEMMs; mx as bits 8-9 of clipmi_dbg_gemm_fp8 select it (1 the product's
 * choice, 0 plain FP8, 2 MX off the persistent kernel), a_bscale / out_bscale != 0: block-scaled A / e4m3 + block-scale output.
 * out[0] = the number of launches (> 1: the rows that fill whole rounds of 256 x 256 tiles run first, on the persistent
 * kernel), then per launch 7 values: rows, kernel (0 128 x 128, 1 256 x 256, 2 persistent, 3 skinny, 4 gemm256f8, 5 gemm256f8
 * with block-scaled A), the kernel's epilogue, 1 if it is an f32 launch into the scratch rows with split_stats behind it,
 * 1 if the skinny residual producer writes statistics leaves, and the persistent kernel's grid and LDS bytes. out[22], refused
 * or not: what the encode path's own query of the plan answers for (M, N, K) - clipmi_dbg_gemm_plan: the residual GEMM runs on
 * the skinny kernel and can write leaves; clipmi_dbg_gemm_fp8_plan: the QuickGELU GEMM can write e4m3 + block scales. n_out:
 * the length of out (23 holds everything). A shape the launcher refuses returns its error code and message. */
int clipmi_dbg_gemm_plan(int M, int N, int K, int epi, int algo, int ln_leaf, int ln_leaf_in, int dbg, int32_t* out, int n_out);
int clipmi_dbg_gemm_fp8_plan(int M, int N, int K, int epi, int mx, int a_bscale, int out_bscale, int32_t* out, int n_out);

/* The embedding front ends of the two towers - everything in front of the first block - as clipmi_encode_image /
 * clipmi_encode_text enqueue them (the same function runs in both), in the tower's ordinary workspace
 * (clipmi_encode_*_workspace_bytes), followed by copies of the results on the same stream. Every `*_out_dev` pointer may be NULL.
 * clipmi_dbg_embed_image: patchify (pix_dtype as clipmi_encode_image) -> patch GEMM with the positional rows (`algo`: 0 = the
 * product's choice by shape, 1 / 2 = force the 128 x 128 / 256 x 256 kernel; 2 needs width % 256 == 0) -> class-token rows ->
 * ln_pre when with_ln_pre != 0.
 *   patches_out_dev : bf16 [B*np][patch_k], the patch matrix (np = tokens - 1)
 *   rows_out_dev    : f32 [B*L][W] - with_ln_pre == 0: the rows in front of ln_pre; with_ln_pre != 0: the rows behind it, for
 *                     towers that keep f32 rows there (ln_fold 0, FP8 weights)
 *   x3_out_dev, part_out_dev : with_ln_pre != 0 and a bf16 LN-folded tower: the split rows [B*L][3 W bytes] and their statistics
 *                     partials f32 [B*L][W/256][2] (clipmi_dbg_split_stats' layout)
 * An output the tower does not produce in that form (rows_out_dev for split rows and the reverse) is CLIPMI_EINVAL.
 * clipmi_dbg_embed_text: token + positional embedding and the EOT rows; rows_out_dev f32 [Q*L][W] (towers without folded
 * LayerNorms) or x3_out_dev + part_out_dev (LN-folded towers), rowidx_out_dev int32 [Q] = q*L + first argmax of ids[q][:]. */
int clipmi_dbg_embed_image(const clipmi_tower* t, const void* blob_dev, const void* pixels_dev, int pix_dtype, int B,
                           int algo, int with_ln_pre, void* patches_out_dev, float* rows_out_dev, void* x3_out_dev,
                           float* part_out_dev, void* ws_dev, size_t ws_bytes, void* stream);
int clipmi_dbg_embed_text(const clipmi_tower* t, const void* blob_dev, const int32_t* ids_dev, int Q, float* rows_out_dev,
                          void* x3_out_dev, float* part_out_dev, int32_t* rowidx_out_dev, void* ws_dev, size_t ws_bytes,
                          void* stream);

/* clipmi_encode_image `reps` times with HIP events around every launch of the GEMM whose
 * epilogue is `probe_epi` (1 = MLP c_fc + QuickGELU), on `stream`; synchronises;
 * *kernel_ms = average duration of the timed launches (bench.py roofline) */
int clipmi_dbg_encode_image_probe_ms(const clipmi_tower* t, const void* blob_dev, const void* pixels_dev,
                                     int pix_dtype, int B, float* out_dev, void* ws_dev, size_t ws_bytes,
                                     void* stream, int probe_epi, int reps, float* kernel_ms, int* launches);

/* The same with three estimators of the kernel's in-situ duration, ms3[0..2] (csrc/encode.hip encode_probe): begin -> end
 * events of the launch itself (reads long in a back-to-back stream), plain event in front -> end event, and end event of the
 * GEMM directly in front -> end event of this one (completion to completion; 0 when not applicable). *kernel_kind: 0 / 1 / 2 =
 * gemm_bf16_nt_kernel / gemm256_bf16_nt_kernel / gemm256p_bf16_nt_kernel; *epi_ran: its EPI template argument.
 * probe_epi bits 8 and up, when non-zero, restrict the probe to launches with that K (attn.out_proj and mlp.c_proj share the
 * residual epilogue: 2 | (3072 << 8) times c_proj alone). */
int clipmi_dbg_encode_image_probe3_ms(const clipmi_tower* t, const void* blob_dev, const void* pixels_dev,
                                      int pix_dtype, int B, float* out_dev, void* ws_dev, size_t ws_bytes,
                                      void* stream, int probe_epi, int reps, float* ms3, int* launches,
                                      int* kernel_kind, int* epi_ran);

#ifdef __cplusplus
}
#endif
#endif /* CLIPMI_H */
