// jpeg.hip — `Image.open(tfn)` on the device for baseline JPEG files (the decode in front of
// `transform(...)`, reference build-index.py:47-48). Pillow decodes with libjpeg-turbo (third-party, absent from the
// reference tree); its published algorithm is restated here for the subset the host parser (cli-p_amd/jpeg.py) lets
// through - 8-bit baseline / extended-sequential Huffman, one interleaved scan, grey or YCbCr with luma sampling 1x1 /
// 2x1 / 2x2 and 1x1 chroma, with or without restart intervals - and produces Pillow's bytes (tests/test_jpeg_gpu.py compares with
// Pillow itself; oracle/jpeg_oracle.py is the CPU restatement, pinned against Pillow in tests/test_jpeg.py).
// Where the host opts in (jpeg_parse.parse(layouts=True)) the records also name luma sampling 1x2 (4:4:0: jdsample.c's
// h1v2_fancy_upsample), 4x1 (4:1:1) and 1x4 (int_upsample: replication), and a colour transform of "none" for the files libjpeg
// takes for RGB-coded: further values of JpegGeom's `mode` and its `rgb` flag (tests/test_jpeg_layouts_gpu.py).
// Four-component files (jpeg_parse.parse(cmyk=True): CMYK as stored and YCCK, components 1-3 sampled 1x1) go through the same
// chain over their own record, clipmi_jpeg_image4, to Pillow's mode-CMYK bytes (clipmi_jpeg_decode_cmyk8, jpeg_cmyk_kernel;
// tests/test_jpeg_cmyk_gpu.py); resize.hip's clipmi_resize_crop_cmyk8 resamples those and converts them to RGB as Pillow does.
// Everything else (12-bit, arithmetic coding, ...) stays with Pillow in the decode workers; PNG files have png.hip.
//
// Kernels, one batch of images per call (every kernel takes an image's block and plane layout from jpeg_geom):
//   jpeg_unstuff_kernel      the baseline record's first reader and its checker (jp_record_ok): a record whose sampling factors,
//                            colour transform or size the kernels do not take is emptied in place, for jpeg_huffman_kernel to
//                            report (status 1) and every later kernel to pass over. Then, for segments the host hands over as
//                            they are in the file, the 0x00 behind every 0xFF removed in place
//   jpeg_build_luts_kernel   canonical Huffman codes of the batch's distinct DHT tables -> 10-bit look-up + slow-path arrays
//                            (jpeg_build_pluts_kernel: the progressive form of the entries; one builder, jp_build_lut)
//   jpeg_huffman_kernel      the entropy-coded segment -> int16 coefficients (DC still differential). Huffman decoding is a
//                            serial chain (a symbol's first bit is known only when the previous symbol has been decoded);
//                            a workgroup owns an image and decodes it in 1024-bit SUBSEQUENCES, one per thread: every thread
//                            starts at its subsequence's first bit as if a block began there, then repeatedly restarts from
//                            its predecessor's exit state (bit position, block within the MCU, coefficient index) until no
//                            exit state changes. Thread 0's start is exact, so by induction the fixed point is the
//                            sequential decode; Huffman streams re-synchronise by themselves after a few symbols, so on
//                            photographs the loop ends after 2-3 rounds (Klein & Wiseman's observation, used for JPEG by
//                            Weissenberger & Schmidt); on noise images without end-of-block symbols it degenerates to the
//                            serial chain, one subsequence per round, and still ends. A scan of the blocks completed per
//                            subsequence gives every thread its first block; a last pass writes the coefficients.
//                            Files with restart intervals need none of that: every interval starts on a byte the host found,
//                            at a known block, with fresh DC predictions - one thread walks one interval.
//   jpeg_dc_kernel           DC prediction: per-component running sums over the blocks in scan order
//   jpeg_idct_kernel         jidctint.c's jpeg_idct_islow with the dequantisation folded in, one block per thread; a block
//                            outside the range where libjpeg-turbo's IDCT provably equals it is reported (status 4)
//   jpeg_color_kernel        jdsample.c's fancy (triangle) upsampling with jdmainct.c's edge rows + jdcolor.c's
//                            16-bit fixed-point YCbCr -> RGB (jp_pixel); rows of width*3 bytes, as Pillow's array
//   jpeg_color_resize_h_kernel   the transform entries' form of the last step: the same upsampling and colour conversion fused with
//                            Pillow's horizontal resampling pass (resize.hip's resize_h_kernel), over the rows and columns the
//                            transform's window needs only - the full-size RGB rows are never written
//   jpeg_cmyk_kernel         the last step for a four-component record: the same upsampling per plane, then Pillow's CMYK bytes,
//                            rows of width*4 (the kernels in front of it are instantiated over the wider record, JpegImage4)
//   jpeg_progressive_kernel  progressive files: every scan of an image applied to its coefficients, in place of
//                            jpeg_huffman_kernel and jpeg_dc_kernel; jpeg_idct_kernel and the colour kernels follow as above
#include <type_traits>

#include "common.hpp"

namespace clipmi {
namespace {

// The baseline record at the two component counts it comes in: clipmi_jpeg_image (1 or 3 components; JpegImage) and
// clipmi_jpeg_image4 (4: CMYK / YCCK files; JpegImage4). The decode chain up to the sample planes is written once over the record
// type (kernel templates over Im below), instantiated per record, so that the three-component kernels are compiled from the code
// they always had, with the count a constant.
template <int NC_>
struct JpegImageT {            // mirrors clipmi_jpeg_image / clipmi_jpeg_image4 (include/clipmi.h)
    static constexpr int NC = NC_;
    long long stream_off, coef_off, out_off, intervals_off;
    int stream_bytes;
    int width, height;
    int ncomp;
    int hs, vs;
    int dc_tbl[NC_], ac_tbl[NC_];
    int restart_interval, n_intervals;
    int stuffed, transform;    // transform: the records' `reserved` - 0 YCbCr -> RGB, 1 none (the components are R, G, B); four
                               // components: 2 CMYK as stored, 3 YCCK
    unsigned char quant[NC_][64];
};
using JpegImage = JpegImageT<3>;
using JpegImage4 = JpegImageT<4>;

// The luma sampling factors the kernels take (chroma is 1 x 1): 1x1, 2x1, 2x2, and 1x2, 4x1, 1x4
__device__ __forceinline__ bool jp_sampling_ok(int hs, int vs) {
    return (hs == 1 && (vs == 1 || vs == 2 || vs == 4)) || (hs == 2 && (vs == 1 || vs == 2)) || (hs == 4 && vs == 1);
}

// What every kernel behind the record's first reader relies on. A record outside it is reported (status 1), never decoded: its
// first reader (jpeg_unstuff_kernel; jpeg_progressive_kernel for its own records) leaves an empty grey image in its place.
__device__ __forceinline__ bool jp_record_ok(int ncomp, int width, int height, int hs, int vs, int transform) {
    return width >= 1 && height >= 1 && (ncomp == 1 ? transform == 0 : ncomp == 3 && jp_sampling_ok(hs, vs) && (transform == 0 || transform == 1));
}
// The same for a clipmi_jpeg_image4: four components, component 0 at one of the samplings above, CMYK as stored or YCCK
__device__ __forceinline__ bool jp_record4_ok(int ncomp, int width, int height, int hs, int vs, int transform) {
    return width >= 1 && height >= 1 && ncomp == 4 && jp_sampling_ok(hs, vs) && (transform == 2 || transform == 3);
}

// Chroma upsampling (JpegGeom.mode). 0, 1, 2 are luma 1x1, 2x1, 2x2 - every file before the layouts switch -, and the pixel
// functions test for these three first and run the code they always ran; the other two go through the `_more` functions. (With
// all five in one chain, the mode a chain of branches and the colour transform loaded in front of it, jpeg_color_kernel - a pixel
// per thread - took 8.9 instead of 8.2 ms over 435 photos of 2 000 x 1 500 and the fused kernel 7.6 instead of 7.0.)
enum { JM_COPY = 0, JM_H2V1 = 1, JM_H2V2 = 2, JM_H1V2 = 3, JM_REPL = 4 };

// An image's blocks and planes. Coefficients (int16 [64] per block, from coef_all + coef_off * 64) come in scan order: MCU
// after MCU, each the hv luma blocks, then Cb, Cr. Planes of an image (bytes from planes + coef_off * 64):
// Y [my vs 8][mx hs 8], then Cb, Cr [my 8][mx 8]. A four-component record (JpegImage4) has the same layout with a third
// one-by-one component behind the two: hv + 3 blocks per MCU, a fourth plane [my 8][mx 8].
struct JpegGeom {
    int W, H;
    int hs, vs;                    // luma sampling factors (grey: 1, whatever the file says); chroma is 1 x 1
    int hv, bpm;                   // luma blocks, all blocks per MCU
    int mx, my;                    // MCUs per row, per column
    long long nmcu;                // mx my
    int yw, cw;                    // bytes per row of the luma plane, of a chroma plane
    int dw, dh;                    // chroma columns, rows under the image: ceil(W / hs), ceil(H / vs) (fancy upsampling's edges)
    int mode;                      // chroma upsampling: JM_COPY 1x1, JM_H2V1, JM_H2V2, JM_H1V2 (fancy), JM_REPL 4x1 / 1x4 (replication)
    int sx, sy;                    // log2 hs, log2 vs: the chroma sample of pixel (x, y) without filtering is (x >> sx, y >> sy)
    bool color;
    bool rgb;                      // no colour conversion: the three planes are R, G, B
    const unsigned char* py;       // the planes: luma, Cb and Cr (only from jpeg_geom with the planes' base)
    const unsigned char* pc[2];
    // bytes from the luma plane to the plane of component c = 1 (Cb), 2 (Cr) - and 3, the fourth component of a four-component
    // record, whose planes follow each other the same way (its pixel kernel takes that plane from here; pc holds the first two)
    __device__ __forceinline__ long long plane_off(int c) const { return (long long)mx * my * hv * 64 + (long long)(c - 1) * mx * my * 64; }
};

// (The record by pointer, and the sampling factors read behind the test for grey, as the kernels did before they shared this: a
// reference parameter lets the compiler load every field up front, which cost jpeg_huffman_kernel a VGPR and two spilled SGPRs.)
// Im: JpegImage or JpegImage4 - a record that is not grey has Im::NC components, hv blocks of the first and one of each other
// per MCU (a four-component record's `rgb` flag means nothing: its pixel kernel reads the transform itself).
template <class Im>
__device__ __forceinline__ JpegGeom jpeg_geom(const Im* im, const unsigned char* planes = nullptr) {
    JpegGeom g;
    const int tf = im->transform;
    g.color = im->ncomp != 1;
    g.hs = im->ncomp == 1 ? 1 : im->hs;
    g.vs = im->ncomp == 1 ? 1 : im->vs;
    g.hv = g.hs * g.vs;
    g.bpm = im->ncomp == 1 ? 1 : g.hv + (Im::NC - 1);
    g.W = im->width;
    g.H = im->height;
    g.mx = (g.W + 8 * g.hs - 1) / (8 * g.hs);
    g.my = (g.H + 8 * g.vs - 1) / (8 * g.vs);
    g.nmcu = (long long)g.mx * g.my;
    g.yw = g.mx * g.hs * 8;
    g.cw = g.mx * 8;
    g.sx = g.hs >> 1;              // (1, 2, 4 -> 0, 1, 2)
    g.sy = g.vs >> 1;
    g.dw = (g.W + g.hs - 1) >> g.sx;
    g.dh = (g.H + g.vs - 1) >> g.sy;
    // (selects, not branches; and the transform - 0 or 1 in a record that passed jp_record_ok, 0 in a grey one - is read with no
    // test in front of it and used only behind the samples' loads, see jp_pixel)
    static_assert(JM_H2V1 == 1 && JM_H2V2 == 2, "hs == 2: the mode is vs");
    g.mode = g.hs == 2 ? g.vs : (g.vs == 2 ? JM_H1V2 : (g.hv == 4 ? JM_REPL : JM_COPY));
    g.rgb = tf != 0;
    g.py = planes + im->coef_off * 64;
    g.pc[0] = g.py + g.plane_off(1);
    g.pc[1] = g.py + g.plane_off(2);
    return g;
}

constexpr int JP_T = 128;          // threads per workgroup = subsequences per chunk: ONE wave (waves that walk serial chains
                                   // must not share a SIMD: 870 two-wave workgroups ran 3.2 x slower than one)
constexpr int JP_SUB_BITS = 1024;  // bits per subsequence (32 words)
constexpr int JP_FAST = 10;        // bits of the direct look-up
constexpr int JP_SPEC = 3;         // speculative rounds before the rounds turn serial (jpeg_huffman_kernel)
constexpr int JP_RAW = 288;        // bytes of a raw table: 16 counts + 256 symbols + class (0 DC, 1 AC) + 15 zero bytes

// A 16-bit table entry says everything the state machine needs about a symbol: the bits to skip (code + the value bits behind it,
// 1..31), the step of the coefficient index (DC: 0 -> 1; AC: run + 1, 16 for ZRL, 64 = end of block) and the number of value bits.
// (LDS per workgroup decides how many images are resident at once, and an image can be a serial chain of milliseconds.)
__device__ __forceinline__ unsigned jp_entry(unsigned sym, unsigned len, bool ac) {
    const unsigned s = sym & 15, r = sym >> 4;
    const unsigned dz = !ac ? 1u : (s ? r + 1 : (r == 15 ? 16u : 64u));
    return (len + s) | (dz << 5) | (s << 12);
}
#define JP_ADV(e) ((e) & 31u)
#define JP_DZ(e) (((e) >> 5) & 127u)
#define JP_S(e) ((e) >> 12)

constexpr int JP_LONG = 8;         // canonical codes grow upwards, so the codes longer than JP_FAST bits sit under the LAST few
                                   // JP_FAST-bit prefixes (the standard tables: 5); the last JP_LONG prefixes get a 16-bit table
struct JpLut {
    unsigned short fast[1 << JP_FAST];   // jp_entry of codes of up to JP_FAST bits, 0 = longer (or invalid)
    unsigned short second[JP_LONG << (16 - JP_FAST)];   // by bits JP_FAST..15 for the last JP_LONG prefixes, 0 = invalid
    int maxcode[18];                     // largest code of length l (-1: none)
    int valoff[18];                      // symbol index of a code of length l = code + valoff[l]
    unsigned char vals[256];
    int covered;                         // every longer code sits in `second` (else: the bit-by-bit walk)
    int pad_[3];
};
static_assert(sizeof(JpLut) % 16 == 0, "tables are copied as 16-byte pieces");

__device__ const unsigned char jp_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Byte stuffing (a 0x00 behind every 0xFF of entropy-coded data) removed on the device, in place: the host then only slices the
// file (removing it there is 1.5 ms per MB of Python in a decode worker - the bound for photo-sized files). A workgroup per image
// walks the segment in 8-KB tiles: 32 bytes per thread in registers, kept bytes counted, an exclusive scan over the workgroup, the
// bytes written back at their compacted positions (never in front of a byte still to be read: the tile is in registers, and the
// output only falls behind the input). Any 0xFF followed by something else than 0x00 is a marker inside the scan: the record is
// tagged (stuffed = 2) and jpeg_huffman_kernel reports the file (status 3: Pillow decides).
template <class Im>
__global__ void __launch_bounds__(256) jpeg_unstuff_kernel(unsigned char* __restrict__ streams, Im* __restrict__ images) {
    Im& im = images[blockIdx.x];
    // the record's first reader: one the kernels do not take (a sampling, a colour transform, a size) becomes an empty grey image
    // without data, which gives no later kernel anything to do and which jpeg_huffman_kernel reports (status 1: no pixels). Thread 0
    // decides and rewrites; the others read the record behind the barrier.
    __shared__ int s_ok;
    if (threadIdx.x == 0) {
        s_ok = Im::NC == 4 ? jp_record4_ok(im.ncomp, im.width, im.height, im.hs, im.vs, im.transform)
                           : jp_record_ok(im.ncomp, im.width, im.height, im.hs, im.vs, im.transform);
        if (!s_ok) {
            im.width = im.height = 0;
            im.ncomp = im.hs = im.vs = 1;
            im.transform = im.stuffed = 0;
            im.stream_bytes = im.restart_interval = im.n_intervals = 0;
        }
    }
    __syncthreads();
    if (!s_ok || im.stuffed != 1) return;
    __shared__ int wsum[4];
    __shared__ unsigned char lastb[256];
    __shared__ int s_marker;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char* s = streams + im.stream_off;
    const int nraw = im.stream_bytes;
    if (tid == 0) s_marker = 0;
    int outpos = 0;
    unsigned char tile_prev = 0;
    for (int t0 = 0; t0 < nraw; t0 += 8192) {
        const int b0 = t0 + tid * 32;
        uint4 v[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
        if (b0 < nraw) v[0] = *reinterpret_cast<const uint4*>(s + b0);                 // (the segment is 16-byte aligned and padded)
        if (b0 + 16 < nraw) v[1] = *reinterpret_cast<const uint4*>(s + b0 + 16);
        const unsigned char* b = reinterpret_cast<const unsigned char*>(v);
        lastb[tid] = b[31];
        __syncthreads();
        unsigned char prev = tid ? lastb[tid - 1] : tile_prev;
        const unsigned char next_prev = lastb[255];
        int nk = 0, mk = 0;
        unsigned dropmask = 0;                              // bit k: byte k is a stuffed 0x00 (or lies behind the segment)
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const unsigned char cur = b[k];
            const bool in = b0 + k < nraw;
            const bool drop = !in || (prev == 0xFF && cur == 0);
            if (in && prev == 0xFF && cur != 0) mk = 1;
            if (in && b0 + k == nraw - 1 && cur == 0xFF) mk = 1;         // a 0xFF with nothing behind it
            dropmask |= (drop ? 1u : 0u) << k;
            nk += drop ? 0 : 1;
            prev = cur;
        }
        // exclusive scan of nk over the workgroup: within the wave by shuffles, across the four waves through LDS
        int inc = nk;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int base = outpos;
        for (int w = 0; w < wave; ++w) base += wsum[w];
        const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        unsigned char* o = s + base + inc - nk;
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (!((dropmask >> k) & 1)) *o++ = b[k];
        if (mk) s_marker = 1;
        outpos += total;
        tile_prev = next_prev;
        __syncthreads();                                    // wsum / lastb are rewritten by the next tile
    }
    if (tid < 16) s[outpos + tid] = 0;                      // a zero tail for the last word (>= 16 bytes of padding follow the segment)
    __syncthreads();
    if (tid == 0) {
        im.stream_bytes = outpos;
        im.stuffed = s_marker ? 2 : 0;
    }
}

// The canonical codes of one raw DHT table (jdhuff.c jpeg_make_d_derived_tbl) into a look-up table, by one workgroup of 256:
// thread 0 walks the code lengths, then a thread per symbol fills the entries its code is a prefix of. The table types share
// `fast`, maxcode, valoff and vals; per type: the entry's encoding (jp_lut_entry) and JpLut's second level with its `covered`.
__device__ __forceinline__ unsigned short jp_lut_entry(const JpLut&, unsigned sym, unsigned len, bool ac) {
    return (unsigned short)jp_entry(sym, len, ac);
}

template <class Lut>
__device__ __forceinline__ void jp_build_lut(const unsigned char* __restrict__ t, Lut& L) {
    constexpr bool LONG = std::is_same<Lut, JpLut>::value;
    __shared__ int first_code[18], first_idx[18];
    const int tid = threadIdx.x;
    for (int i = tid; i < (1 << JP_FAST); i += 256) L.fast[i] = 0;
    if constexpr (LONG)
        for (int i = tid; i < (JP_LONG << (16 - JP_FAST)); i += 256) L.second[i] = 0;
    if (tid == 0) {
        int code = 0, k = 0, covered = 1;
        for (int l = 1; l <= 16; ++l) {
            const int n = t[l - 1];
            first_code[l] = code;
            first_idx[l] = k;
            L.maxcode[l] = n ? code + n - 1 : -1;
            L.valoff[l] = k - code;
            if (n && l > JP_FAST && (code >> (l - JP_FAST)) < (1 << JP_FAST) - JP_LONG) covered = 0;
            code = (code + n) << 1;
            k += n;
        }
        first_idx[17] = k > 256 ? 256 : k;
        L.maxcode[0] = L.maxcode[17] = -1;
        L.valoff[0] = L.valoff[17] = 0;
        if constexpr (LONG) L.covered = covered;
    }
    L.vals[tid] = t[16 + tid];
    __syncthreads();
    if (tid < first_idx[17]) {
        int l = 1;
        while (l < 16 && tid >= first_idx[l + 1]) ++l;
        const int code = first_code[l] + (tid - first_idx[l]);
        const unsigned short e = jp_lut_entry(L, t[16 + tid], (unsigned)l, t[272] != 0);
        if (l <= JP_FAST && code < (1 << l)) {
            const int base = code << (JP_FAST - l);
            for (int j = 0; j < (1 << (JP_FAST - l)); ++j) L.fast[base + j] = e;
        } else if constexpr (LONG) {
            if (l > JP_FAST && code < (1 << l)) {
                const int v16 = code << (16 - l);
                const int pre = (v16 >> (16 - JP_FAST)) - ((1 << JP_FAST) - JP_LONG);
                if (pre >= 0) {
                    const int base = (pre << (16 - JP_FAST)) + (v16 & ((1 << (16 - JP_FAST)) - 1));
                    for (int j = 0; j < (1 << (16 - l)); ++j) L.second[base + j] = e;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(256) jpeg_build_luts_kernel(const unsigned char* __restrict__ raw, JpLut* __restrict__ luts) {
    jp_build_lut(raw + (size_t)blockIdx.x * JP_RAW, luts[blockIdx.x]);
}

struct JpState {
    unsigned p;      // bit position in the image's entropy-coded segment
    unsigned bz;     // (block within the MCU) << 8 | index of the next coefficient (0 = the block's DC symbol comes next)
};

template <int NC>
struct JpSharedT {
    JpLut lut[2 * NC];                         // [component][DC, AC]
    unsigned words[JP_T * 33 + 40];            // the chunk's big-endian words, word i at i + i / 32 (subsequence i at 33 i: bank spread)
    JpState exit_state[JP_T];
    JpState start_state[JP_T];
    int blocks[JP_T];
    unsigned char nat[64];
    int first[2];                              // (restart intervals: [0] = an interval ended early)
    int end_p;
    int bad;
};
using JpShared = JpSharedT<3>;

// The table entry of the symbol whose code starts the 32-bit window x (0: no such code)
__device__ __forceinline__ unsigned jp_lookup(const JpLut& L, unsigned x, bool ac) {
    const unsigned k = x >> (32 - JP_FAST);
    unsigned e = L.fast[k];
    if (!e) {
        if (k >= (1u << JP_FAST) - JP_LONG) {
            e = L.second[((k - ((1u << JP_FAST) - JP_LONG)) << (16 - JP_FAST)) + ((x >> 16) & ((1u << (16 - JP_FAST)) - 1))];
        } else if (!L.covered) {
            for (int l = JP_FAST + 1; l <= 16; ++l) {
                const int code = (int)(x >> (32 - l));
                if (code <= L.maxcode[l]) {
                    e = jp_entry(L.vals[(code + L.valoff[l]) & 255], (unsigned)l, ac);
                    break;
                }
            }
        }
    }
    return e;
}

__device__ __forceinline__ int jp_comp(unsigned blk, int hv) { return blk < (unsigned)hv ? 0 : (int)blk - hv + 1; }

// One subsequence: symbols from state (p, bz) while p < end. WRITE: also stores the coefficients of blocks ablk, ablk+1, ...
// (stops behind block `total` - 1). Returns the number of blocks completed.
// GLOBAL: the words come straight from the image's segment in memory (restart intervals: a thread walks a whole interval).
template <bool WRITE, bool GLOBAL = false, class Sh = JpShared>
__device__ __forceinline__ int jp_decode(Sh& sh, unsigned cw0, int bpm, int hv, unsigned& p, unsigned& bz, unsigned end,
                                         short* __restrict__ coef, long long ablk, long long total,
                                         const unsigned* __restrict__ src = nullptr, unsigned nwords = 0) {
    unsigned blk = bz >> 8, z = bz & 255;
    int done = 0;
    unsigned cur = ~0u, w0 = 0, w1 = 0;
    int comp = blk < (unsigned)hv ? 0 : (int)blk - hv + 1;
    while (p < end) {
        const unsigned gw = p >> 5;
        if (gw != cur) {
            cur = gw;
            if (GLOBAL) {
                w0 = gw < nwords ? __builtin_bswap32(src[gw]) : 0u;
                w1 = gw + 1 < nwords ? __builtin_bswap32(src[gw + 1]) : 0u;
            } else {
                const unsigned r = gw - cw0;
                w0 = sh.words[r + (r >> 5)];               // (word i sits at i + i / 32)
                w1 = sh.words[r + 1 + ((r + 1) >> 5)];
            }
        }
        const unsigned x = (unsigned)(((((unsigned long long)w0) << 32) | w1) << (p & 31) >> 32);
        const bool ac = z != 0;
        const JpLut& L = sh.lut[comp * 2 + (ac ? 1 : 0)];
        const unsigned e = jp_lookup(L, x, ac);
        if (!e) {                            // no such code: a wrong start state's garbage (discarded) or a corrupt file
            if (WRITE) sh.bad = 1;
            p += 1;
            continue;
        }
        if (WRITE) {
            const unsigned s = JP_S(e);
            int v = 0;
            if (s) {
                v = (int)((x << (JP_ADV(e) - s)) >> (32 - s));
                if (v < (1 << (s - 1))) v -= (1 << s) - 1;
            }
            if (!ac) {
                coef[ablk * 64] = (short)v;
            } else if (s) {
                const unsigned k = z + JP_DZ(e) - 1;
                coef[ablk * 64 + (k < 64 ? sh.nat[k] : 63)] = (short)v;
            }
        }
        p += JP_ADV(e);
        z += JP_DZ(e);
        if (z >= 64) {
            z = 0;
            blk = blk + 1 == (unsigned)bpm ? 0 : blk + 1;
            comp = blk < (unsigned)hv ? 0 : (int)blk - hv + 1;
            ++done;
            if (WRITE) {
                ++ablk;
                if (ablk >= total) {
                    sh.end_p = (int)p;
                    break;
                }
            }
        }
    }
    bz = (blk << 8) | z;
    return done;
}

// The same walk as jp_decode<false>, by a whole WAVE for ONE subsequence (all arguments wave-uniform): when only one or two
// threads of a wave have anything to re-decode - always, on images whose subsequences do not re-synchronise - a lane's serial
// chain of look-ups (window -> LDS -> length -> next window, ~470 cycles per symbol) is the whole kernel's time. Here the 64
// lanes look up the entries of the 64 bit offsets behind p at once, and the chain that is left is a scalar walk over registers:
// v_readlane of the entry at the current offset, add its bit count, step the coefficient index. A window ends after 64 bits or
// with its block (the next block may use other tables).
constexpr int JP_WIN = 4;          // 64-bit pieces of a wave's window: the look-ups of all pieces are in flight together, so the
                                   // two LDS round trips in front of a walk are paid once per JP_WIN * 64 bits
template <class Sh>
__device__ __forceinline__ int jp_decode_wave(Sh& sh, unsigned cw0, int bpm, int hv, unsigned& p_, unsigned& bz_, unsigned end) {
    const unsigned lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    unsigned p = p_, blk = bz_ >> 8, z = bz_ & 255;
    int done = 0;
    while (p < end) {
        const int c = jp_comp(blk, hv);
        unsigned x[JP_WIN], a[JP_WIN];
#pragma unroll
        for (int h = 0; h < JP_WIN; ++h) {
            const unsigned q = p + 64u * h + lane;
            unsigned r = (q >> 5) - cw0;
            r = r < JP_T * 32u + 6u ? r : JP_T * 32u + 6u;                            // (behind the staged words: never walked)
            const unsigned w0 = sh.words[r + (r >> 5)], w1 = sh.words[r + 1 + ((r + 1) >> 5)];    // (word i sits at i + i / 32)
            x[h] = (unsigned)(((((unsigned long long)w0) << 32) | w1) << (q & 31) >> 32);
        }
#pragma unroll
        for (int h = 0; h < JP_WIN; ++h) {
            const unsigned e = jp_lookup(sh.lut[2 * c + 1], x[h], true);
            a[h] = e ? JP_ADV(e) | (JP_DZ(e) << 16) : 1u;                // (no such code: one bit on, no step - as jp_decode)
        }
        const unsigned room = end - p < 64u * JP_WIN ? end - p : 64u * JP_WIN;
        unsigned o = 0;
        if (z == 0) {                                    // the block's DC symbol starts the window
            const unsigned e = __builtin_amdgcn_readfirstlane(jp_lookup(sh.lut[2 * c], x[0], false));
            if (!e) {
                p += 1;
                continue;
            }
            o = JP_ADV(e);
            z = 1;
        }
        // AC symbols up to the window's or the block's end, piece by piece. The walk's state is ONE register - the offset, biased
        // so that bit 15 comes up at the piece's limit, and the coefficient index from bit 16, where 64 is bit 22 - and an entry is
        // (bits to skip | index step << 16): a symbol is a v_readlane, an add and a test.
#pragma unroll
        for (int h = 0; h < JP_WIN; ++h) {
            const unsigned lim = room < 64u * (h + 1) ? room : 64u * (h + 1);
            if ((o < lim) & (z < 64)) {
                const unsigned bias = 0x8000u - lim;
                unsigned st = (o + bias) | (z << 16);
                do {
                    st += __builtin_amdgcn_readlane(a[h], (st & 0x7fffu) - bias - 64u * h);
                } while (!(st & 0x00c08000u));
                o = (st & 0xffffu) - bias;
                z = st >> 16;
            }
        }
        if (z >= 64) {
            z = 0;
            blk = blk + 1 == (unsigned)bpm ? 0 : blk + 1;
            ++done;
        }
        p += o;
    }
    p_ = p;
    bz_ = (blk << 8) | z;
    return done;
}

// (a four-component record's eight tables in LDS: 47 KB with the chunk's words, against 40 KB)
template <class Im>
__global__ void __launch_bounds__(JP_T) jpeg_huffman_kernel(const unsigned char* __restrict__ streams, const Im* __restrict__ images,
                                                           const JpLut* __restrict__ luts, short* __restrict__ coef_all,
                                                           int* __restrict__ status) {
    __shared__ JpSharedT<Im::NC> sh;
    const Im& im = images[blockIdx.x];
    const int tid = threadIdx.x;
    const JpegGeom g = jpeg_geom(&im);
    // Four components that all name ONE pair of tables - what Pillow's encoder writes for CMYK: the block within the MCU then
    // decides nothing about a symbol, but as part of the state it would keep subsequences from ever agreeing with their
    // predecessors (a start that guessed block 0 stays off by a constant, with nothing in the data to correct it), and every image
    // would take the serial walk. Such a record is walked as one component's blocks (hv = bpm = 1: the state is bit position and
    // coefficient index, as for a grey file); only the block counts (rbpm) keep the real MCU.
    bool one_pair = false;
    if constexpr (Im::NC == 4)
        one_pair = im.dc_tbl[1] == im.dc_tbl[0] && im.dc_tbl[2] == im.dc_tbl[0] && im.dc_tbl[3] == im.dc_tbl[0] &&
                   im.ac_tbl[1] == im.ac_tbl[0] && im.ac_tbl[2] == im.ac_tbl[0] && im.ac_tbl[3] == im.ac_tbl[0];
    const int hv = one_pair ? 1 : g.hv, bpm = one_pair ? 1 : g.bpm;
    const int rbpm = Im::NC == 4 ? g.bpm : bpm;            // blocks per MCU of the image (bpm: of the walk)
    const long long nmcu = g.nmcu, total = nmcu * rbpm;
    const unsigned nbits = (unsigned)im.stream_bytes * 8u;
    short* coef = coef_all + im.coef_off * 64;
    const unsigned* src = reinterpret_cast<const unsigned*>(streams + im.stream_off);
    const unsigned nwords = ((unsigned)im.stream_bytes + 3u) >> 2;

    for (int c = 0; c < im.ncomp; ++c) {
        const uint4* d = reinterpret_cast<const uint4*>(&luts[im.dc_tbl[c]]);
        const uint4* a = reinterpret_cast<const uint4*>(&luts[im.ac_tbl[c]]);
        uint4* dd = reinterpret_cast<uint4*>(&sh.lut[2 * c]);
        uint4* da = reinterpret_cast<uint4*>(&sh.lut[2 * c + 1]);
        for (int i = tid; i < (int)(sizeof(JpLut) / 16); i += JP_T) {
            dd[i] = d[i];
            da[i] = a[i];
        }
    }
    if (tid < 64) sh.nat[tid] = jp_natural[tid];
    if (tid == 0) {
        sh.end_p = -1;
        sh.bad = im.width < 1;                          // (the empty image jpeg_unstuff_kernel left for a record it refused: status 1)
    }
    if (im.stuffed == 2) {                              // jpeg_unstuff_kernel found a marker inside the scan
        if (tid == 0) status[blockIdx.x] = 3;
        return;
    }
    if (im.restart_interval > 0) {
        // Restart intervals: every interval starts on a byte the host knows, with fresh DC predictions, and its first block is
        // k * interval * blocks per MCU - independent chains, one thread each, no synchronisation to find.
        if (tid == 0) sh.first[0] = 0;
        __syncthreads();
        const unsigned* offs = reinterpret_cast<const unsigned*>(streams + im.intervals_off);
        const long long ri = im.restart_interval;
        for (int k = tid; k < im.n_intervals; k += JP_T) {
            unsigned p = offs[k] * 8u, bz = 0;
            const unsigned end = (k + 1 < im.n_intervals ? offs[k + 1] : (unsigned)im.stream_bytes) * 8u;
            const long long left = nmcu - k * ri, want = (left < ri ? left : ri) * rbpm;
            const int done = end <= nbits && p <= end
                                 ? jp_decode<true, true>(sh, 0, bpm, hv, p, bz, end, coef, k * ri * rbpm, k * ri * rbpm + want, src, nwords)
                                 : -1;
            if (done != want || p > end) sh.first[0] = 1;          // the interval's data ended early or ran over
        }
        __syncthreads();
        if (tid == 0) status[blockIdx.x] = sh.bad ? 1 : (sh.first[0] || (long long)im.n_intervals * ri < nmcu ? 2 : 0);
        return;
    }
    JpState carry{0u, 0u};
    long long carry_blocks = 0;
    const unsigned nsub = (nbits + JP_SUB_BITS - 1) / JP_SUB_BITS;
    for (unsigned c0 = 0; c0 < nsub && carry_blocks < total; c0 += JP_T) {
        __syncthreads();                                   // the previous chunk's readers are done with sh.words
        const unsigned cw0 = c0 * 32u;
        for (unsigned r = tid; r < (unsigned)JP_T * 32u + 8u; r += JP_T) {      // the chunk's words + 8 of the next chunk
            const unsigned g = cw0 + r;
            sh.words[r + (r >> 5)] = g < nwords ? __builtin_bswap32(src[g]) : 0u;
        }
        const unsigned i = c0 + tid;
        const bool act = i < nsub;
        const unsigned end = (i + 1) * JP_SUB_BITS < nbits ? (i + 1) * JP_SUB_BITS : nbits;
        JpState start = tid ? JpState{i * JP_SUB_BITS, 0u} : carry;
        JpState ex = start;
        int nb = 0;
        __syncthreads();
        if (act) nb = jp_decode<false>(sh, cw0, bpm, hv, ex.p, ex.bz, end, nullptr, 0, 0);
        sh.exit_state[tid] = ex;
        // Rounds. JP_SPEC speculative ones: every thread whose predecessor's exit state moved decodes again - on photographs that
        // is all it takes. When states still move after that (noise: nothing re-synchronises), wave 0 walks the rest of the chunk
        // ALONE, one subsequence after the other from the first thread whose predecessor moved (jp_decode_wave; a subsequence whose
        // start did not move is skipped): no barrier, no exchange per subsequence - everything in front of that thread is final,
        // everything behind it would decode garbage, and a round per subsequence cost more than its walk. Either way the fixed
        // point is the sequential decode: thread 0 is exact, and a thread that decodes from a final predecessor is final.
        bool moving = true;
        for (int round = 0; round < JP_SPEC && moving; ++round) {
            __syncthreads();
            const JpState prev = tid ? sh.exit_state[tid - 1] : carry;
            const bool ch = act && tid && (prev.p != start.p || prev.bz != start.bz);
            moving = __syncthreads_or(ch);
            if (!moving) break;
            const unsigned long long m = __ballot(ch);
            if (__popcll(m) <= 2) {                        // (wave-uniform) the whole wave walks each of them: jp_decode_wave
                unsigned long long mm = m;
                while (mm) {
                    const int b = __builtin_ctzll(mm);
                    mm &= mm - 1;
                    unsigned sp = __builtin_amdgcn_readlane(prev.p, b), sbz = __builtin_amdgcn_readlane(prev.bz, b);
                    const unsigned se = __builtin_amdgcn_readlane(end, b);
                    const int d = jp_decode_wave(sh, cw0, bpm, hv, sp, sbz, se);
                    if ((tid & 63) == b) {
                        start = prev;
                        ex = JpState{sp, sbz};
                        nb = d;
                        sh.exit_state[tid] = ex;
                    }
                }
            } else if (ch) {
                start = prev;
                ex = start;
                nb = jp_decode<false>(sh, cw0, bpm, hv, ex.p, ex.bz, end, nullptr, 0, 0);
                sh.exit_state[tid] = ex;
            }
        }
        if (moving) {
            sh.start_state[tid] = start;
            sh.blocks[tid] = nb;
            __syncthreads();
            if (tid < 64) {
                const unsigned nact = nsub - c0 < (unsigned)JP_T ? nsub - c0 : (unsigned)JP_T;
                JpState run = carry;
                bool fresh = false;                       // `run` comes from a subsequence this walk decoded
                for (unsigned i = 1; i < nact; ++i) {
                    const JpState pe = fresh ? run : sh.exit_state[i - 1], st = sh.start_state[i];
                    if (pe.p == st.p && pe.bz == st.bz) {  // consistent with its predecessor: its exit state stands
                        fresh = false;
                        continue;
                    }
                    unsigned sp = __builtin_amdgcn_readfirstlane(pe.p), sbz = __builtin_amdgcn_readfirstlane(pe.bz);    // (wave-uniform)
                    const unsigned se = (c0 + i + 1) * JP_SUB_BITS < nbits ? (c0 + i + 1) * JP_SUB_BITS : nbits;
                    const int d = jp_decode_wave(sh, cw0, bpm, hv, sp, sbz, se);
                    if (tid == 0) {
                        sh.start_state[i] = pe;
                        sh.exit_state[i] = JpState{sp, sbz};
                        sh.blocks[i] = d;
                    }
                    run = JpState{sp, sbz};
                    fresh = true;
                }
            }
            __syncthreads();
            start = sh.start_state[tid];
            ex = sh.exit_state[tid];
            nb = sh.blocks[tid];
            __syncthreads();                               // sh.blocks is rewritten below
        }
        // first block of every subsequence: exclusive scan of the blocks completed
        sh.blocks[tid] = act ? nb : 0;
        __syncthreads();
        for (int d = 1; d < JP_T; d <<= 1) {
            const int add = tid >= d ? sh.blocks[tid - d] : 0;
            __syncthreads();
            sh.blocks[tid] += add;
            __syncthreads();
        }
        const long long first = carry_blocks + sh.blocks[tid] - (act ? nb : 0);
        if (act && first < total) {
            JpState w = start;
            jp_decode<true>(sh, cw0, bpm, hv, w.p, w.bz, end, coef, first, total);
        }
        carry_blocks += sh.blocks[JP_T - 1];
        const unsigned last = (nsub - c0 < (unsigned)JP_T ? nsub - c0 : (unsigned)JP_T) - 1;
        carry = sh.exit_state[last];
    }
    __syncthreads();
    if (tid == 0) {
        int st = 0;
        if (sh.bad) st = 1;
        else if (carry_blocks < total || sh.end_p < 0 || (unsigned)sh.end_p > nbits) st = 2;
        status[blockIdx.x] = st;
    }
}

// DC prediction (jdhuff.c: last_dc_val per component): running sums over the blocks in scan order
template <class Im>
__global__ void __launch_bounds__(256) jpeg_dc_kernel(const Im* __restrict__ images, short* __restrict__ coef_all) {
    constexpr int NC = Im::NC;
    __shared__ int part[NC][256];
    const Im& im = images[blockIdx.x];
    const int tid = threadIdx.x;
    const JpegGeom g = jpeg_geom(&im);
    const int hv = g.hv, bpm = g.bpm;
    const long long nmcu = g.nmcu;
    const long long per = (nmcu + 255) / 256;
    const long long m0 = per * tid, m1 = m0 + per < nmcu ? m0 + per : nmcu;
    short* coef = coef_all + im.coef_off * 64;
    if (im.restart_interval > 0) {                      // predictions start at 0 in every restart interval: a thread per interval
        const long long ri = im.restart_interval;
        for (long long k = tid; k * ri < nmcu; k += 256) {
            int run[NC] = {};
            const long long e = (k + 1) * ri < nmcu ? (k + 1) * ri : nmcu;
            for (long long m = k * ri; m < e; ++m)
                for (int b = 0; b < bpm; ++b) {
                    const int c = b < hv ? 0 : b - hv + 1;
                    run[c] += coef[(m * bpm + b) * 64];
                    coef[(m * bpm + b) * 64] = (short)run[c];
                }
        }
        return;
    }
    int s[NC] = {};
    for (long long m = m0; m < m1; ++m)
        for (int b = 0; b < bpm; ++b) s[b < hv ? 0 : b - hv + 1] += coef[(m * bpm + b) * 64];
    for (int c = 0; c < NC; ++c) part[c][tid] = s[c];
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        int a[NC];
        for (int c = 0; c < NC; ++c) a[c] = tid >= d ? part[c][tid - d] : 0;
        __syncthreads();
        for (int c = 0; c < NC; ++c) part[c][tid] += a[c];
        __syncthreads();
    }
    int run[NC];
    for (int c = 0; c < NC; ++c) run[c] = part[c][tid] - s[c];
    for (long long m = m0; m < m1; ++m)
        for (int b = 0; b < bpm; ++b) {
            const int c = b < hv ? 0 : b - hv + 1;
            run[c] += coef[(m * bpm + b) * 64];
            coef[(m * bpm + b) * 64] = (short)run[c];
        }
}

// jidctint.c jpeg_idct_islow: one dimension of the LL&M butterfly (CONST_BITS = 13), results descaled by `SHIFT`
template <int SHIFT>
__device__ __forceinline__ void jp_idct8(const int* v, int stride, int* o, int ostride) {
    int z2 = v[2 * stride], z3 = v[6 * stride];
    int z1 = (z2 + z3) * 4433;
    const int t2 = z1 - z3 * 15137, t3 = z1 + z2 * 6270;
    const int t0 = (v[0] + v[4 * stride]) << 13, t1 = (v[0] - v[4 * stride]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int o0 = v[7 * stride], o1 = v[5 * stride], o2 = v[3 * stride], o3 = v[stride];
    z1 = o0 + o3;
    z2 = o1 + o2;
    z3 = o0 + o2;
    int z4 = o1 + o3;
    const int z5 = (z3 + z4) * 9633;
    o0 *= 2446;
    o1 *= 16819;
    o2 *= 25172;
    o3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o0 += z1 + z3;
    o1 += z2 + z4;
    o2 += z2 + z3;
    o3 += z1 + z4;
    constexpr int R = 1 << (SHIFT - 1);
    o[0] = (t10 + o3 + R) >> SHIFT;
    o[7 * ostride] = (t10 - o3 + R) >> SHIFT;
    o[ostride] = (t11 + o2 + R) >> SHIFT;
    o[6 * ostride] = (t11 - o2 + R) >> SHIFT;
    o[2 * ostride] = (t12 + o1 + R) >> SHIFT;
    o[5 * ostride] = (t12 - o1 + R) >> SHIFT;
    o[3 * ostride] = (t13 + o0 + R) >> SHIFT;
    o[4 * ostride] = (t13 - o0 + R) >> SHIFT;
}

// Status 4: a block outside the range where Pillow's IDCT provably equals this one. libjpeg-turbo runs jpeg_idct_islow in one of
// two forms, chosen by the CPU it runs on, and both equal int32 arithmetic + a clamp to [0, 255] only on a bounded range:
//   * SIMD (jidctint-sse2 / -avx2): the dequantisation is a 16-bit multiply (pmullw: the low 16 bits), the pass-1 outputs are
//     packed to 16 bits with saturation (packssdw; the all-zero-AC column shortcut shifts 16-bit words left instead), and the
//     sums in0 +- in4, in3 + in7, in1 + in5 of each pass are 16-bit adds (paddw: wrap). Pass 2's outputs are saturated to 8
//     bits (packssdw, packsswb) before the +128: a clamp.
//   * C (jidctint.c): int dequantisation and workspace, but the output is range_limit[x & RANGE_MASK] - the clamp for
//     x in [-512, 511] only (MAXJSAMPLE * 4 + 3 = 1023; outside it the table wraps).
// So: every dequantised coefficient and every pass-1 output an int16, every pass-2 output in [-512, 511]. That covers the 16-bit
// sums too: as a linear function of the eight outputs of a pass (the 1-D transform inverted), an input pair's sum is at most
// 0.31 x the largest |output| in pass 1 (<= 10 031 for int16 outputs) and 39.2 x in pass 2 (<= 20 061 for outputs in
// [-512, 511]), rounding included. And this kernel's own int32 arithmetic is exact there: with |inputs| <= 32 768 the largest row sum of the 1-D
// transform's coefficients (61 214) keeps every pre-shift output under 2^31, so the wrap-around of any partial sum cancels.
// A file outside the range goes back to Pillow (status 4) - whatever the SIMD level of the machine that decodes it there.
// Files Pillow encodes itself stay far inside it (tests/test_jpeg.py).
template <class Im>
__global__ void __launch_bounds__(128) jpeg_idct_kernel(const Im* __restrict__ images, const short* __restrict__ coef_all,
                                                        unsigned char* __restrict__ planes, int* __restrict__ status) {
    const Im& im = images[blockIdx.y];
    const JpegGeom g = jpeg_geom(&im, planes);
    const int hs = g.hs, vs = g.vs, hv = g.hv, bpm = g.bpm, mx = g.mx;
    const long long b = (long long)blockIdx.x * 128 + threadIdx.x;
    if (b >= g.nmcu * bpm) return;
    const long long mcu = b / bpm;
    const int k = (int)(b - mcu * bpm);
    const int comp = k < hv ? 0 : k - hv + 1;
    const int mcx = (int)(mcu % mx), mcy = (int)(mcu / mx);
    int bx, by, pw;
    unsigned char* plane = const_cast<unsigned char*>(g.py);    // (this kernel writes the planes the others read)
    if (comp == 0) {
        bx = mcx * hs + k % hs;
        by = mcy * vs + k / hs;
        pw = g.yw;
    } else {
        bx = mcx;
        by = mcy;
        pw = g.cw;
        plane += g.plane_off(comp);
    }
    const uint4* cp = reinterpret_cast<const uint4*>(coef_all + (im.coef_off + b) * 64);
    int x[64], ws[64];
    unsigned out16 = 0, out10 = 0;           // nonzero: a value left int16 / [-512, 511] (status 4)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 q = cp[i];
        const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x[i * 8 + 2 * j] = (int)(short)(u[j] & 0xffff) * im.quant[comp][i * 8 + 2 * j];
            x[i * 8 + 2 * j + 1] = ((int)u[j] >> 16) * im.quant[comp][i * 8 + 2 * j + 1];
            out16 |= ((unsigned)x[i * 8 + 2 * j] + 32768u) | ((unsigned)x[i * 8 + 2 * j + 1] + 32768u);
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) jp_idct8<11>(x + c, 8, ws + c, 8);       // pass 1: columns (CONST_BITS - PASS1_BITS)
#pragma unroll
    for (int i = 0; i < 64; ++i) out16 |= (unsigned)ws[i] + 32768u;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        int o[8];
        jp_idct8<18>(ws + r * 8, 1, o, 1);                                // pass 2: rows (CONST_BITS + PASS1_BITS + 3)
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            out10 |= ((unsigned)o[j] + 512u) | ((unsigned)o[4 + j] + 512u);
            int a = o[j] + 128, c2 = o[4 + j] + 128;
            a = a < 0 ? 0 : (a > 255 ? 255 : a);
            c2 = c2 < 0 ? 0 : (c2 > 255 ? 255 : c2);
            lo |= (unsigned)a << (8 * j);
            hi |= (unsigned)c2 << (8 * j);
        }
        *reinterpret_cast<uint2*>(plane + (size_t)(by * 8 + r) * pw + bx * 8) = make_uint2(lo, hi);
    }
    if (((out16 >> 16) | (out10 >> 10)) && status[blockIdx.y] == 0) status[blockIdx.y] = 4;     // (the first error found stands)
}

// ---- A pixel from the planes: the file's one statement of jdsample.c's fancy (triangle) upsampling, with jdmainct.c's context
// rows duplicated at the image's edges, and of jdcolor.c's 16-bit fixed-point YCbCr -> RGB. jpeg_color_kernel and the transform
// entries' jpeg_color_resize_h_kernel both compute their pixels here, so the two paths cannot drift apart.
__device__ __forceinline__ unsigned jp_rgb(int Y, int cbs, int crs) {          // -> R | G << 8 | B << 16
    const int cb = cbs - 128, cr = crs - 128;             // jdcolor.c build_ycc_rgb_table: FIX(1.402), FIX(0.34414), ...
    int r = Y + ((91881 * cr + 32768) >> 16);
    int g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    int b = Y + ((116130 * cb + 32768) >> 16);
    r = r < 0 ? 0 : (r > 255 ? 255 : r);
    g = g < 0 ? 0 : (g > 255 ? 255 : g);
    b = b < 0 ? 0 : (b > 255 ? 255 : b);
    return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16);
}

// The chroma sample of source column x: r0 = the chroma row of the pixel's own row, r1 = the context row (2x2 only), both indexed
// by chroma column - `off`. mode (JpegGeom): JM_COPY, JM_H2V1 h2v1_fancy_upsample, JM_H2V2 h2v2_fancy_upsample
__device__ __forceinline__ int jp_chroma(const unsigned char* r0, const unsigned char* r1, int off, int x, int dw, int mode) {
    if (mode == JM_COPY) return r0[x - off];
    const int cx = x >> 1, i = cx - off;
    if (mode == JM_H2V1) {
        const int p = r0[i];
        if (x & 1) return cx == dw - 1 ? p : (3 * p + r0[i + 1] + 2) >> 2;
        return cx == 0 ? p : (3 * p + r0[i - 1] + 1) >> 2;
    }
    const int s = 3 * r0[i] + r1[i];
    if (x & 1) return cx == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * r0[i + 1] + r1[i + 1] + 7) >> 4;
    return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * r0[i - 1] + r1[i - 1] + 8) >> 4;
}

__device__ __forceinline__ int jp_context_row(const JpegGeom& g, int y) {      // h2v2, h1v2: the other chroma row of source row y
    const int cy = y >> 1;
    return (y & 1) ? (cy + 1 < g.dh ? cy + 1 : g.dh - 1) : (cy > 0 ? cy - 1 : 0);
}

// jp_chroma for any mode: also JM_H1V2 h1v2_fancy_upsample (r1: the context row; k: the rounding bias, 1 in
// an even row and 2 in an odd one; no horizontal filtering, at any width) and JM_REPL int_upsample (k: JpegGeom.sx)
__device__ __forceinline__ int jp_chroma_more(const unsigned char* r0, const unsigned char* r1, int off, int x, int dw, int samp, int k) {
    if (samp == JM_H1V2) return (3 * r0[x - off] + r1[x - off] + k) >> 2;
    if (samp == JM_REPL) return r0[(x >> k) - off];
    return jp_chroma(r0, r1, off, x, dw, samp);
}

// The pixel of three upsampled samples: jdcolor.c's conversion, or none for an RGB-coded file (JpegGeom.rgb). Both are computed and
// one is selected, so that the record's transform is needed only here, behind the loads of the samples.
__device__ __forceinline__ unsigned jp_color(bool rgb, int c0, int c1, int c2) {
    const unsigned v = jp_rgb(c0, c1, c2), raw = (unsigned)c0 | ((unsigned)c1 << 8) | ((unsigned)c2 << 16);
    return rgb ? raw : v;
}

// jp_pixel for the modes behind the first three: a colour pixel of luma sample Y
__device__ __forceinline__ unsigned jp_pixel_more(const JpegGeom& g, int x, int y, int Y) {
    const bool vfancy = g.mode == JM_H1V2;
    const int cy = y >> g.sy, oy = vfancy ? jp_context_row(g, y) : cy;
    const int k = vfancy ? 1 + (y & 1) : g.sx;
    int cc[2];
    for (int c = 0; c < 2; ++c) cc[c] = jp_chroma_more(g.pc[c] + (size_t)cy * g.cw, g.pc[c] + (size_t)oy * g.cw, 0, x, g.dw, g.mode, k);
    return jp_color(g.rgb, Y, cc[0], cc[1]);
}

// One pixel (x, y) of the image straight from the planes in memory
__device__ __forceinline__ unsigned jp_pixel(const JpegGeom& g, int x, int y) {
    const int Y = g.py[(size_t)y * g.yw + x];
    if (!g.color) return (unsigned)Y * 0x010101u;
    int cc[2];
    // (the sampling decided once for both chroma planes, a constant for jp_chroma in each branch: with jp_chroma left to decide per
    // plane, jpeg_color_kernel took 8.5 instead of 8.1 ms over 435 photos of 2 000 x 1 500)
    if (g.mode == JM_COPY) {
        for (int c = 0; c < 2; ++c) cc[c] = jp_chroma(g.pc[c] + (size_t)y * g.cw, nullptr, 0, x, g.dw, JM_COPY);
    } else if (g.mode == JM_H2V1) {
        for (int c = 0; c < 2; ++c) cc[c] = jp_chroma(g.pc[c] + (size_t)y * g.cw, nullptr, 0, x, g.dw, JM_H2V1);
    } else if (g.mode == JM_H2V2) {
        const int cy = y >> 1, oy = jp_context_row(g, y);
        for (int c = 0; c < 2; ++c) cc[c] = jp_chroma(g.pc[c] + (size_t)cy * g.cw, g.pc[c] + (size_t)oy * g.cw, 0, x, g.dw, JM_H2V2);
    } else {
        return jp_pixel_more(g, x, y, Y);
    }
    return jp_color(g.rgb, Y, cc[0], cc[1]);
}

__device__ __forceinline__ unsigned jp_pixel_clamped(const JpegGeom& g, int x, int y) {       // coordinates clamped into the image
    return jp_pixel(g, x < 0 ? 0 : (x >= g.W ? g.W - 1 : x), y < 0 ? 0 : (y >= g.H ? g.H - 1 : y));
}

__global__ void __launch_bounds__(256) jpeg_color_kernel(const JpegImage* __restrict__ images, const unsigned char* __restrict__ planes,
                                                         unsigned char* __restrict__ out) {
    const JpegImage& im = images[blockIdx.y];
    const JpegGeom g = jpeg_geom(&im, planes);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)g.W * g.H) return;
    const int y = (int)(idx / g.W), x = (int)(idx - (long long)y * g.W);
    const unsigned v = jp_pixel(g, x, y);
    unsigned char* o = out + im.out_off + ((size_t)y * g.W + x) * 3;
    o[0] = (unsigned char)v; o[1] = (unsigned char)(v >> 8); o[2] = (unsigned char)(v >> 16);
}

// ---- Four-component files (clipmi_jpeg_decode_cmyk8): Pillow's mode-CMYK bytes, rows of width*4. Pillow reads libjpeg's CMYK
// output with rawmode CMYK;I - every byte inverted - whatever the markers say. With p0..p3 the four upsampled samples (components
// 1-3 upsampled exactly as chroma is, per plane: jp_chroma_more):
//   transform 2, CMYK as stored: libjpeg copies the samples        -> (255 - p0, 255 - p1, 255 - p2, 255 - p3)
//   transform 3, YCCK: jdcolor.c ycck_cmyk_convert gives (255 - R, 255 - G, 255 - B, p3) with R, G, B jp_rgb's of (p0, p1, p2)
//                                                                   -> (R, G, B, 255 - p3)
// One pixel per thread, the four bytes in one store where the image's rows are 4-byte aligned.
__global__ void __launch_bounds__(256) jpeg_cmyk_kernel(const JpegImage4* __restrict__ images, const unsigned char* __restrict__ planes,
                                                        unsigned char* __restrict__ out) {
    const JpegImage4& im = images[blockIdx.y];
    const JpegGeom g = jpeg_geom(&im, planes);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (!g.color || idx >= (long long)g.W * g.H) return;        // (a record jpeg_unstuff_kernel emptied has no pixels)
    const int y = (int)(idx / g.W), x = (int)(idx - (long long)y * g.W);
    const int p0 = g.py[(size_t)y * g.yw + x];
    const bool vfancy = g.mode == JM_H2V2 || g.mode == JM_H1V2;
    const int cy = y >> g.sy, oy = vfancy ? jp_context_row(g, y) : cy;
    const int k = g.mode == JM_H1V2 ? 1 + (y & 1) : g.sx;      // jp_chroma_more's last argument
    int p[3];
    for (int c = 0; c < 3; ++c) {
        const unsigned char* pl = g.py + g.plane_off(c + 1);
        p[c] = jp_chroma_more(pl + (size_t)cy * g.cw, pl + (size_t)oy * g.cw, 0, x, g.dw, g.mode, k);
    }
    const unsigned stored = ~((unsigned)p0 | ((unsigned)p[0] << 8) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 24));
    const unsigned ycck = jp_rgb(p0, p[0], p[1]) | ((255u - (unsigned)p[2]) << 24);
    const unsigned v = im.transform == 3 ? ycck : stored;
    unsigned char* o = out + im.out_off + ((size_t)y * g.W + x) * 4;
    if ((reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<unsigned*>(o) = v;
    } else {
        o[0] = (unsigned char)v; o[1] = (unsigned char)(v >> 8); o[2] = (unsigned char)(v >> 16); o[3] = (unsigned char)(v >> 24);
    }
}

// ---- jpeg_color_kernel + resize_h_kernel (resize.hip) in one pass, for the transform entries: the full-size RGB image is never
// written. Only the source rows [r0, r0 + nrows) and the source columns under the n_px-wide window are converted, from the
// sample planes jpeg_idct_kernel left, and what reaches memory is what resize_h_kernel writes: the 8-bit rows between Pillow's
// two passes, scratch[tmp_off + (row * n_px + x) * 3 + c]. The arithmetic per output is that of the two kernels, in their order.
//
// A workgroup takes a job and a band of JF_ROWS source rows and walks the window in chunks of output columns. A chunk is as
// many outputs as fit its three LDS pieces: JF_SPAN source columns, JF_COEF coefficients, JF_T outputs. Per chunk:
//   stage     the band's luma bytes and the chroma rows and columns the chunk's source columns read (for 2x2 the neighbouring
//             chroma rows too), 8 bytes per load (plane rows are multiples of 8 bytes at 64-byte aligned bases), and the chunk's
//             first taps, tap counts and coefficients
//   convert   every staged source pixel once: upsampled chroma + YCbCr -> RGB into an LDS row of R | G << 8 | B << 16
//   resample  one thread per (row, output): the dot product over LDS pixels and LDS coefficients, three byte stores
// LDS use does not depend on the image's width. An output whose taps do not fit a chunk by themselves (more than JF_SPAN source
// columns or JF_COEF coefficients under ONE output: a shorter side beyond 100 x n_px) is computed tap by tap from the planes in
// memory (jp_pixel), as is any output whose first tap and count do not lie inside the staged span.
constexpr int JF_T = 256;
constexpr int JF_ROWS = 8;                 // source rows per workgroup; 2x2 chroma needs JF_ROWS / 2 + 3 <= JF_ROWS rows
constexpr int JF_SPAN = 512;               // source columns per chunk
constexpr int JF_COEF = 3072;              // coefficients per chunk
constexpr int JF_TILE_W = JF_SPAN + 16;    // staged bytes per row: the span, widened to multiples of 8 at both ends

// One tap of the horizontal pass: a pixel R | G << 8 | B << 16 times its coefficient, into the three sums
__device__ __forceinline__ void jf_tap(int (&a)[3], unsigned v, int c) {
    a[0] += (int)(v & 255u) * c; a[1] += (int)((v >> 8) & 255u) * c; a[2] += (int)(v >> 16) * c;
}

__global__ void __launch_bounds__(JF_T) jpeg_color_resize_h_kernel(const JpegImage* __restrict__ images,
                                                                   const unsigned char* __restrict__ planes,
                                                                   const clipmi_resize_job* __restrict__ jobs,
                                                                   const int* __restrict__ coef, int n_px,
                                                                   unsigned char* __restrict__ scratch) {
    __shared__ __attribute__((aligned(16))) unsigned char s_y[JF_ROWS][JF_TILE_W];
    __shared__ __attribute__((aligned(16))) unsigned char s_c[2][JF_ROWS][JF_TILE_W];
    __shared__ unsigned s_rgb[JF_ROWS][JF_SPAN];
    __shared__ int s_coef[JF_COEF];
    __shared__ int s_xmin[JF_T], s_cnt[JF_T];
    __shared__ int s_end;
    const JpegImage& im = images[blockIdx.y];
    const clipmi_resize_job j = jobs[blockIdx.y];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * JF_ROWS;
    const JpegGeom g = jpeg_geom(&im, planes);
    if (row0 >= j.nrows || g.W < 1 || g.H < 1) return;                      // (the whole workgroup)
    const int nr = j.nrows - row0 < JF_ROWS ? j.nrows - row0 : JF_ROWS;
    const int hk = j.hk > 0 ? j.hk : 0;
    const int* cf = coef + j.hcoef_off;
    unsigned char* dst = scratch + j.tmp_off + (size_t)row0 * n_px * 3;
    // the band's source rows (consecutive; clamped into the image whatever the job says)
    const int ylo = min(max(j.r0 + row0, 0), g.H - 1), yhi = min(max(j.r0 + row0 + nr - 1, 0), g.H - 1);
    // the staged chroma rows: with vertical fancy upsampling (2x2, 1x2) a band's own rows and their neighbours, <= JF_ROWS / 2 + 3;
    // else the rows y >> sy of the band's rows - the band's rows themselves (sy = 0), or at most three (1x4)
    const bool vfancy = g.mode == JM_H2V2 || g.mode == JM_H1V2, hfancy = g.mode == JM_H2V1 || g.mode == JM_H2V2;
    const int cylo = vfancy ? max((ylo >> 1) - 1, 0) : g.sy ? ylo >> g.sy : ylo;       // first staged chroma row
    const int ncr = vfancy ? min((yhi >> 1) + 1, g.dh - 1) - cylo + 1 : g.sy ? (yhi >> g.sy) - cylo + 1 : nr;

    for (int x0 = 0; x0 < n_px;) {
        // ---- the chunk: outputs [x0, x1) read the source columns [sx0, sx1)
        int x1, sx0, sx1;
        if (j.need_h) {
            sx0 = cf[x0];
            const int c = x0 + tid;                                             // the chunk may end behind output c
            int end = 0;
            bool fits = false;
            if (c < n_px) {
                end = cf[c] + cf[n_px + c];
                fits = cf[c] >= sx0 && end - sx0 <= JF_SPAN && (long long)(tid + 1) * hk <= JF_COEF;
            }
            // (first taps and ends do not decrease along an axis, so `fits` holds for a prefix of the threads; a table that breaks
            // this only sends outputs to jp_pixel below)
            const int n = __syncthreads_count(fits);
            if (fits && tid == n - 1) s_end = end;
            __syncthreads();
            x1 = x0 + (n > 0 ? n : 1);
            sx1 = n > 0 ? s_end : sx0;                                          // (n == 0: nothing staged, output x0 from memory)
        } else {
            x1 = min(x0 + JF_SPAN, n_px);
            sx0 = j.left + x0;
            sx1 = j.left + x1;
        }
        sx0 = min(max(sx0, 0), g.W);
        sx1 = min(max(sx1, sx0), min(g.W, sx0 + JF_SPAN));
        const int span = sx1 - sx0, nx = x1 - x0;
        // ---- stage
        const int yb = sx0 & ~7, ye = min((sx1 + 7) & ~7, g.yw);
        int cb = yb, ce = ye;
        if (hfancy) {
            cb = max((sx0 >> 1) - 1, 0) & ~7;
            ce = min((min(((sx1 - 1) >> 1) + 1, g.dw - 1) + 8) & ~7, g.cw);
        } else if (g.sx && span > 0) {                                          // 4x1: a quarter of the columns
            cb = (sx0 >> g.sx) & ~7;
            ce = min((((sx1 - 1) >> g.sx) + 8) & ~7, g.cw);
        }
        if (span > 0) {
            const int nu = (ye - yb) >> 3;
            for (int i = tid; i < nr * nu; i += JF_T) {
                const int r = i / nu, u = i - r * nu;
                *reinterpret_cast<uint2*>(&s_y[r][8 * u]) = *reinterpret_cast<const uint2*>(g.py + (size_t)min(ylo + r, g.H - 1) * g.yw + yb + 8 * u);
            }
            if (g.color) {
                const int nc = (ce - cb) >> 3;
                for (int i = tid; i < 2 * ncr * nc; i += JF_T) {
                    const int c = i / (ncr * nc), t = i - c * ncr * nc, r = t / nc, u = t - r * nc;
                    const int cy = vfancy || g.sy ? cylo + r : min(ylo + r, g.H - 1);
                    *reinterpret_cast<uint2*>(&s_c[c][r][8 * u]) = *reinterpret_cast<const uint2*>((c ? g.pc[1] : g.pc[0]) + (size_t)cy * g.cw + cb + 8 * u);
                }
            }
            if (j.need_h) {
                if (tid < nx) {
                    s_xmin[tid] = cf[x0 + tid];
                    s_cnt[tid] = cf[n_px + x0 + tid];
                }
                const int* kk = cf + 2 * (size_t)n_px + (size_t)x0 * hk;
                for (int i = tid; i < nx * hk; i += JF_T) s_coef[i] = kk[i];
            }
        }
        __syncthreads();
        // ---- convert
        for (int r = 0; r < nr; ++r) {
            const int y = min(ylo + r, g.H - 1);
            const int t0 = vfancy || g.sy ? (y >> g.sy) - cylo : r, t1 = vfancy ? jp_context_row(g, y) - cylo : t0;
            const int k = g.mode == JM_H1V2 ? 1 + (y & 1) : g.sx;                  // jp_chroma_more's last argument
            // (the mode decided once per row, a constant for jp_chroma in each loop, as in jp_pixel)
            const unsigned char *yr = s_y[r], *a0 = s_c[0][t0], *a1 = s_c[0][t1], *b0 = s_c[1][t0], *b1 = s_c[1][t1];
            const auto row = [&](auto&& px) {
                for (int p = tid; p < span; p += JF_T) s_rgb[r][p] = px(sx0 + p, (int)yr[sx0 + p - yb]);
            };
            if (!g.color) row([&](int, int Y) { return (unsigned)Y * 0x010101u; });
            else if (g.rgb || g.mode > JM_H2V2) row([&](int x, int Y) { return jp_color(g.rgb, Y, jp_chroma_more(a0, a1, cb, x, g.dw, g.mode, k), jp_chroma_more(b0, b1, cb, x, g.dw, g.mode, k)); });
            else if (g.mode == JM_COPY) row([&](int x, int Y) { return jp_rgb(Y, jp_chroma(a0, a1, cb, x, g.dw, JM_COPY), jp_chroma(b0, b1, cb, x, g.dw, JM_COPY)); });
            else if (g.mode == JM_H2V1) row([&](int x, int Y) { return jp_rgb(Y, jp_chroma(a0, a1, cb, x, g.dw, JM_H2V1), jp_chroma(b0, b1, cb, x, g.dw, JM_H2V1)); });
            else row([&](int x, int Y) { return jp_rgb(Y, jp_chroma(a0, a1, cb, x, g.dw, JM_H2V2), jp_chroma(b0, b1, cb, x, g.dw, JM_H2V2)); });
        }
        __syncthreads();
        // ---- resample
        for (int i = tid; i < nr * nx; i += JF_T) {
            const int r = i / nx, xo = i - r * nx;
            unsigned char* o = dst + ((size_t)r * n_px + x0 + xo) * 3;
            if (!j.need_h) {
                const int x = j.left + x0 + xo;
                const unsigned v = x >= sx0 && x < sx1 ? s_rgb[r][x - sx0] : jp_pixel_clamped(g, x, ylo + r);
                o[0] = (unsigned char)v; o[1] = (unsigned char)(v >> 8); o[2] = (unsigned char)(v >> 16);
                continue;
            }
            int a[3] = {1 << (RZ_PREC - 1), 1 << (RZ_PREC - 1), 1 << (RZ_PREC - 1)};     // as resize_h_kernel
            if (span > 0 && s_xmin[xo] >= sx0 && s_cnt[xo] >= 0 && s_cnt[xo] <= hk && s_xmin[xo] + s_cnt[xo] <= sx1) {
                const unsigned* px = &s_rgb[r][s_xmin[xo] - sx0];
                const int* kk = &s_coef[xo * hk];
                const int cnt = s_cnt[xo];
                for (int k = 0; k < cnt; ++k) jf_tap(a, px[k], kk[k]);
            } else {
                const int xmin = cf[x0 + xo], cnt = min(max(cf[n_px + x0 + xo], 0), hk);
                const int* kk = cf + 2 * (size_t)n_px + (size_t)(x0 + xo) * hk;
                for (int k = 0; k < cnt; ++k) jf_tap(a, jp_pixel_clamped(g, xmin + k, ylo + r), kk[k]);
            }
            // three byte stores, as resize_h_kernel: the packed form has been miscompiled (resize_h_rgba_kernel's comment)
            o[0] = rz_clip8(a[0]); o[1] = rz_clip8(a[1]); o[2] = rz_clip8(a[2]);
        }
        __syncthreads();                                         // the next chunk rewrites every LDS piece
        x0 = x1;
    }
}

// ---- Progressive files (SOF2, Huffman; ITU T.81 Annex G as libjpeg's jdphuff.c decodes it). The host (jpeg_parse.parse_progressive)
// hands over only files whose scan script is complete - every coefficient of every component at Al = 0 by EOI - so that
// libjpeg applies no block smoothing and the output is jpeg_idct_islow of the final coefficients. jpeg_progressive_kernel
// writes those final coefficients (absolute DC, every refinement applied) into the buffer jpeg_idct_kernel reads, in its MCU
// order; jpeg_idct_kernel and jpeg_color_kernel then run as for a baseline file (jpeg_dc_kernel does not: the walk predicts DC).
//
// Progressive symbols need the symbol itself (EOBn's run bits, a refinement's (r, s)), which the baseline entry does not keep:
// a second table form, entry = code length << 8 | symbol.
struct JppLut {
    unsigned short fast[1 << JP_FAST];   // length << 8 | symbol of codes of up to JP_FAST bits, 0 = longer (or invalid)
    int maxcode[18];
    int valoff[18];
    unsigned char vals[256];
};
static_assert(sizeof(JppLut) % 16 == 0, "tables are copied as 16-byte pieces");

struct JpegScan {              // mirrors clipmi_jpeg_scan (include/clipmi.h)
    long long stream_off;
    int stream_bytes;
    int ncomp;
    int comp[3];
    int tbl[3];
    int ss, se, ah, al;
    int reserved[2];
};

struct JpegProgImage {         // mirrors clipmi_jpeg_progressive_image
    long long coef_off, out_off;
    int width, height;
    int ncomp;
    int hs, vs;
    int first_scan, n_scans;
    int transform;             // clipmi_jpeg_progressive_image.reserved[0]: as JpegImage's
    int reserved[4];
    unsigned char quant[3][64];
};

__device__ __forceinline__ unsigned short jp_lut_entry(const JppLut&, unsigned sym, unsigned len, bool) {
    return (unsigned short)((len << 8) | sym);
}

__global__ void __launch_bounds__(256) jpeg_build_pluts_kernel(const unsigned char* __restrict__ raw, JppLut* __restrict__ luts) {
    jp_build_lut(raw + (size_t)blockIdx.x * JP_RAW, luts[blockIdx.x]);
}

// A lane's bit reader over one scan's segment: 64 bits buffered, MSB first (bits behind the segment read as zeros).
struct JppBits {
    const unsigned* src;
    unsigned nwords, wpos, p;
    unsigned long long buf;
    int nb;
    __device__ __forceinline__ void fill() {
        while (nb <= 32) {
            const unsigned w = wpos < nwords ? __builtin_bswap32(src[wpos]) : 0u;
            buf |= (unsigned long long)w << (32 - nb);
            ++wpos;
            nb += 32;
        }
    }
    __device__ __forceinline__ unsigned peek() {
        fill();
        return (unsigned)(buf >> 32);
    }
    __device__ __forceinline__ void skip(int n) {
        buf <<= n;
        nb -= n;
        p += (unsigned)n;
    }
    __device__ __forceinline__ int get(int n) {          // n <= 16
        if (!n) return 0;
        const int v = (int)(peek() >> (32 - n));
        skip(n);
        return v;
    }
    // the next Huffman symbol, -1 for no such code
    __device__ __forceinline__ int sym(const JppLut& L) {
        const unsigned x = peek();
        unsigned e = L.fast[x >> (32 - JP_FAST)];
        if (!e) {
            for (int l = JP_FAST + 1; l <= 16; ++l) {
                const int code = (int)(x >> (32 - l));
                if (code <= L.maxcode[l]) {
                    e = (unsigned)(l << 8) | L.vals[(code + L.valoff[l]) & 255];
                    break;
                }
            }
            if (!e) return -1;
        }
        skip((int)(e >> 8));
        return (int)(e & 255);
    }
};

__device__ __forceinline__ int jpp_extend(int v, int s) { return s && v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

constexpr int JPP_T = 64;            // one wave per image: its lanes walk the image's independent scan chains
constexpr int JPP_MAX_SCANS = 128;

// One workgroup (one wave) per image. Scans that share no (component, coefficient) pair do not depend on each other: lane 0
// groups the scans into chains (a scan joins every earlier scan it shares a pair with), and every lane walks whole chains,
// scan after scan, block after block - a serial walk per chain. In libjpeg's standard YCbCr script the chains are the DC
// scans, Cb's two, Cr's two and luma's four. Each chain writes only its own coefficients, so lanes never write the same int16.
// Status: 1 an invalid Huffman code, a coefficient behind its band or a record the kernel cannot take; 2 a scan's data ran out.
__global__ void __launch_bounds__(JPP_T) jpeg_progressive_kernel(const unsigned char* __restrict__ streams,
                                                                const JpegProgImage* __restrict__ pimages,
                                                                const JpegScan* __restrict__ scans_all, int nscans_all,
                                                                const JppLut* __restrict__ luts, int ntables,
                                                                JpegImage* __restrict__ images, short* __restrict__ coef_all,
                                                                int* __restrict__ status) {
    __shared__ unsigned long long mask[JPP_MAX_SCANS][3];
    __shared__ int root[JPP_MAX_SCANS];
    __shared__ int roots[JPP_MAX_SCANS];
    __shared__ int nroots, bad, ran_out;
    __shared__ unsigned char nat[80];
    const JpegProgImage& pim = pimages[blockIdx.x];
    const int tid = threadIdx.x;
    const int ncomp = pim.ncomp;
    const int nsc = pim.n_scans, s0 = pim.first_scan;
    short* coef = coef_all + pim.coef_off * 64;
    const bool valid = nsc >= 1 && nsc <= JPP_MAX_SCANS && s0 >= 0 && s0 <= nscans_all - nsc &&
                       jp_record_ok(ncomp, pim.width, pim.height, pim.hs, pim.vs, pim.transform);
    JpegImage r{};                                      // the record jpeg_idct_kernel / jpeg_color_kernel read
    r.coef_off = pim.coef_off;
    r.out_off = pim.out_off;
    r.ncomp = 1;                                        // a record outside the limits: an empty grey image, nothing to do
    r.hs = r.vs = 1;
    if (valid) {
        r.width = pim.width;
        r.height = pim.height;
        r.ncomp = ncomp;
        r.hs = pim.hs;
        r.vs = pim.vs;
        r.transform = pim.transform;
    }
    const JpegGeom g = jpeg_geom(&r);                    // (of the record written: no division by a sampling factor not checked)
    const int hs = g.hs, vs = g.vs, hv = g.hv, bpm = g.bpm, mx = g.mx, my = g.my;
    if (tid == 0) {
        if (valid)
            for (int c = 0; c < 3; ++c)
                for (int k = 0; k < 64; ++k) r.quant[c][k] = pim.quant[c][k];
        images[blockIdx.x] = r;
        bad = ran_out = 0;
        nroots = 0;
    }
    for (int k = tid; k < 80; k += JPP_T) nat[k] = k < 64 ? jp_natural[k] : 63;
    __syncthreads();
    if (!valid) {
        if (tid == 0) status[blockIdx.x] = 1;
        return;
    }
    for (int s = tid; s < nsc; s += JPP_T) {            // the (component, coefficient) pairs of every scan; records checked
        const JpegScan& sc = scans_all[s0 + s];
        bool ok = sc.ncomp >= 1 && sc.ncomp <= ncomp && sc.ss >= 0 && sc.ss <= sc.se && sc.se <= 63 && (sc.ss == 0) == (sc.se == 0) &&
                  (sc.ss == 0 || sc.ncomp == 1) && sc.al >= 0 && sc.al <= 13 && sc.stream_bytes >= 0;
        const unsigned long long band = (sc.se == 63 ? ~0ull : ((1ull << (sc.se + 1)) - 1)) & ~((1ull << sc.ss) - 1);
        unsigned long long m[3] = {0, 0, 0};
        for (int i = 0; ok && i < sc.ncomp; ++i) {
            const int c = sc.comp[i];
            ok = c >= 0 && c < ncomp && (i == 0 || c > sc.comp[i - 1]);
            if (ok && !(sc.ss == 0 && sc.ah)) ok = sc.tbl[i] >= 0 && sc.tbl[i] < ntables;
            if (ok) m[c] = band;
        }
        for (int c = 0; c < 3; ++c) mask[s][c] = m[c];
        if (!ok) bad = 1;
    }
    __syncthreads();
    if (bad) {
        if (tid == 0) status[blockIdx.x] = 1;
        return;
    }
    if (tid == 0) {                                     // chains: union of scans that share a pair (roots: the first scan of a chain)
        for (int s = 0; s < nsc; ++s) {
            int r = s;
            root[s] = s;
            for (int t = 0; t < s; ++t) {
                if (!((mask[s][0] & mask[t][0]) | (mask[s][1] & mask[t][1]) | (mask[s][2] & mask[t][2]))) continue;
                int u = t;
                while (root[u] != u) u = root[u];
                if (u < r) {
                    root[r] = u;
                    r = u;
                } else if (u > r) {
                    root[u] = r;
                }
            }
        }
        for (int s = 0; s < nsc; ++s) {
            int u = s;
            while (root[u] != u) u = root[u];
            root[s] = u;
            if (u == s) roots[nroots++] = s;
        }
    }
    __syncthreads();
    for (int ch = tid; ch < nroots; ch += JPP_T) {
        const int r = roots[ch];
        bool failed = false;
        for (int s = r; s < nsc && !failed; ++s) {
            if (root[s] != r) continue;
            const JpegScan& sc = scans_all[s0 + s];
            JppBits br{reinterpret_cast<const unsigned*>(streams + sc.stream_off), ((unsigned)sc.stream_bytes + 3u) >> 2, 0u, 0u, 0ull, 0};
            const int al = sc.al, p1 = 1 << al, m1 = -(1 << al);
            const bool inter = sc.ncomp > 1;
            // the scan's walk: interleaved - MCU after MCU, each scan component's blocks in turn; non-interleaved - the
            // component's own block grid ceil(ceil(W h / hmax) / 8) x ceil(ceil(H v / vmax) / 8) in raster order, no padding blocks
            const int c1 = sc.comp[0];
            const int cw = inter ? mx : (c1 == 0 ? (pim.width + 7) / 8 : ((pim.width + hs - 1) / hs + 7) / 8);
            const int chh = inter ? my : (c1 == 0 ? (pim.height + 7) / 8 : ((pim.height + vs - 1) / vs + 7) / 8);
            const int per = inter ? (sc.comp[0] == 0 ? hv : 1) + sc.ncomp - 1 : 1;      // blocks per unit
            const long long units = (long long)cw * chh;
            int pred[3] = {0, 0, 0};
            int eobrun = 0;
            const JppLut* lut0 = &luts[sc.tbl[0] < 0 ? 0 : sc.tbl[0]];
            for (long long u = 0; u < units && !failed; ++u) {
                const int ux = (int)(u % cw), uy = (int)(u / cw);
                for (int j = 0; j < per && !failed; ++j) {
                    long long slot;
                    int c;
                    const JppLut* L = lut0;
                    if (inter) {
                        int i = 0, k = j;                  // block j of the MCU: which scan component, which of its blocks
                        if (sc.comp[0] == 0) {
                            if (k < hv) i = 0;
                            else i = k - hv + 1, k = 0;
                        } else {
                            i = k, k = 0;
                        }
                        c = sc.comp[i];
                        slot = u * bpm + (c == 0 ? k : hv + c - 1);
                        if (sc.ah == 0) L = &luts[sc.tbl[i]];
                    } else {
                        c = c1;
                        slot = c == 0 ? ((long long)(uy / vs) * mx + ux / hs) * bpm + (uy % vs) * hs + ux % hs
                                      : ((long long)uy * mx + ux) * bpm + hv + c - 1;
                    }
                    short* blk = coef + slot * 64;
                    if (sc.ss == 0) {
                        if (sc.ah == 0) {
                            const int t = br.sym(*L);
                            if (t < 0 || t > 15) { failed = true; break; }
                            pred[c] += jpp_extend(br.get(t), t);
                            if (pred[c] > (1 << 30) || pred[c] < -(1 << 30)) { failed = true; break; }
                            blk[0] = (short)((unsigned)pred[c] << al);
                        } else if (br.get(1)) {
                            blk[0] = (short)(blk[0] | p1);
                        }
                        continue;
                    }
                    if (sc.ah == 0) {                       // AC first scan
                        if (eobrun) {
                            --eobrun;
                            continue;
                        }
                        for (int k = sc.ss; k <= sc.se; ++k) {
                            const int t = br.sym(*L);
                            if (t < 0) { failed = true; break; }
                            const int rr = t >> 4, ss = t & 15;
                            if (ss) {
                                k += rr;
                                if (k > sc.se) { failed = true; break; }
                                blk[nat[k]] = (short)((unsigned)jpp_extend(br.get(ss), ss) << al);
                            } else if (rr == 15) {
                                k += 15;
                            } else {
                                eobrun = (1 << rr) + br.get(rr) - 1;
                                break;
                            }
                        }
                        continue;
                    }
                    int k = sc.ss;                          // AC refinement
                    if (!eobrun) {
                        for (; k <= sc.se; ++k) {
                            const int t = br.sym(*L);
                            if (t < 0) { failed = true; break; }
                            int rr = t >> 4, ss = t & 15, v = 0;
                            if (ss) {
                                if (ss != 1) { failed = true; break; }
                                v = br.get(1) ? p1 : m1;
                            } else if (rr != 15) {
                                eobrun = (1 << rr) + br.get(rr);
                                break;
                            }
                            for (; k <= sc.se; ++k) {       // skip rr zeros; a correction bit for every nonzero passed
                                const int z = nat[k];
                                const int cv = blk[z];
                                if (cv) {
                                    if (br.get(1) && !(cv & p1)) blk[z] = (short)(cv + (cv >= 0 ? p1 : m1));
                                } else if (--rr < 0) {
                                    break;
                                }
                            }
                            if (v) {
                                if (k > sc.se) { failed = true; break; }
                                blk[nat[k]] = (short)v;
                            }
                        }
                        if (failed) break;
                    }
                    if (eobrun) {                           // the rest of the band in an EOB run: correction bits only
                        for (; k <= sc.se; ++k) {
                            const int z = nat[k];
                            const int cv = blk[z];
                            if (cv && br.get(1) && !(cv & p1)) blk[z] = (short)(cv + (cv >= 0 ? p1 : m1));
                        }
                        --eobrun;
                    }
                }
            }
            if (failed) bad = 1;
            else if (br.p > (unsigned)sc.stream_bytes * 8u) {
                ran_out = 1;
                failed = true;
            }
        }
    }
    __syncthreads();
    if (tid == 0) status[blockIdx.x] = bad ? 1 : (ran_out ? 2 : 0);
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" int64_t clipmi_jpeg_workspace_bytes(int64_t total_blocks, int ntables) {
    if (total_blocks < 0 || ntables < 0) return -1;
    return (int64_t)align_up((size_t)ntables * sizeof(JpLut), 256) + (int64_t)align_up((size_t)total_blocks * 128, 256) +
           (int64_t)align_up((size_t)total_blocks * 64, 256);
}

// What all four decode entries ask of the arguments they share
static bool jpeg_args_ok(const void* streams_dev, const void* images_dev, int n, const void* tables_dev, int ntables, int64_t total_blocks,
                         int64_t max_blocks, const int32_t* status_dev, const void* ws_dev) {
    return streams_dev && images_dev && tables_dev && status_dev && ws_dev && n >= 0 && ntables >= 1 && total_blocks >= 1 &&
           max_blocks >= 1 && max_blocks <= total_blocks;
}

// The baseline decode up to the sample planes (shared by the decode and the transform entry, and by the four-component decode
// entry: Im = JpegImage4 launches that record's instantiation of each kernel) -> 0 and the planes, or an error
template <class Im = JpegImage>
static int jpeg_baseline_planes(const char* who, void* streams_dev, void* images_dev, int n, const void* tables_dev, int ntables,
                                int64_t total_blocks, int64_t max_blocks, int32_t* status_dev, void* ws_dev, int64_t ws_bytes,
                                hipStream_t st, unsigned char** planes_out) {
    static_assert(sizeof(JpegImage) == sizeof(clipmi_jpeg_image) && sizeof(JpegImage) == 288, "clipmi_jpeg_image layout");
    static_assert(sizeof(JpegImage4) == sizeof(clipmi_jpeg_image4) && sizeof(JpegImage4) == 360, "clipmi_jpeg_image4 layout");
    if (ws_bytes < clipmi_jpeg_workspace_bytes(total_blocks, ntables))
        return set_err(CLIPMI_EINVAL, "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes,
                       (long long)clipmi_jpeg_workspace_bytes(total_blocks, ntables));
    if ((max_blocks + 127) / 128 > 0x7fffffffLL || n > 65535) return set_err(CLIPMI_EINVAL, "%s: batch too large for one launch", who);
    Arena ar(ws_dev, (size_t)ws_bytes);
    JpLut* luts = ar.take<JpLut>((size_t)ntables);
    short* coef = ar.take<short>((size_t)total_blocks * 64);
    unsigned char* planes = ar.take<unsigned char>((size_t)total_blocks * 64);
    Im* images = static_cast<Im*>(images_dev);
    hipLaunchKernelGGL(jpeg_unstuff_kernel<Im>, dim3((unsigned)n), dim3(256), 0, st, static_cast<unsigned char*>(streams_dev), images);
    CLIPMI_CHECK_LAUNCH("jpeg_unstuff_kernel");
    if (zero_async(coef, (size_t)total_blocks * 128, st) != hipSuccess) return set_err(CLIPMI_EHIP, "%s: zero_async", who);
    hipLaunchKernelGGL(jpeg_build_luts_kernel, dim3((unsigned)ntables), dim3(256), 0, st, static_cast<const unsigned char*>(tables_dev), luts);
    CLIPMI_CHECK_LAUNCH("jpeg_build_luts_kernel");
    const unsigned char* streams = static_cast<const unsigned char*>(streams_dev);
    const dim3 idct_grid((unsigned)((max_blocks + 127) / 128), (unsigned)n);
    hipLaunchKernelGGL(jpeg_huffman_kernel<Im>, dim3((unsigned)n), dim3(JP_T), 0, st, streams, static_cast<const Im*>(images), luts, coef,
                       status_dev);
    CLIPMI_CHECK_LAUNCH("jpeg_huffman_kernel");
    hipLaunchKernelGGL(jpeg_dc_kernel<Im>, dim3((unsigned)n), dim3(256), 0, st, static_cast<const Im*>(images), coef);
    CLIPMI_CHECK_LAUNCH("jpeg_dc_kernel");
    hipLaunchKernelGGL(jpeg_idct_kernel<Im>, idct_grid, dim3(128), 0, st, static_cast<const Im*>(images), static_cast<const short*>(coef),
                       planes, status_dev);
    CLIPMI_CHECK_LAUNCH("jpeg_idct_kernel");
    *planes_out = planes;
    return 0;
}

// The plain decode entries' tail: jpeg_color_kernel over the planes, a thread per pixel of the largest image
static int jpeg_color_tail(const char* who, const JpegImage* images, const unsigned char* planes, int n, int64_t max_pixels, void* out_dev,
                           hipStream_t st) {
    if ((max_pixels + 255) / 256 > 0x7fffffffLL) return set_err(CLIPMI_EINVAL, "%s: batch too large for one launch", who);
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((max_pixels + 255) / 256), (unsigned)n), dim3(256), 0, st, images, planes,
                       static_cast<unsigned char*>(out_dev));
    CLIPMI_CHECK_LAUNCH("jpeg_color_kernel");
    return 0;
}

extern "C" int clipmi_jpeg_decode_rgb8(void* streams_dev, void* images_dev, int n, const void* tables_dev, int ntables,
                                       int64_t total_blocks, int64_t max_blocks, int64_t max_pixels, void* out_dev, int32_t* status_dev,
                                       void* ws_dev, int64_t ws_bytes, void* stream) {
    if (n == 0) return 0;
    if (!jpeg_args_ok(streams_dev, images_dev, n, tables_dev, ntables, total_blocks, max_blocks, status_dev, ws_dev) || !out_dev ||
        max_pixels < 1)
        return set_err(CLIPMI_EINVAL, "jpeg_decode_rgb8: bad arguments");
    hipStream_t st = as_stream(stream);
    unsigned char* planes = nullptr;
    if (int rc = jpeg_baseline_planes("jpeg_decode_rgb8", streams_dev, images_dev, n, tables_dev, ntables, total_blocks, max_blocks,
                                      status_dev, ws_dev, ws_bytes, st, &planes))
        return rc;
    return jpeg_color_tail("jpeg_decode_rgb8", static_cast<const JpegImage*>(images_dev), planes, n, max_pixels, out_dev, st);
}

// Four-component files to Pillow's mode-CMYK rows: the baseline chain over clipmi_jpeg_image4 records, then jpeg_cmyk_kernel
extern "C" int clipmi_jpeg_decode_cmyk8(void* streams_dev, void* images_dev, int n, const void* tables_dev, int ntables,
                                        int64_t total_blocks, int64_t max_blocks, int64_t max_pixels, void* out_dev, int32_t* status_dev,
                                        void* ws_dev, int64_t ws_bytes, void* stream) {
    if (n == 0) return 0;
    if (!jpeg_args_ok(streams_dev, images_dev, n, tables_dev, ntables, total_blocks, max_blocks, status_dev, ws_dev) || !out_dev ||
        max_pixels < 1)
        return set_err(CLIPMI_EINVAL, "jpeg_decode_cmyk8: bad arguments");
    if ((max_pixels + 255) / 256 > 0x7fffffffLL) return set_err(CLIPMI_EINVAL, "jpeg_decode_cmyk8: batch too large for one launch");
    hipStream_t st = as_stream(stream);
    unsigned char* planes = nullptr;
    if (int rc = jpeg_baseline_planes<JpegImage4>("jpeg_decode_cmyk8", streams_dev, images_dev, n, tables_dev, ntables, total_blocks,
                                                  max_blocks, status_dev, ws_dev, ws_bytes, st, &planes))
        return rc;
    hipLaunchKernelGGL(jpeg_cmyk_kernel, dim3((unsigned)((max_pixels + 255) / 256), (unsigned)n), dim3(256), 0, st,
                       static_cast<const JpegImage4*>(images_dev), planes, static_cast<unsigned char*>(out_dev));
    CLIPMI_CHECK_LAUNCH("jpeg_cmyk_kernel");
    return 0;
}

// The transform entries' tail: the fused colour conversion + horizontal pass over the planes, then resize.hip's vertical pass
static int jpeg_transform_tail(const JpegImage* images, const unsigned char* planes, int n, const void* jobs_dev,
                               int max_rows, const int32_t* coef_dev, int n_px, void* out_dev, void* scratch_dev, hipStream_t st) {
    static_assert(sizeof(clipmi_resize_job) == 80, "clipmi_resize_job layout");
    hipLaunchKernelGGL(jpeg_color_resize_h_kernel, dim3((unsigned)((max_rows + JF_ROWS - 1) / JF_ROWS), (unsigned)n), dim3(JF_T), 0, st,
                       images, planes, static_cast<const clipmi_resize_job*>(jobs_dev), coef_dev, n_px,
                       static_cast<unsigned char*>(scratch_dev));
    CLIPMI_CHECK_LAUNCH("jpeg_color_resize_h_kernel");
    return launch_resize_v_rgb8(jobs_dev, n, coef_dev, n_px, scratch_dev, out_dev, st);
}

static bool jpeg_transform_args_ok(const void* jobs_dev, int max_rows, const int32_t* coef_dev, int n_px, void* out_dev, void* scratch_dev) {
    return jobs_dev && coef_dev && out_dev && scratch_dev && n_px >= 1 && n_px <= 4096 && max_rows >= 1;
}

extern "C" int clipmi_jpeg_decode_transform_rgb8(void* streams_dev, void* images_dev, int n, const void* tables_dev, int ntables,
                                                 int64_t total_blocks, int64_t max_blocks, const void* jobs_dev, int max_rows,
                                                 const int32_t* coef_dev, int n_px, void* out_dev, void* scratch_dev, int32_t* status_dev,
                                                 void* ws_dev, int64_t ws_bytes, void* stream) {
    if (n == 0) return 0;
    if (!jpeg_args_ok(streams_dev, images_dev, n, tables_dev, ntables, total_blocks, max_blocks, status_dev, ws_dev) ||
        !jpeg_transform_args_ok(jobs_dev, max_rows, coef_dev, n_px, out_dev, scratch_dev))
        return set_err(CLIPMI_EINVAL, "jpeg_decode_transform_rgb8: bad arguments");
    hipStream_t st = as_stream(stream);
    unsigned char* planes = nullptr;
    if (int rc = jpeg_baseline_planes("jpeg_decode_transform_rgb8", streams_dev, images_dev, n, tables_dev, ntables, total_blocks,
                                      max_blocks, status_dev, ws_dev, ws_bytes, st, &planes))
        return rc;
    return jpeg_transform_tail(static_cast<const JpegImage*>(images_dev), planes, n, jobs_dev, max_rows, coef_dev, n_px, out_dev,
                               scratch_dev, st);
}

extern "C" int64_t clipmi_jpeg_progressive_workspace_bytes(int n, int64_t total_blocks, int ntables) {
    if (n < 0 || total_blocks < 0 || ntables < 0) return -1;
    return (int64_t)align_up((size_t)ntables * sizeof(JppLut), 256) + (int64_t)align_up((size_t)n * sizeof(JpegImage), 256) +
           (int64_t)align_up((size_t)total_blocks * 128, 256) + (int64_t)align_up((size_t)total_blocks * 64, 256);
}

// The progressive decode up to the sample planes -> 0, the planes and the records jpeg_progressive_kernel wrote for the later kernels
static int jpeg_progressive_planes(const char* who, const void* streams_dev, const void* images_dev, int n, const void* scans_dev,
                                   int nscans, const void* tables_dev, int ntables, int64_t total_blocks, int64_t max_blocks,
                                   int32_t* status_dev, void* ws_dev, int64_t ws_bytes, hipStream_t st, unsigned char** planes_out,
                                   JpegImage** images_out) {
    static_assert(sizeof(JpegScan) == sizeof(clipmi_jpeg_scan) && sizeof(JpegScan) == 64, "clipmi_jpeg_scan layout");
    static_assert(sizeof(JpegProgImage) == sizeof(clipmi_jpeg_progressive_image) && sizeof(JpegProgImage) == 256,
                  "clipmi_jpeg_progressive_image layout");
    if (ws_bytes < clipmi_jpeg_progressive_workspace_bytes(n, total_blocks, ntables))
        return set_err(CLIPMI_EINVAL, "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes,
                       (long long)clipmi_jpeg_progressive_workspace_bytes(n, total_blocks, ntables));
    if ((max_blocks + 127) / 128 > 0x7fffffffLL || n > 65535) return set_err(CLIPMI_EINVAL, "%s: batch too large for one launch", who);
    Arena ar(ws_dev, (size_t)ws_bytes);
    JppLut* luts = ar.take<JppLut>((size_t)ntables);
    JpegImage* images = ar.take<JpegImage>((size_t)n);
    short* coef = ar.take<short>((size_t)total_blocks * 64);
    unsigned char* planes = ar.take<unsigned char>((size_t)total_blocks * 64);
    if (zero_async(coef, (size_t)total_blocks * 128, st) != hipSuccess) return set_err(CLIPMI_EHIP, "%s: zero_async", who);
    hipLaunchKernelGGL(jpeg_build_pluts_kernel, dim3((unsigned)ntables), dim3(256), 0, st, static_cast<const unsigned char*>(tables_dev), luts);
    CLIPMI_CHECK_LAUNCH("jpeg_build_pluts_kernel");
    hipLaunchKernelGGL(jpeg_progressive_kernel, dim3((unsigned)n), dim3(JPP_T), 0, st, static_cast<const unsigned char*>(streams_dev),
                       static_cast<const JpegProgImage*>(images_dev), static_cast<const JpegScan*>(scans_dev), nscans, luts, ntables,
                       images, coef, status_dev);
    CLIPMI_CHECK_LAUNCH("jpeg_progressive_kernel");
    hipLaunchKernelGGL(jpeg_idct_kernel<JpegImage>, dim3((unsigned)((max_blocks + 127) / 128), (unsigned)n), dim3(128), 0, st,
                       static_cast<const JpegImage*>(images), static_cast<const short*>(coef), planes, status_dev);
    CLIPMI_CHECK_LAUNCH("jpeg_idct_kernel");
    *planes_out = planes;
    *images_out = images;
    return 0;
}

extern "C" int clipmi_jpeg_decode_progressive_rgb8(const void* streams_dev, const void* images_dev, int n, const void* scans_dev, int nscans,
                                                   const void* tables_dev, int ntables, int64_t total_blocks, int64_t max_blocks,
                                                   int64_t max_pixels, void* out_dev, int32_t* status_dev, void* ws_dev, int64_t ws_bytes,
                                                   void* stream) {
    if (n == 0) return 0;
    if (!jpeg_args_ok(streams_dev, images_dev, n, tables_dev, ntables, total_blocks, max_blocks, status_dev, ws_dev) || !scans_dev ||
        nscans < 1 || !out_dev || max_pixels < 1)
        return set_err(CLIPMI_EINVAL, "jpeg_decode_progressive_rgb8: bad arguments");
    hipStream_t st = as_stream(stream);
    unsigned char* planes = nullptr;
    JpegImage* images = nullptr;
    if (int rc = jpeg_progressive_planes("jpeg_decode_progressive_rgb8", streams_dev, images_dev, n, scans_dev, nscans, tables_dev, ntables,
                                         total_blocks, max_blocks, status_dev, ws_dev, ws_bytes, st, &planes, &images))
        return rc;
    return jpeg_color_tail("jpeg_decode_progressive_rgb8", images, planes, n, max_pixels, out_dev, st);
}

extern "C" int clipmi_jpeg_decode_progressive_transform_rgb8(const void* streams_dev, const void* images_dev, int n, const void* scans_dev,
                                                             int nscans, const void* tables_dev, int ntables, int64_t total_blocks,
                                                             int64_t max_blocks, const void* jobs_dev, int max_rows,
                                                             const int32_t* coef_dev, int n_px, void* out_dev, void* scratch_dev,
                                                             int32_t* status_dev, void* ws_dev, int64_t ws_bytes, void* stream) {
    if (n == 0) return 0;
    if (!jpeg_args_ok(streams_dev, images_dev, n, tables_dev, ntables, total_blocks, max_blocks, status_dev, ws_dev) || !scans_dev ||
        nscans < 1 || !jpeg_transform_args_ok(jobs_dev, max_rows, coef_dev, n_px, out_dev, scratch_dev))
        return set_err(CLIPMI_EINVAL, "jpeg_decode_progressive_transform_rgb8: bad arguments");
    hipStream_t st = as_stream(stream);
    unsigned char* planes = nullptr;
    JpegImage* images = nullptr;
    if (int rc = jpeg_progressive_planes("jpeg_decode_progressive_transform_rgb8", streams_dev, images_dev, n, scans_dev, nscans, tables_dev,
                                         ntables, total_blocks, max_blocks, status_dev, ws_dev, ws_bytes, st, &planes, &images))
        return rc;
    return jpeg_transform_tail(images, planes, n, jobs_dev, max_rows, coef_dev, n_px, out_dev, scratch_dev, st);
}
