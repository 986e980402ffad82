// png.hip — `Image.open(f).convert("RGB")` for PNG files on the device (include/clipmi.h clipmi_png_decode_rgb8:
// 8-bit grey and RGB files), and the file's own-mode pixels for alpha, palette and low-depth files and for files of depth 16 - RGB,
// RGBA, grey + alpha, of which every sample's high byte is kept as Pillow does (clipmi_png_decode_px8). The host
// (cli-p_amd/png_parse.py) walks the chunks and hands over the DEFLATE stream behind the zlib header. Both entries run the same
// three kernels:
//   png_inflate_kernel          one wave per image: RFC 1951 inflate into the workspace's scanline buffer, with zlib's own table checks
//   png_unfilter_kernel<modes>  one wave per image: PNG reconstruction (None, Sub, Up, Average, Paeth) as a 64-row diagonal
//                               wavefront, decoded pixels out; <0> for clipmi_png_decode_rgb8, <1> for clipmi_png_decode_px8
//   png_adler_kernel            one block per image: Adler-32 of the scanlines against the stream's trailer
// What a record's file is - filter unit, bits per pixel, layout of the decoded pixels, Adam7 or not - is read in one place
// (png_format -> PngFormat), and every kernel starts from it. An Adam7 file's stream holds up to seven reduced images one after the
// other, each filtered on its own: inflate and Adler-32 only see a byte string of another length (png_scanline_bytes), and the
// unfilter kernel reconstructs the passes in file order (png_unfilter_passes, the one walk over a record's passes) and scatters
// their pixels (PngPass, png_pixel). What becomes of the reconstructed bytes is one of two stores': PngSampleStore for pixels of
// whole-byte samples, PngPackedStore for palette indices and samples below a byte.
// PNG is lossless, so a file either comes back with exactly Pillow's bytes (status 0) or goes back to Pillow. Status 0 is given
// only where zlib certainly accepts: valid data that ends with the final block's end-of-block code after exactly
// height x (1 + width x channels) bytes (Adam7: the sum of that over the non-empty passes), filter bytes <= 4, and a present,
// matching Adler-32. That covers the image data only:
// that Pillow does not refuse the file for a chunk in front of or behind it is the host parser's part (png_parse.py).
// These kernels read untrusted bytes: every stream read is bounded by stream_bytes + the 16 pad bytes, every scanline write by
// the image's own byte count, every table index by the table's size; a malformed file ends in a status.
#include "common.hpp"

namespace clipmi {
namespace {

struct PngImage {               // mirrors clipmi_png_image
    int64_t stream_off, raw_off, out_off;
    int32_t stream_bytes, width, height, channels;
    int32_t reserved[2];
};

constexpr int PNG_T = 64;                   // one wave
constexpr unsigned PNG_RING = 32768;        // the DEFLATE window, an LDS ring; also what is waiting to be flushed
constexpr unsigned PNG_RMASK = PNG_RING - 1;
constexpr unsigned PNG_FLUSH = 8192;        // flush to HBM from this many waiting bytes on (waiting + one match stays < the ring)
constexpr int PNG_LIT_BITS = 10, PNG_DIST_BITS = 9, PNG_CL_BITS = 7;
constexpr int PNG_PAD = 16;                 // zero bytes behind every stream
constexpr int PNG_MAX_WIDTH = 16384;        // the unfilter kernel holds one row in LDS (48 KiB); png_parse.MAX_WIDTH
constexpr int PNG_MAX_ROW = 49152;          // ... that many bytes: what bounds the rows of clipmi_png_decode_px8; png_parse.MAX_ROW_BYTES

// What a record's file is. A pixel has `samples` samples of `sample_bytes` bytes each, or is packed: a palette index of any depth
// or a grey sample below a byte, several to a byte, which PNG filters byte by byte (unit 1). layout: what the entry leaves of a
// pixel - RGB3: 3 bytes R G B (grey as L L L); ALPHA4: 4 bytes R G B A (grey + alpha as L L L A, packed grey as L L L 255);
// INDEX1: 1 byte, the palette index (1-bit grey: 0 or 1, black and white).
enum { PNG_RGB3 = 0, PNG_ALPHA4 = 1, PNG_INDEX1 = 2 };
struct PngFormat {
    int unit;                   // the filter's unit in bytes: 1, 2, 3, 4, 6 or 8
    int bpp;                    // bits per pixel
    int samples, sample_bytes;
    bool packed;
    int layout;
    int depth, entries;         // bit depth; a packed sample has to stay below `entries` (status 5)
    bool interlaced;            // Adam7
};

// The only reader of a record's `channels` and `reserved`. -> whether the record is one its entry takes.
// modes == 0 (clipmi_png_decode_rgb8): 8-bit grey or RGB by `channels`. The entry never looked at `reserved`, so only the one value
// 1 << 16 of reserved[0] means Adam7 there and every other value means what it meant before: nothing.
// modes == 1 (clipmi_png_decode_px8): reserved[0] = Adam7 << 16 | colour type << 8 | bit depth, reserved[1] = palette entries;
// RGBA and grey + alpha at 8 bits, palette at 1/2/4/8, grey at 1/2/4; and at 16 bits RGB, RGBA and grey + alpha, whose rows of 6, 8
// and 4 bytes a pixel are bounded by PNG_MAX_ROW like the others: 8192, 6144 and 12288 pixels.
__device__ __forceinline__ bool png_format(const PngImage& im, int modes, PngFormat& f) {
    if (im.width < 1 || im.width > PNG_MAX_WIDTH) return false;
    const int word = im.reserved[0];
    int ctype;
    f.sample_bytes = 1;
    f.packed = false;
    f.entries = 2;
    if (!modes) {
        if (im.channels != 1 && im.channels != 3) return false;
        ctype = im.channels == 3 ? 2 : 0;
        f.depth = 8;
        f.samples = im.channels;
        f.interlaced = word == (1 << 16);
    } else {
        if (word >> 17) return false;
        ctype = (word >> 8) & 255;
        f.depth = word & 255;
        f.interlaced = ((word >> 16) & 1) != 0;
        const bool low = f.depth == 1 || f.depth == 2 || f.depth == 4;
        if (ctype == 6 && f.depth == 8) f.samples = 4;
        else if (ctype == 4 && f.depth == 8) f.samples = 2;
        else if (ctype == 3 && (low || f.depth == 8) && im.reserved[1] >= 1 && im.reserved[1] <= (1 << f.depth)) {
            f.samples = 1;
            f.packed = true;
            f.entries = im.reserved[1];
        } else if (ctype == 0 && low) {
            f.samples = 1;
            f.packed = true;
        } else if (f.depth == 16 && (ctype == 2 || ctype == 6 || ctype == 4)) {
            f.samples = ctype == 2 ? 3 : ctype == 6 ? 4 : 2;
            f.sample_bytes = 2;
        } else return false;
        if (im.channels != f.samples) return false;
    }
    f.bpp = f.samples * f.depth;
    f.unit = f.samples * f.sample_bytes;
    if (f.packed) f.layout = ctype == 3 || f.depth == 1 ? PNG_INDEX1 : PNG_ALPHA4;
    else f.layout = f.samples == 1 || f.samples == 3 ? PNG_RGB3 : PNG_ALPHA4;
    return !modes || (((int64_t)im.width * f.bpp + 7) >> 3) <= PNG_MAX_ROW;
}

// Adam7: pass p holds the pixels (x0 + i dx, y0 + j dy) of the image, i < w, j < h, as an image of w x h pixels of its own. The
// seven passes partition the image; w or h is 0 where the image has no pixel of the pass, and such a pass has no bytes at all.
struct PngPass {
    int x0, y0, dx, dy, w, h;
};

// (x0, y0, dx, dy) of pass p = 0 .. 6, one nibble each: (0,0,8,8) (4,0,8,8) (0,4,4,8) (2,0,4,4) (0,2,2,4) (1,0,2,2) (0,1,1,2);
// png_parse.ADAM7. width, height >= 1.
__device__ __forceinline__ PngPass png_pass(int width, int height, int p) {
    const int s = 4 * p;
    PngPass ps;
    ps.x0 = (0x0102040 >> s) & 15;
    ps.y0 = (0x1020400 >> s) & 15;
    ps.dx = (0x1224488 >> s) & 15;
    ps.dy = (0x2244888 >> s) & 15;
    ps.w = width > ps.x0 ? (width - ps.x0 - 1) / ps.dx + 1 : 0;
    ps.h = height > ps.y0 ? (height - ps.y0 - 1) / ps.dy + 1 : 0;
    return ps;
}

// The one pass of a file that is not interlaced: the image
__device__ __forceinline__ PngPass png_whole(int width, int height) { return PngPass{0, 0, 1, 1, width, height}; }

// Bytes of filtered scanlines of the record, interlace included: what the stream has to inflate to, what the Adler-32 covers and
// what the unfilter kernel walks. A row of w pixels - the image's, or a pass's - has 1 + ceil(w x bpp / 8) bytes.
__device__ __forceinline__ int64_t png_scanline_bytes(const PngImage& im, const PngFormat& f) {
    if (im.height < 1) return 0;
    if (!f.interlaced) return (int64_t)im.height * (1 + (((int64_t)im.width * f.bpp + 7) >> 3));
    int64_t n = 0;
    for (int p = 0; p < 7; p++) {
        const PngPass ps = png_pass(im.width, im.height, p);
        if (ps.w && ps.h) n += (int64_t)ps.h * (1 + (((int64_t)ps.w * f.bpp + 7) >> 3));
    }
    return n;
}

// The image pixel (counted row by row) of pixel x of row `row` of a pass
template <bool LACE>
__device__ __forceinline__ int64_t png_pixel(const PngPass& ps, int width, int row, int x) {
    if (!LACE) return (int64_t)row * width + x;
    return ((int64_t)ps.y0 + (int64_t)row * ps.dy) * width + ps.x0 + x * ps.dx;
}

__constant__ unsigned char png_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// One canonical Huffman code in LDS: the number of codes per length, the symbols sorted by (length, symbol), and a direct
// look-up of `bits` bits: entry = symbol << 4 | length, 0 where those bits do not hold a whole code.
struct PngCode {
    int* count;                 // [16]
    unsigned short* sorted;     // [nsym]
    unsigned short* lut;        // [1 << bits]
    int nsym, bits;
};

// The canonical first-code walk: the code whose bits (first bit of the code in bit 0 of `v`) start `v`, at most `maxlen` bits
// long. -> symbol, length in `len`; -1 where no code of that length matches (an unused code of an incomplete set).
__device__ __forceinline__ int png_walk(const PngCode& c, unsigned v, int maxlen, int& len) {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= maxlen; l++) {
        code |= (int)(v & 1u);
        v >>= 1;
        const int cnt = c.count[l];
        if (code - cnt < first) {
            const int at = index + (code - first);
            if (at < 0 || at >= c.nsym) return -1;
            len = l;
            return c.sorted[at];
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -1;
}

enum { PNG_KIND_CL = 0, PNG_KIND_LIT = 1, PNG_KIND_DIST = 2 };

// Build `c` from lens[0 .. c.nsym) (each <= 15), the whole wave together. zlib's checks (inftrees.c): an over-subscribed set is
// refused; an incomplete one too, except a literal/length or distance code that consists of a single one-bit code; a distance
// code may be empty. -> false where zlib refuses. Wave-uniform.
__device__ bool png_build(const PngCode& c, const unsigned char* lens, int kind, int lane) {
    if (lane < 16) c.count[lane] = 0;
    __syncthreads();
    for (int s = lane; s < c.nsym; s += PNG_T) atomicAdd(&c.count[lens[s] & 15], 1);
    __syncthreads();
    int left = 1, maxl = 0;
    bool over = false;
    for (int l = 1; l <= 15; l++) {
        const int cnt = c.count[l];
        left = left * 2 - cnt;
        if (left < 0) { over = true; break; }
        if (cnt) maxl = l;
    }
    if (over) return false;
    if (maxl == 0) {
        if (kind != PNG_KIND_DIST) return false;      // (zlib lets an empty code-length code through and then misses code 256)
    } else if (left > 0 && (kind == PNG_KIND_CL || maxl != 1)) {
        return false;
    }
    // lane l collects the symbols of length l, in symbol order
    if (lane >= 1 && lane <= 15) {
        int at = 0;
        for (int l = 1; l < lane; l++) at += c.count[l];
        const int end = at + c.count[lane];
        for (int s = 0; s < c.nsym && at < end; s++)
            if (lens[s] == lane) c.sorted[at++] = (unsigned short)s;
    }
    __syncthreads();
    for (int i = lane; i < (1 << c.bits); i += PNG_T) {
        int len = 0;
        const int s = png_walk(c, (unsigned)i, c.bits, len);
        c.lut[i] = s >= 0 ? (unsigned short)(s << 4 | len) : (unsigned short)0;
    }
    __syncthreads();
    return true;
}

// LSB-first bit reader over one stream. Reads stay inside [0, limit) with limit = stream_bytes + PNG_PAD (zero bytes beyond);
// over() tells that more bits were taken than the stream has.
struct PngBits {
    const unsigned char* p;
    unsigned limit, pos;        // pos: the next byte to load
    unsigned long long buf, total_bits;
    int cnt;
    __device__ __forceinline__ void refill() {       // at least 33 bits afterwards
        if (cnt <= 32) {
            unsigned w = 0;
            if (pos + 4u <= limit) __builtin_memcpy(&w, p + pos, 4);
            buf |= (unsigned long long)w << cnt;
            cnt += 32;
            pos += 4;
        }
    }
    __device__ __forceinline__ unsigned peek(int n) const { return (unsigned)buf & ((1u << n) - 1u); }
    __device__ __forceinline__ void drop(int n) { buf >>= n; cnt -= n; }
    __device__ __forceinline__ unsigned take(int n) { const unsigned v = peek(n); drop(n); return v; }
    __device__ __forceinline__ unsigned long long used() const { return (unsigned long long)pos * 8ull - (unsigned long long)cnt; }
    __device__ __forceinline__ bool over() const { return used() > total_bits; }
    __device__ __forceinline__ unsigned byte_pos() { drop(cnt & 7); return pos - (unsigned)(cnt >> 3); }   // skips to the byte boundary
    __device__ __forceinline__ void seek(unsigned byte) { pos = byte; buf = 0; cnt = 0; }
};

// Everything below is wave-uniform: all 64 lanes walk the symbols with the same values (stream loads are broadcasts), so the
// barriers sit in uniform control flow; only the copies into the ring and out of it are spread over the lanes.
__global__ void __launch_bounds__(PNG_T) png_inflate_kernel(const unsigned char* __restrict__ streams, const PngImage* __restrict__ images,
                                                            int64_t total_raw, int64_t max_raw, unsigned char* __restrict__ rawbuf,
                                                            unsigned* __restrict__ adler_want, int32_t* __restrict__ status, int modes) {
    __shared__ __attribute__((aligned(16))) unsigned char ring[PNG_RING];
    __shared__ unsigned short lit_lut[1 << PNG_LIT_BITS], dist_lut[1 << PNG_DIST_BITS], cl_lut[1 << PNG_CL_BITS];
    __shared__ unsigned short lit_sorted[288], dist_sorted[32], cl_sorted[19];
    __shared__ int lit_count[16], dist_count[16], cl_count[16];
    __shared__ unsigned char lens[320], cl_lens[19];
    const int lane = threadIdx.x;
    const PngImage im = images[blockIdx.x];
    PngFormat fmt;
    const bool known = png_format(im, modes, fmt);
    const int64_t raw_bytes64 = known ? png_scanline_bytes(im, fmt) : 0;
    if (!known || im.height < 1 || im.stream_bytes < 0 || im.stream_off < 0 ||
        raw_bytes64 > 0x7fffffffLL || raw_bytes64 > max_raw || im.raw_off < 0 || (im.raw_off & 15) ||
        im.raw_off + raw_bytes64 > total_raw) {
        if (lane == 0) status[blockIdx.x] = 1;
        return;
    }
    const unsigned raw_bytes = (unsigned)raw_bytes64;
    unsigned char* dst = rawbuf + im.raw_off;
    PngBits br;
    br.p = streams + im.stream_off;
    br.limit = (unsigned)im.stream_bytes + PNG_PAD;
    br.total_bits = (unsigned long long)im.stream_bytes * 8ull;
    br.seek(0);
    const unsigned stream_bytes = (unsigned)im.stream_bytes;

    PngCode lit{lit_count, lit_sorted, lit_lut, 288, PNG_LIT_BITS};
    PngCode dist{dist_count, dist_sorted, dist_lut, 32, PNG_DIST_BITS};
    const PngCode cl{cl_count, cl_sorted, cl_lut, 19, PNG_CL_BITS};

    unsigned outpos = 0, flushed = 0;   // bytes produced; bytes of them already in HBM (a multiple of 16 until the end)
    int st = 0;
    bool last = false, fixed_built = false;

    // ring[flushed .. outpos) -> HBM, 16 bytes a lane; all but the last call leave the odd bytes for the next one
    auto flush = [&](bool final) {
        __syncthreads();
        unsigned nb = outpos - flushed;
        if (!final) nb &= ~15u;
        for (unsigned o = (unsigned)lane * 16u; o + 16u <= nb; o += PNG_T * 16u)
            *reinterpret_cast<uint4*>(dst + flushed + o) = *reinterpret_cast<const uint4*>(&ring[(flushed + o) & PNG_RMASK]);
        const unsigned tail = nb & 15u;
        if ((unsigned)lane < tail) dst[flushed + (nb - tail) + lane] = ring[(flushed + (nb - tail) + lane) & PNG_RMASK];
        flushed += nb;
        __syncthreads();
    };

    while (!last && st == 0) {          // one block per turn: at least its 3 header bits are consumed
        br.refill();
        if (br.over()) { st = 2; break; }
        last = br.take(1) != 0;
        const unsigned type = br.take(2);
        if (type == 3) { st = 1; break; }
        if (type == 0) {                // stored: LEN, ~LEN behind the byte boundary, then LEN bytes
            unsigned at = br.byte_pos();
            if (at + 4u > stream_bytes) { st = 2; break; }
            const unsigned len = br.p[at] | (unsigned)br.p[at + 1] << 8, nlen = br.p[at + 2] | (unsigned)br.p[at + 3] << 8;
            if ((len ^ 0xffffu) != nlen) { st = 1; break; }
            at += 4;
            if (at + len > stream_bytes || len > raw_bytes - outpos) { st = 2; break; }
            const unsigned start = outpos;
            for (unsigned o = 0; o < len; o += PNG_T) {
                const unsigned i = o + lane;
                if (i < len) ring[(start + i) & PNG_RMASK] = br.p[at + i];
                outpos = start + min(o + (unsigned)PNG_T, len);
                if (outpos - flushed >= PNG_FLUSH) flush(false);
            }
            __syncthreads();
            br.seek(at + len);
            continue;
        }
        if (type == 1) {
            if (!fixed_built) {
                for (int s = lane; s < 320; s += PNG_T) lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
                __syncthreads();
                lit.nsym = 288;
                dist.nsym = 32;
                png_build(lit, lens, PNG_KIND_LIT, lane);           // complete codes, by construction
                png_build(dist, lens + 288, PNG_KIND_DIST, lane);
                fixed_built = true;
            }
        } else {
            fixed_built = false;
            const int nlen = (int)br.take(5) + 257, ndist = (int)br.take(5) + 1, ncode = (int)br.take(4) + 4;
            if (nlen > 286 || ndist > 30) { st = 1; break; }
            if (lane < 19) cl_lens[lane] = 0;
            __syncthreads();
            for (int i = 0; i < ncode; i++) {
                br.refill();
                const unsigned v = br.take(3);
                if (lane == 0) cl_lens[png_cl_order[i]] = (unsigned char)v;
            }
            __syncthreads();
            if (!png_build(cl, cl_lens, PNG_KIND_CL, lane)) { st = 1; break; }
            int have = 0, prev = 0;
            while (have < nlen + ndist) {                           // every turn consumes at least one bit
                br.refill();
                if (br.over()) { st = 2; break; }
                const unsigned e = cl_lut[br.peek(PNG_CL_BITS)];
                if ((e & 15u) == 0) { st = 1; break; }              // a code-length code has at most 7 bits: the look-up is complete
                br.drop((int)(e & 15u));
                const int s = (int)(e >> 4);
                int rep = 1, val = s;
                if (s == 16) {
                    if (have == 0) { st = 1; break; }
                    val = prev;
                    rep = 3 + (int)br.take(2);
                } else if (s == 17) {
                    val = 0;
                    rep = 3 + (int)br.take(3);
                } else if (s == 18) {
                    val = 0;
                    rep = 11 + (int)br.take(7);
                }
                if (have + rep > nlen + ndist) { st = 1; break; }   // (a repeat from the literal lengths into the distance lengths is legal)
                for (int i = lane; i < rep; i += PNG_T) lens[have + i] = (unsigned char)val;
                have += rep;
                prev = val;
            }
            if (st) break;
            __syncthreads();
            if (lens[256] == 0) { st = 1; break; }
            lit.nsym = nlen;
            dist.nsym = ndist;
            if (!png_build(lit, lens, PNG_KIND_LIT, lane) || !png_build(dist, lens + nlen, PNG_KIND_DIST, lane)) { st = 1; break; }
        }
        // the symbols of a Huffman block: every turn consumes at least one bit
        for (;;) {
            br.refill();
            if (br.over()) { st = 2; break; }
            unsigned e = lit_lut[br.peek(PNG_LIT_BITS)];
            int l = (int)(e & 15u), sym = (int)(e >> 4);
            if (l == 0) {
                sym = png_walk(lit, br.peek(15), 15, l);
                if (sym < 0) { st = 1; break; }
            }
            br.drop(l);
            if (sym < 256) {
                if (outpos >= raw_bytes) { st = 2; break; }
                if (lane == 0) ring[outpos & PNG_RMASK] = (unsigned char)sym;
                outpos++;
            } else if (sym == 256) {
                break;
            } else {
                if (sym >= 286) { st = 1; break; }
                unsigned len;
                if (sym < 265) len = (unsigned)sym - 254u;
                else if (sym == 285) len = 258u;
                else {
                    const int eb = (sym - 261) >> 2;
                    len = 3u + ((4u + (unsigned)((sym - 261) & 3)) << eb) + br.take(eb);
                }
                br.refill();
                e = dist_lut[br.peek(PNG_DIST_BITS)];
                l = (int)(e & 15u);
                int ds = (int)(e >> 4);
                if (l == 0) {
                    ds = png_walk(dist, br.peek(15), 15, l);
                    if (ds < 0) { st = 1; break; }
                }
                br.drop(l);
                if (ds >= 30) { st = 1; break; }
                unsigned d;
                if (ds < 4) d = (unsigned)ds + 1u;
                else {
                    const int eb = (ds >> 1) - 1;
                    d = 1u + ((2u + (unsigned)(ds & 1)) << eb) + br.take(eb);
                }
                if (d > outpos) { st = 1; break; }                  // beyond the bytes produced so far (d <= 32768 by the code)
                if (len > raw_bytes - outpos) { st = 2; break; }
                // byte i of the match is window[outpos - d + i % d]: all of them lie before the match, so the 64 lanes copy
                // independent bytes; a piece's reads come before its writes (one wave, in order), which matters where the
                // ring slot of a read byte is the slot of a written one (d close to the ring's size)
                __syncthreads();
                const unsigned from = outpos - d;
                for (unsigned o = 0; o < len; o += PNG_T) {
                    const unsigned i = o + lane;
                    unsigned char v = 0;
                    if (i < len) v = ring[(from + (d >= len ? i : i % d)) & PNG_RMASK];
                    __syncthreads();
                    if (i < len) ring[(outpos + i) & PNG_RMASK] = v;
                }
                __syncthreads();
                outpos += len;
            }
            if (outpos - flushed >= PNG_FLUSH) flush(false);
        }
    }
    if (st == 0 && br.over()) st = 2;
    if (st == 0 && outpos != raw_bytes) st = 2;
    if (st == 0) {
        flush(true);
        const unsigned at = br.byte_pos();
        if (at + 4u > stream_bytes) st = 2;
        else if (lane == 0)
            adler_want[blockIdx.x] = (unsigned)br.p[at] << 24 | (unsigned)br.p[at + 1] << 16 | (unsigned)br.p[at + 2] << 8 | br.p[at + 3];
    }
    if (lane == 0) status[blockIdx.x] = st;
}

// ---- reconstruction. Lane j owns row r0 + j of a 64-row band and runs one step of 4 pixels behind lane j - 1: the pixels above
// (b) are the ones lane j - 1 finished in the step before and arrive by a cross-lane move; left (a) and upper left (c) stay in
// registers. The first row of a band needs the last row of the band before: lane 63 leaves its finished words in an LDS row
// (`prev`, PNG_MAX_ROW bytes: png_format refuses longer rows) and lane 0 of the next band takes them from there, so
// the kernel never reads back what it stored to HBM. Within a band lane 63 writes word index t - 63 while lane 0 reads index
// t: every word is read before it is overwritten, and the barrier between two bands orders the rest.
// The filter works on units of CH bytes (PngFormat.unit): a pixel's bytes, or 1 for packed rows. At depth 16 that reconstructs
// both bytes of every sample - Sub, Average and Paeth of the high bytes' neighbours do not depend on the low bytes, but a row is
// only complete with them and the Adler-32 covers them. `w` counts units. What becomes of a step's finished bytes is the store's
// business: store.put(row, x0, words) gets the units x0 .. x0 + 3 of the row (those below w are valid), packed as they lie in
// the file.
template <int CH, class Store>
__device__ void png_unfilter_image(const unsigned char* __restrict__ raw, Store& store, unsigned* prev, int w, int h, int lane, bool& bad) {
    constexpr int PX = 4, NW = CH;                      // 4 units a step: CH words of 4 bytes
    const int64_t stride = 1 + (int64_t)w * CH;
    const int steps = (w + PX - 1) / PX;
    for (int r0 = 0; r0 < h; r0 += PNG_T) {
        const int row = r0 + lane;
        const bool active = row < h;
        int ft = active ? raw[row * stride] : 0;
        if (ft > 4) { bad = true; ft = 0; }
        const unsigned char* src = raw + row * stride + 1;
        unsigned res[NW];
        int a[CH], c[CH];
#pragma unroll
        for (int k = 0; k < NW; k++) res[k] = 0;
#pragma unroll
        for (int k = 0; k < CH; k++) a[k] = c[k] = 0;
        for (int t = 0; t < steps + PNG_T - 1; t++) {
            unsigned bw[NW];
#pragma unroll
            for (int k = 0; k < NW; k++) bw[k] = __shfl_up(res[k], 1);
            const int m = t - lane;
            const bool on = active && m >= 0 && m < steps;
            const int x0 = m * PX;
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < NW; k++) bw[k] = (on && r0 > 0) ? prev[m * NW + k] : 0u;
            }
            if (on) {
                unsigned f[NW];
#pragma unroll
                for (int k = 0; k < NW; k++) f[k] = 0;
#pragma unroll
                for (int q = 0; q < PX * CH; q++)
                    if (x0 + q / CH < w) f[q >> 2] |= (unsigned)src[(int64_t)x0 * CH + q] << (8 * (q & 3));
#pragma unroll
                for (int k = 0; k < NW; k++) res[k] = 0;
#pragma unroll
                for (int q = 0; q < PX * CH; q++) {
                    const int k = q % CH;
                    const int b = (int)(bw[q >> 2] >> (8 * (q & 3))) & 255;
                    const int fv = (int)(f[q >> 2] >> (8 * (q & 3))) & 255;
                    const int pa = abs(b - c[k]), pb = abs(a[k] - c[k]), pc = abs(a[k] + b - 2 * c[k]);
                    const int paeth = (pa <= pb && pa <= pc) ? a[k] : (pb <= pc ? b : c[k]);
                    const int pred = ft == 0 ? 0 : ft == 1 ? a[k] : ft == 2 ? b : ft == 3 ? (a[k] + b) >> 1 : paeth;
                    const int v = (fv + pred) & 255;
                    c[k] = b;
                    a[k] = v;
                    res[q >> 2] |= (unsigned)v << (8 * (q & 3));
                }
                store.put(row, x0, res);
                if (lane == PNG_T - 1) {
#pragma unroll
                    for (int k = 0; k < NW; k++) prev[m * NW + k] = res[k];
                }
            }
        }
        __syncthreads();
    }
}

// The stores get the rows of one pass (`ps`: the image itself where the file is not interlaced, LACE false) and put each pixel
// where png_pixel says it belongs in the image of `width` columns: x < ps.w and row < ps.h keep every store inside the image's
// width x height pixels. UNIT: the filter unit png_unfilter_image runs the store with.
//
// Pixels of S samples of B bytes (B == 2: depth 16, a sample's high byte comes first and is the one Pillow keeps; the low bytes
// were only needed to reconstruct the row and for the Adler-32). S == 3 and S == 1 leave rows of width * 3 bytes, R G B and L L L
// (PNG_RGB3); S == 4 and S == 2 rows of width words, R G B A and L L L A (PNG_ALPHA4; out_off is a multiple of 16).
template <int S, int B, bool LACE>
struct PngSampleStore {
    static constexpr int UNIT = S * B;
    static constexpr bool over = false;                 // no palette, so never status 5
    unsigned char* out;
    int width;
    PngPass ps;
    static __device__ __forceinline__ unsigned first(const unsigned* res, int p, int s) {    // the first byte of sample s of unit p
        const int i = p * UNIT + s * B;
        return (res[i >> 2] >> (8 * (i & 3))) & 255u;
    }
    __device__ __forceinline__ void put(int row, int x0, const unsigned* res) {
#pragma unroll
        for (int p = 0; p < 4; p++) {
            if (x0 + p >= ps.w) break;
            const int64_t at = png_pixel<LACE>(ps, width, row, x0 + p);
            if (S == 3 || S == 1) {
                unsigned char* d = out + at * 3;
#pragma unroll
                for (int k = 0; k < 3; k++) d[k] = (unsigned char)first(res, p, S == 3 ? k : 0);
            } else if (S == 4) {
                reinterpret_cast<unsigned*>(out)[at] = first(res, p, 0) | first(res, p, 1) << 8 | first(res, p, 2) << 16 | first(res, p, 3) << 24;
            } else {
                reinterpret_cast<unsigned*>(out)[at] = first(res, p, 0) * 0x010101u | first(res, p, 1) << 24;
            }
        }
    }
};

// Palette indices at depth 1/2/4/8 and grey samples at depth 1/2/4: a step's 4 bytes hold 8 / depth samples each, the most
// significant bits of a byte first; a pass row is packed on its own, ceil(ps.w x depth / 8) bytes, and the padding bits at its
// end are dropped at ps.w. PNG_INDEX1: rows of width bytes, one unpacked sample each, and a sample >= `entries` sets over (status
// 5). PNG_ALPHA4: grey at depth 2 / 4 as v*85 / v*17 three times and 255 (Pillow opens those files as L with these values).
template <bool LACE>
struct PngPackedStore {
    static constexpr int UNIT = 1;
    unsigned char* out;
    int width, layout, depth, entries;
    PngPass ps;
    bool over;
    __device__ __forceinline__ void put(int row, int x0, const unsigned* res) {
        const int per = 8 / depth;                                  // samples in a byte: 1, 2, 4 or 8
        const unsigned mask = (1u << depth) - 1u;
        for (int q = 0; q < 4; q++) {
            const unsigned byte = (res[0] >> (8 * q)) & 255u;
            const int64_t px0 = ((int64_t)x0 + q) * per;
            for (int s = 0; s < per; s++) {
                const int64_t px = px0 + s;
                if (px >= ps.w) return;
                const unsigned v = (byte >> (8 - depth * (s + 1))) & mask;
                const int64_t at = png_pixel<LACE>(ps, width, row, (int)px);
                if (layout == PNG_ALPHA4) {
                    reinterpret_cast<unsigned*>(out)[at] = v * (depth == 2 ? 85u : 17u) * 0x010101u | 0xff000000u;
                } else {
                    if ((int)v >= entries) over = true;
                    out[at] = (unsigned char)v;
                }
            }
        }
    }
};

// The record's passes in file order (one, the image, where LACE is false): each non-empty pass is an image of its own - its
// first row has a zero row above it (png_unfilter_image reads `prev` from the second band on only), its filter bytes are
// checked, and its bytes start where the previous pass's end. png_unfilter_image ends every band with a barrier, so the LDS row
// is free when the next pass begins. The early passes are short of rows for the 64-row wavefront (pass 1 has height / 8).
// A row of unit-1 pixels is ceil(ps.w x bpp / 8) units long (several packed pixels to a byte, or one), every other row ps.w
// units: at most PNG_MAX_ROW bytes (png_format), so ceil(units / 4) * UNIT words of `prev` fit, PNG_MAX_ROW / UNIT being a
// multiple of 4. -> bit 0: a filter byte above 4 (status 3), bit 1: store.over (status 5)
template <bool LACE, class Store>
__device__ __forceinline__ int png_unfilter_passes(int width, int height, int bpp, const unsigned char* __restrict__ raw, Store store,
                                                   unsigned* prev, int lane) {
    constexpr int UNIT = Store::UNIT;
    bool bad = false;
    for (int p = 0; p < (LACE ? 7 : 1); p++) {
        store.ps = LACE ? png_pass(width, height, p) : png_whole(width, height);
        if (store.ps.w == 0 || store.ps.h == 0) continue;
        const int units = UNIT == 1 ? (int)(((int64_t)store.ps.w * bpp + 7) >> 3) : store.ps.w;
        png_unfilter_image<UNIT>(raw, store, prev, units, store.ps.h, lane, bad);
        raw += (int64_t)store.ps.h * (1 + (int64_t)units * UNIT);
    }
    return (bad ? 1 : 0) | (store.over ? 2 : 0);
}

// The walk behind a call, for png_unfilter_kernel<1>: with the walks of its six stores inlined into one body its packed rows
// ran 3 % slower than before (435 4-bit palette files of 224 x 224: 694 us against 674 us), each behind a call of its own 2 %
// faster (660 us; profiles/png_unfilter_refactor.txt). png_unfilter_kernel<0> inlines its two walks: a call saves registers to
// scratch memory, and that kernel has none.
template <bool LACE, class Store>
__device__ __noinline__ int png_unfilter_passes_call(int width, int height, int bpp, const unsigned char* __restrict__ raw, Store store,
                                                     unsigned* prev, int lane) {
    return png_unfilter_passes<LACE>(width, height, bpp, raw, store, prev, lane);
}

// The walk with the store of the record's format; MODES as in png_unfilter_kernel: <0> never sees another format than 8-bit RGB
// and grey
template <int MODES, bool LACE>
__device__ __forceinline__ int png_unfilter_record(const PngImage& im, const PngFormat& f, const unsigned char* __restrict__ raw, unsigned char* out,
                                                   unsigned* prev, int lane) {
    const auto run = [&](auto store) {
        return MODES ? png_unfilter_passes_call<LACE>(im.width, im.height, f.bpp, raw, store, prev, lane)
                     : png_unfilter_passes<LACE>(im.width, im.height, f.bpp, raw, store, prev, lane);
    };
    const PngPass ps{};                                 // (png_unfilter_passes sets it)
    if (!MODES) return f.samples == 3 ? run(PngSampleStore<3, 1, LACE>{out, im.width, ps}) : run(PngSampleStore<1, 1, LACE>{out, im.width, ps});
    if (f.packed) return run(PngPackedStore<LACE>{out, im.width, f.layout, f.depth, f.entries, ps, false});
    if (f.sample_bytes == 1) return f.samples == 4 ? run(PngSampleStore<4, 1, LACE>{out, im.width, ps}) : run(PngSampleStore<2, 1, LACE>{out, im.width, ps});
    return f.samples == 3   ? run(PngSampleStore<3, 2, LACE>{out, im.width, ps})
           : f.samples == 4 ? run(PngSampleStore<4, 2, LACE>{out, im.width, ps})
                            : run(PngSampleStore<2, 2, LACE>{out, im.width, ps});
}

// MODES 0: the records of clipmi_png_decode_rgb8 (units 3 and 1 only, the kernel of the measured workload: it must not carry the
// registers of the wide units), 1: those of clipmi_png_decode_px8. Status 3: a filter byte above 4; 5: an index beyond the palette.
template <int MODES>
__global__ void __launch_bounds__(PNG_T) png_unfilter_kernel(const PngImage* __restrict__ images, const unsigned char* __restrict__ rawbuf,
                                                             unsigned char* __restrict__ out, int32_t* status) {
    __shared__ unsigned prev[PNG_MAX_ROW / 4];         // a band's last row: PNG_MAX_ROW bytes (png_format refused longer rows)
    if (status[blockIdx.x] != 0) return;               // nothing was inflated: the record or the stream was refused
    const PngImage im = images[blockIdx.x];
    const int lane = threadIdx.x;
    PngFormat f;
    if (!png_format(im, MODES, f)) return;             // (not reached: png_inflate_kernel gave status 1)
    const unsigned char* raw = rawbuf + im.raw_off;
    const int flags = f.interlaced ? png_unfilter_record<MODES, true>(im, f, raw, out + im.out_off, prev, lane)
                                   : png_unfilter_record<MODES, false>(im, f, raw, out + im.out_off, prev, lane);
    const int is_bad = __syncthreads_or(flags & 1), is_over = MODES ? __syncthreads_or(flags & 2) : 0;
    if (lane == 0 && (is_bad || is_over)) status[blockIdx.x] = is_bad ? 3 : 5;
}

// ---- Adler-32 of the scanlines. With d_0 .. d_{n-1} the bytes: s1 = 1 + sum d_i, s2 = n + sum (n - i) d_i (mod 65521), which is
// what combining per-piece sums by s2 = s2A + s2B + lenB (s1A - 1) comes to. Each thread adds its 16-byte pieces exactly in 64
// bits: a piece contributes at most 2^31 x 4080 < 2^43, and a thread sees at most 2^31 / 16 / 256 = 2^19 pieces, so < 2^62.
constexpr int PNG_ADLER_T = 256;
constexpr unsigned long long PNG_ADLER_MOD = 65521ull;

__global__ void __launch_bounds__(PNG_ADLER_T) png_adler_kernel(const PngImage* __restrict__ images, const unsigned char* __restrict__ rawbuf,
                                                                const unsigned* __restrict__ adler_want, int32_t* status, int modes) {
    __shared__ unsigned long long red1[PNG_ADLER_T], red2[PNG_ADLER_T];
    if (status[blockIdx.x] != 0) return;
    const PngImage im = images[blockIdx.x];
    PngFormat fmt;
    if (!png_format(im, modes, fmt)) return;                       // (not reached: png_inflate_kernel gave status 1)
    const unsigned n = (unsigned)png_scanline_bytes(im, fmt);
    const unsigned char* raw = rawbuf + im.raw_off;
    const int tid = threadIdx.x;
    unsigned long long s1 = 0, s2 = 0;
    const unsigned pieces = n / 16u;
    for (unsigned p = tid; p < pieces; p += PNG_ADLER_T) {
        const uint4 v = *reinterpret_cast<const uint4*>(raw + (size_t)p * 16u);
        const unsigned wv[4] = {v.x, v.y, v.z, v.w};
        unsigned p1 = 0, pk = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const unsigned d = (wv[k >> 2] >> (8 * (k & 3))) & 255u;
            p1 += d;
            pk += (unsigned)k * d;
        }
        s1 += p1;
        s2 += (unsigned long long)(n - p * 16u) * p1 - pk;          // sum (n - i0 - k) d_k
    }
    const unsigned i = pieces * 16u + (unsigned)tid;                // the last n % 16 bytes
    if (i < n) {
        const unsigned d = raw[i];
        s1 += d;
        s2 += (unsigned long long)(n - i) * d;
    }
    red1[tid] = s1 % PNG_ADLER_MOD;
    red2[tid] = s2 % PNG_ADLER_MOD;
    __syncthreads();
    for (int s = PNG_ADLER_T / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red1[tid] += red1[tid + s];
            red2[tid] += red2[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned a = (unsigned)((1ull + red1[0]) % PNG_ADLER_MOD), b = (unsigned)(((unsigned long long)n + red2[0]) % PNG_ADLER_MOD);
        if ((b << 16 | a) != adler_want[blockIdx.x]) status[blockIdx.x] = 4;
    }
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" int64_t clipmi_png_workspace_bytes(int n, int64_t total_raw_bytes) {
    if (n < 0 || total_raw_bytes < 0) return -1;
    return (int64_t)align_up((size_t)total_raw_bytes, 256) + (int64_t)align_up((size_t)n * sizeof(unsigned), 256);
}

// the three launches behind both entries; modes: 0 clipmi_png_decode_rgb8, 1 clipmi_png_decode_px8
static int png_decode(const char* who, int modes, const void* streams_dev, const void* images_dev, int n, int64_t total_raw_bytes,
                      int64_t max_raw_bytes, void* out_dev, int32_t* status_dev, void* ws_dev, int64_t ws_bytes, void* stream) {
    static_assert(sizeof(PngImage) == sizeof(clipmi_png_image) && sizeof(PngImage) == 48, "clipmi_png_image layout");
    if (!streams_dev || !images_dev || !out_dev || !status_dev || !ws_dev || n < 1 || total_raw_bytes < 1 || max_raw_bytes < 1 ||
        max_raw_bytes > total_raw_bytes || max_raw_bytes > 0x7fffffffLL || (reinterpret_cast<uintptr_t>(ws_dev) & 15))
        return set_err(CLIPMI_EINVAL, "%s: bad arguments", who);
    if (n > 0x7fffffff / 2)
        return set_err(CLIPMI_EINVAL, "%s: batch too large for one launch", who);
    if (ws_bytes < clipmi_png_workspace_bytes(n, total_raw_bytes))
        return set_err(CLIPMI_EWORKSPACE, "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes,
                       (long long)clipmi_png_workspace_bytes(n, total_raw_bytes));
    hipStream_t st = as_stream(stream);
    Arena ar(ws_dev, (size_t)ws_bytes);
    unsigned char* raw = ar.take<unsigned char>((size_t)total_raw_bytes);
    unsigned* want = ar.take<unsigned>((size_t)n);
    const PngImage* images = static_cast<const PngImage*>(images_dev);
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)n), dim3(PNG_T), 0, st, static_cast<const unsigned char*>(streams_dev), images,
                       total_raw_bytes, max_raw_bytes, raw, want, status_dev, modes);
    CLIPMI_CHECK_LAUNCH("png_inflate_kernel");
    hipLaunchKernelGGL(modes ? png_unfilter_kernel<1> : png_unfilter_kernel<0>, dim3((unsigned)n), dim3(PNG_T), 0, st, images, raw,
                       static_cast<unsigned char*>(out_dev), status_dev);
    CLIPMI_CHECK_LAUNCH("png_unfilter_kernel");
    hipLaunchKernelGGL(png_adler_kernel, dim3((unsigned)n), dim3(PNG_ADLER_T), 0, st, images, raw, want, status_dev, modes);
    CLIPMI_CHECK_LAUNCH("png_adler_kernel");
    return 0;
}

extern "C" int clipmi_png_decode_rgb8(const void* streams_dev, const void* images_dev, int n, int64_t total_raw_bytes,
                                      int64_t max_raw_bytes, void* out_dev, int32_t* status_dev, void* ws_dev, int64_t ws_bytes,
                                      void* stream) {
    return png_decode("png_decode_rgb8", 0, streams_dev, images_dev, n, total_raw_bytes, max_raw_bytes, out_dev, status_dev, ws_dev,
                      ws_bytes, stream);
}

extern "C" int64_t clipmi_png_px8_workspace_bytes(int n, int64_t total_raw_bytes) {
    return clipmi_png_workspace_bytes(n, total_raw_bytes);
}

extern "C" int clipmi_png_decode_px8(const void* streams_dev, const void* images_dev, int n, int64_t total_raw_bytes,
                                     int64_t max_raw_bytes, void* out_dev, int32_t* status_dev, void* ws_dev, int64_t ws_bytes,
                                     void* stream) {
    return png_decode("png_decode_px8", 1, streams_dev, images_dev, n, total_raw_bytes, max_raw_bytes, out_dev, status_dev, ws_dev,
                      ws_bytes, stream);
}
