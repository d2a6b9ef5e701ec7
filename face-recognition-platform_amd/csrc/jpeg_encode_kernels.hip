// Baseline JPEG encoder for rectangles of the resident frames (frp.h: frp_encode_jpeg; host side: jpeg_encode_api.cpp) - or for images
// in another device buffer of 3-byte pixels (frp_encode_jpeg_enhanced: the enhancer's output): an image is a first pixel and a row pitch.
// All arithmetic is libjpeg's integer arithmetic at its defaults (jccolor / jcsample / jfdctint / jcdctmgr / jccoefct / jchuff), so the
// files equal PIL's byte for byte (tests/test_gpu_jpeg_encode.py against tests/jpeg_encode_model.py and PIL).
//
// Forward half - jpeg_enc_forward_kernel, 256 threads = 32 blocks of 8 x 8:
//   A. every thread fetches 8 samples: colour conversion (and the 2 x 2 box filter of 4:2:0 chroma, bias 1, 2, 1, 2 by output column)
//      straight from the frame bytes; edges are replicated by clamping the pixel (and, for chroma, first the downsampled row) index;
//   B. / C. one thread per row, then per column, of a block: the two LL&M passes of jfdctint through LDS (row stride 9, block stride 72
//      dwords: both passes hit 32 distinct banks per half wave);
//   D. quantisation, int16 stores in natural order.
//   A dummy block of a partial MCU (4:2:0 luma only: at most one column and one row of them) keeps the DC of a real block whose place
//   follows from the geometry alone - the block to its left, or the last block of the row above in its MCU - so it is computed from that
//   block's samples with its AC zeroed: no pass over the finished coefficients.
//
// Entropy half - nothing in it is serial.  A block's DC difference needs the DC of the previous block of its component in scan order,
// whose place is known; bit positions are prefix sums.
//   jpeg_enc_bits_kernel      a wave per block, lane = zig-zag position: __ballot of the non-zero lanes gives every lane its zero run
//                             (ZRL prefixes for runs >= 16 are part of the lane's code, EOB is lane 63's when coefficient 63 is zero);
//                             the wave's sum of code lengths -> blk_bits (scan order)
//   jpeg_enc_hist_kernel      (FRP_FLAG_JPEG_OPTIMIZE only, in front of the others) the same lanes, counting the symbols instead of
//                             coding them: per image dc [2][16] + ac [2][256], from which the host makes the image's own tables
//                             (tab[i * tab_stride]: Annex K's for every image, or one set per image)
//   prefix sum 1              bit_prefix over all blocks of the call; an interval's bits are a difference of two entries
//   jpeg_enc_intervals_kernel each interval gets words [int_word, ...) of the unstuffed stream: (bits before it >> 5) + its index, which
//                             leaves every interval its own words without a second scan (intervals start on a word)
//   jpeg_enc_pack_kernel      the codes again, OR-ed into the zeroed words with vector atomics; an interval's last block adds the 1-padding
//   jpeg_enc_ffcount_kernel + prefix sum 2: 0xFF bytes per chunk of words -> where stuffing moves every byte
//   jpeg_enc_layout_kernel + prefix sum 3: bytes per interval in the file (stuffed, + RSTm) -> every interval's offset; img_off for the host
//   jpeg_enc_emit_kernel      a thread per word: its four bytes, a 0x00 behind every 0xFF, the RSTm behind an interval's last byte
// Bounds: every frame byte read lies in a validated rectangle (and below total_bytes); every coefficient index is below n_blocks * 64 by
// construction of the grids; every access to `words` checks n_words, every store to `out` checks out_bytes - the output length depends
// on the data, the guards do not.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "frp_internal.h"

namespace frp {

typedef unsigned long long u64;

#define JE_BLOCKS 32
#define JE_BS 72
#define JE_RS 9

__constant__ unsigned char je_zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// largest i in [0, n) with img[i].blk0 <= g
__device__ inline int je_image_of_block(const JpegEncParams& p, long long g) {
    int lo = 0, hi = p.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p.img[mid].blk0 <= g) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ inline int je_image_of_interval(const JpegEncParams& p, long long I) {
    int lo = 0, hi = p.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)p.img[mid].int0 <= I) lo = mid; else hi = mid;
    }
    return lo;
}

// ----------------------------------------------------------------------------------------------------------------- forward half
constexpr int je_fix(double x) { return (int)(x * 65536.0 + 0.5); }

__device__ inline int je_component(const JpegEncParams& p, long long a, int comp) {
    int b0 = 0, b1 = 0, b2 = 0;
    if (a >= 0 && a + 2 < p.total_bytes) { b0 = p.frames[a]; b1 = p.frames[a + 1]; b2 = p.frames[a + 2]; }
    const int R = p.rgb_in ? b0 : b2, G = b1, B = p.rgb_in ? b2 : b0;
    if (comp == 0) return (je_fix(0.299) * R + je_fix(0.587) * G + je_fix(0.114) * B + 32768) >> 16;
    if (comp == 1) return (-je_fix(0.16874) * R - je_fix(0.33126) * G + je_fix(0.5) * B + (128 << 16) + 32767) >> 16;
    return (je_fix(0.5) * R - je_fix(0.41869) * G - je_fix(0.08131) * B + (128 << 16) + 32767) >> 16;
}

#define JE_CONST_BITS 13
#define JE_PASS1_BITS 2
__device__ inline int je_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one LL&M pass (jfdctint.c) over d[0..7] in place
template <bool FIRST>
__device__ inline void je_fdct_1d(int* d) {
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int sh = FIRST ? JE_CONST_BITS - JE_PASS1_BITS : JE_CONST_BITS + JE_PASS1_BITS;
    d[0] = FIRST ? (tmp10 + tmp11) * (1 << JE_PASS1_BITS) : je_descale(tmp10 + tmp11, JE_PASS1_BITS);
    d[4] = FIRST ? (tmp10 - tmp11) * (1 << JE_PASS1_BITS) : je_descale(tmp10 - tmp11, JE_PASS1_BITS);
    int z1 = (tmp12 + tmp13) * 4433;
    d[2] = je_descale(z1 + tmp13 * 6270, sh);
    d[6] = je_descale(z1 + tmp12 * (-15137), sh);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * (-16069) + z5;
    z4 = z4 * (-3196) + z5;
    d[7] = je_descale(t4 + z1 + z3, sh);
    d[5] = je_descale(t5 + z2 + z4, sh);
    d[3] = je_descale(t6 + z2 + z3, sh);
    d[1] = je_descale(t7 + z1 + z4, sh);
}

__global__ __launch_bounds__(256) void jpeg_enc_forward_kernel(JpegEncParams p) {
    __shared__ int ws[JE_BLOCKS * JE_BS];
    __shared__ int desc[JE_BLOCKS][6];          // image (-1: no such block), component, source block row, column, dummy
    __shared__ unsigned short qd[2][64];
    const int t = threadIdx.x;
    const long long g0 = (long long)blockIdx.x * JE_BLOCKS;
    if (t < 128) qd[t >> 6][t & 63] = p.tab->q[t >> 6][t & 63];
    if (t < JE_BLOCKS) {
        const long long g = g0 + t;
        int im = -1, comp = 0, sr = 0, sc = 0, dummy = 0;
        if (g < p.n_blocks) {
            im = je_image_of_block(p, g);
            const JpegEncImage I = p.img[im];
            long long l = g - I.blk0;
            const long long nb0 = (long long)I.mx * p.hs * I.my * p.vs, nbc = (long long)I.mx * I.my;
            int bx;
            if (l < nb0) { comp = 0; bx = I.mx * p.hs; } else { l -= nb0; comp = 1; if (l >= nbc) { l -= nbc; comp = 2; } bx = I.mx; }
            sr = (int)(l / bx);
            sc = (int)(l - (long long)sr * bx);
            if (comp == 0) {                    // real blocks of luma; chroma grids have no dummies (their factors are 1 x 1)
                const int rbx = (I.w + 7) >> 3, rby = (I.h + 7) >> 3;
                if (sr >= rby) { dummy = 1; sc = min((sc / p.hs) * p.hs + p.hs - 1, rbx - 1); sr = rby - 1; }
                else if (sc >= rbx) { dummy = 1; sc = rbx - 1; }
            }
        }
        desc[t][0] = im; desc[t][1] = comp; desc[t][2] = sr; desc[t][3] = sc; desc[t][4] = dummy;
    }
    __syncthreads();

    // ---- A: samples minus 128
#pragma unroll 2
    for (int i = 0; i < 8; ++i) {
        const int idx = i * 256 + t, b = idx >> 6, y = (idx >> 3) & 7, x = idx & 7;
        const int im = desc[b][0];
        if (im < 0) continue;
        const JpegEncImage I = p.img[im];
        const int comp = desc[b][1];
        const long long row0 = I.pix0;
        int v;
        if (comp == 0 || p.hs == 1) {
            const int py = min(desc[b][2] * 8 + y, I.h - 1), px = min(desc[b][3] * 8 + x, I.w - 1);
            v = je_component(p, (row0 + (long long)py * I.pitch + px) * 3, comp);
        } else {                                  // 2 x 2 box: the last real downsampled row repeats, the full-size edges repeat inside it
            const int oy = min(desc[b][2] * 8 + y, ((I.h + 1) >> 1) - 1), ox = desc[b][3] * 8 + x;
            const int r0 = min(2 * oy, I.h - 1), r1 = min(2 * oy + 1, I.h - 1), c0 = min(2 * ox, I.w - 1), c1 = min(2 * ox + 1, I.w - 1);
            const long long a0 = row0 + (long long)r0 * I.pitch, a1 = row0 + (long long)r1 * I.pitch;
            v = (je_component(p, (a0 + c0) * 3, comp) + je_component(p, (a0 + c1) * 3, comp) + je_component(p, (a1 + c0) * 3, comp) +
                 je_component(p, (a1 + c1) * 3, comp) + 1 + (ox & 1)) >> 2;
        }
        ws[b * JE_BS + y * JE_RS + x] = v - 128;
    }
    __syncthreads();

    // ---- B: rows, C: columns
    {
        const int b = t >> 3, r = t & 7;
        int d[8];
        int* w = ws + b * JE_BS + r * JE_RS;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = desc[b][0] >= 0 ? w[k] : 0;
        je_fdct_1d<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = d[k];
        __syncthreads();
        w = ws + b * JE_BS + r;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = w[k * JE_RS];
        je_fdct_1d<false>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k * JE_RS] = d[k];
    }
    __syncthreads();

    // ---- D: quantise, natural order
#pragma unroll 2
    for (int i = 0; i < 8; ++i) {
        const int idx = i * 256 + t, b = idx >> 6, pos = idx & 63;
        if (desc[b][0] < 0) continue;
        const int c = ws[b * JE_BS + (pos >> 3) * JE_RS + (pos & 7)];
        const int dq = (int)qd[desc[b][1] ? 1 : 0][pos] << 3;
        int mag = ((c < 0 ? -c : c) + (dq >> 1)) / dq;
        if (desc[b][4] && pos) mag = 0;
        p.coef[(g0 + b) * 64 + pos] = (int16_t)(c < 0 ? -mag : mag);
    }
}

// ----------------------------------------------------------------------------------------------------------------- entropy half
struct JeBlock {       // a block in scan order
    long long nat;     // its index in the image's coefficient layout
    long long prev;    // the block whose DC is its prediction, -1: none (first of its component in the interval)
    int comp;
    long long mcu;
};

__device__ inline long long je_nat(const JpegEncParams& p, const JpegEncImage& I, long long m, int k) {
    const int nl = p.hs * p.vs;
    if (k < nl) {
        const long long myy = m / I.mx, mxx = m - myy * I.mx;
        const int v = k / p.hs, hh = k - v * p.hs;
        return (myy * p.vs + v) * ((long long)I.mx * p.hs) + mxx * p.hs + hh;
    }
    return (long long)I.mx * p.hs * I.my * p.vs + (long long)(k - nl) * I.mx * I.my + m;
}

__device__ inline JeBlock je_scan_block(const JpegEncParams& p, const JpegEncImage& I, long long s) {
    const int nl = p.hs * p.vs, bpm = nl + 2;
    JeBlock b;
    b.mcu = s / bpm;
    const int k = (int)(s - b.mcu * bpm);
    b.comp = k < nl ? 0 : k - nl + 1;
    b.nat = je_nat(p, I, b.mcu, k);
    const bool first = p.ri ? (b.mcu % p.ri == 0) : (b.mcu == 0);
    if (k < nl && k > 0) b.prev = je_nat(p, I, b.mcu, k - 1);
    else if (first) b.prev = -1;
    else b.prev = je_nat(p, I, b.mcu - 1, k < nl ? nl - 1 : k);
    return b;
}

// What this lane's zig-zag position contributes to the scan - the ONE definition of the symbols, for the kernels that code them
// (je_lane_code) and the one that counts them (jpeg_enc_hist_kernel).  Called by whole waves (__ballot).
enum { JE_NONE = 0, JE_DC, JE_AC, JE_EOB };      // a zero coefficient inside the block | lane 0 | a non-zero AC | lane 63 when it is zero
struct JeSymbol {
    int kind;
    int tb;            // table: 0 luminance, 1 chrominance
    int v;             // the coefficient (lane 0: the DC difference)
    int size;          // its magnitude category: the DC symbol, the low nibble of the AC symbol
    int run;           // JE_AC: zeros since the last non-zero AC; run >> 4 ZRL symbols precede the symbol (run & 15) << 4 | size
};
__device__ inline JeSymbol je_lane_symbol(const JpegEncParams& p, const JpegEncImage& I, const JeBlock& b, int lane) {
    const int16_t* c = p.coef + (I.blk0 + b.nat) * 64;
    JeSymbol s;
    s.v = c[je_zigzag[lane]];
    if (lane == 0 && b.prev >= 0) s.v -= p.coef[(I.blk0 + b.prev) * 64];
    const u64 nz = __ballot(s.v != 0) & ~1ull;                // non-zero AC positions
    s.tb = b.comp ? 1 : 0;
    const unsigned a = (unsigned)(s.v < 0 ? -s.v : s.v);
    s.size = a ? 32 - __clz(a) : 0;
    s.run = 0;
    if (lane == 0) s.kind = JE_DC;
    else if (s.v != 0) {
        const u64 below = nz & ((1ull << lane) - 1ull);
        const int prevpos = below ? 63 - __clzll((long long)below) : 0;
        s.run = lane - prevpos - 1;
        s.kind = JE_AC;
    } else s.kind = lane == 63 ? JE_EOB : JE_NONE;
    return s;
}

// the code of this lane's zig-zag position with the image's tables T: `pre` (prelen bits: the ZRL codes of a run >= 16, at most
// 3 * 16) in front of `code` (len bits: Huffman code + magnitude bits, at most 16 + 11), both right-aligned; 0 bits for a zero
// coefficient that is not the end of the block.  (Two parts: with Annex K's 11-bit ZRL a lane's bits fit 64, with a table of the
// image's own, where ZRL may take 16, they need not.)
__device__ inline void je_lane_code(const JpegEncTables& T, const JeSymbol& s, u64& pre, int& prelen, u64& code, int& len) {
    const u64 vbits = (u64)((unsigned)(s.v > 0 ? s.v : s.v - 1) & ((1u << s.size) - 1u));
    pre = 0;
    prelen = 0;
    code = 0;
    len = 0;
    if (s.kind == JE_DC) {
        const uint32_t e = T.dc[s.tb][s.size & 15];
        code = ((u64)(e & 0xffffu) << s.size) | vbits;
        len = (int)(e >> 16) + s.size;
    } else if (s.kind == JE_AC) {
        const uint32_t zrl = T.ac[s.tb][0xF0], e = T.ac[s.tb][((s.run & 15) << 4) | (s.size & 15)];
        for (int i = 0; i < (s.run >> 4); ++i) {
            pre = (pre << (zrl >> 16)) | (zrl & 0xffffu);
            prelen += (int)(zrl >> 16);
        }
        code = ((u64)(e & 0xffffu) << s.size) | vbits;
        len = (int)(e >> 16) + s.size;
    } else if (s.kind == JE_EOB) {
        const uint32_t e = T.ac[s.tb][0];
        code = e & 0xffffu;
        len = (int)(e >> 16);
    }
}

__device__ inline int je_wave_inclusive(int x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

__global__ __launch_bounds__(256) void jpeg_enc_bits_kernel(JpegEncParams p) {
    const int lane = threadIdx.x & 63;
    const long long S = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (S >= p.n_blocks) return;                              // (whole waves leave: S is uniform in a wave)
    const int im = je_image_of_block(p, S);
    const JpegEncImage I = p.img[im];
    const JeBlock b = je_scan_block(p, I, S - I.blk0);
    u64 pre, code;
    int prelen, len;
    je_lane_code(p.tab[(size_t)im * p.tab_stride], je_lane_symbol(p, I, b, lane), pre, prelen, code, len);
    const int tot = je_wave_inclusive(prelen + len, lane);
    if (lane == 63) p.blk_bits[S] = (uint32_t)tot;
}

// The symbol counts of every image (FRP_FLAG_JPEG_OPTIMIZE): the index space of jpeg_enc_bits_kernel, JE_HIST_WG_BLOCKS consecutive
// blocks per workgroup, a wave per block, lane = zig-zag position.  Counts gather in LDS - the EOB and 0x01 bins are hit by nearly
// every block - and the non-zero bins go to the image's histogram with one vector atomic each.  The blocks of all images form one
// index space, so a workgroup may span images (a small crop is 3 or 6 blocks): it works image by image and flushes and clears at
// every boundary.  Integer adds: the result does not depend on the order.
#define JE_HIST_WG_BLOCKS 256
__global__ __launch_bounds__(256) void jpeg_enc_hist_kernel(JpegEncParams p) {
    __shared__ uint32_t h[JE_HIST_BINS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long g0 = (long long)blockIdx.x * JE_HIST_WG_BLOCKS, g1 = min(g0 + JE_HIST_WG_BLOCKS, p.n_blocks);
    for (int i = threadIdx.x; i < JE_HIST_BINS; i += 256) h[i] = 0;
    __syncthreads();
    if (g0 >= g1) return;                                     // (never: the grid covers n_blocks)
    int im = je_image_of_block(p, g0);
    long long s = g0;
    while (s < g1 && im < p.n) {                              // (uniform in the workgroup: the barriers below are met by all)
        const JpegEncImage I = p.img[im];
        const long long end = im + 1 < p.n ? min(g1, p.img[im + 1].blk0) : g1;
        for (long long S = s + wv; S < end; S += 4) {         // (S is uniform in a wave)
            const JeSymbol y = je_lane_symbol(p, I, je_scan_block(p, I, S - I.blk0), lane);
            if (y.kind == JE_DC) atomicAdd(&h[y.tb * 16 + (y.size & 15)], 1u);
            else if (y.kind == JE_AC) {
                atomicAdd(&h[32 + y.tb * 256 + (((y.run & 15) << 4) | (y.size & 15))], 1u);
                if (y.run >> 4) atomicAdd(&h[32 + y.tb * 256 + 0xF0], (uint32_t)(y.run >> 4));
            } else if (y.kind == JE_EOB) atomicAdd(&h[32 + y.tb * 256], 1u);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < JE_HIST_BINS; i += 256) {
            const uint32_t c = h[i];
            if (c) {
                atomicAdd(p.hist + (size_t)im * JE_HIST_BINS + i, c);
                h[i] = 0;
            }
        }
        __syncthreads();
        s = end;
        ++im;
    }
}

// `len` bits of code at bit `bit` of the stream that starts at word w0
__device__ inline void je_put(const JpegEncParams& p, u64 w0, u64 bit, u64 code, int len) {
    u64 w = w0 + (bit >> 5);
    int off = (int)(bit & 31);
    while (len > 0) {
        const int space = 32 - off, take = min(space, len);
        const uint32_t chunk = (uint32_t)((code >> (len - take)) & ((1ull << take) - 1ull));
        if (chunk && w < p.n_words) atomicOr(p.words + w, chunk << (space - take));
        len -= take;
        off = 0;
        ++w;
    }
}

// first and one-past-last scan block (over all images) of interval t of image I
__device__ inline void je_interval_blocks(const JpegEncParams& p, const JpegEncImage& I, long long t, long long& s0, long long& s1) {
    const long long nm = (long long)I.mx * I.my, bpm = p.hs * p.vs + 2;
    const long long m0 = p.ri ? t * p.ri : 0, m1 = p.ri ? min(m0 + p.ri, nm) : nm;
    s0 = I.blk0 + m0 * bpm;
    s1 = I.blk0 + m1 * bpm;
}

__global__ __launch_bounds__(256) void jpeg_enc_intervals_kernel(JpegEncParams p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i > p.n_int) return;
    if (i == p.n_int) {
        p.int_word[i] = (p.bit_prefix[p.n_blocks] >> 5) + (u64)i;
        return;
    }
    const JpegEncImage I = p.img[je_image_of_interval(p, i)];
    long long s0, s1;
    je_interval_blocks(p, I, i - I.int0, s0, s1);
    const u64 P0 = p.bit_prefix[s0], P1 = p.bit_prefix[s1];
    p.int_word[i] = (P0 >> 5) + (u64)i;
    p.int_bytes[i] = (uint32_t)((P1 - P0 + 7) >> 3);
}

__global__ __launch_bounds__(256) void jpeg_enc_pack_kernel(JpegEncParams p) {
    const int lane = threadIdx.x & 63;
    const long long S = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (S >= p.n_blocks) return;
    const int im = je_image_of_block(p, S);
    const JpegEncImage I = p.img[im];
    const JeBlock b = je_scan_block(p, I, S - I.blk0);
    u64 pre, code;
    int prelen, len;
    je_lane_code(p.tab[(size_t)im * p.tab_stride], je_lane_symbol(p, I, b, lane), pre, prelen, code, len);
    const int incl = je_wave_inclusive(prelen + len, lane);
    const long long t = p.ri ? b.mcu / p.ri : 0;
    long long s0, s1;
    je_interval_blocks(p, I, t, s0, s1);
    const u64 w0 = p.int_word[I.int0 + t];
    const u64 at = p.bit_prefix[S] - p.bit_prefix[s0];        // of the block inside its interval
    if (prelen) je_put(p, w0, at + (u64)(incl - prelen - len), pre, prelen);
    if (len) je_put(p, w0, at + (u64)(incl - len), code, len);
    if (lane == 63 && S + 1 == s1) {                          // the interval ends here: 1-bits up to the byte
        const u64 end = at + (u64)incl;
        const int padn = (int)((8 - (end & 7)) & 7);
        if (padn) je_put(p, w0, end, (1ull << padn) - 1ull, padn);
    }
}

__device__ inline int je_ff_in_word(uint32_t w) {
    return ((w >> 24) == 0xFFu) + (((w >> 16) & 0xFFu) == 0xFFu) + (((w >> 8) & 0xFFu) == 0xFFu) + ((w & 0xFFu) == 0xFFu);
}

// exclusive sum of x over the 256 threads of the workgroup (red: 4 ints of LDS); total in `total`
__device__ inline int je_wg_exclusive(int x, int* red, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int incl = je_wave_inclusive(x, lane);
    if (lane == 63) red[wv] = incl;
    __syncthreads();
    int before = 0;
    for (int i = 0; i < wv; ++i) before += red[i];
    total = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return before + incl - x;
}

__global__ __launch_bounds__(256) void jpeg_enc_ffcount_kernel(JpegEncParams p) {
    __shared__ int red[4];
    const u64 w = (u64)blockIdx.x * JE_CHUNK_WORDS + threadIdx.x;
    const int c = w < p.n_words ? je_ff_in_word(p.words[w]) : 0;
    int total;
    (void)je_wg_exclusive(c, red, total);
    if (threadIdx.x == 0) p.ff_chunk[blockIdx.x] = (uint32_t)total;
}

// 0xFF bytes of `words` before byte g (of the whole stream), by one wave
__device__ inline u64 je_ff_before(const JpegEncParams& p, u64 g, int lane) {
    const u64 chunk = g / (JE_CHUNK_WORDS * 4);
    const u64 wfirst = chunk * JE_CHUNK_WORDS, wlast = g >> 2;         // whole words [wfirst, wlast), then g & 3 bytes of wlast
    int c = 0;
    for (u64 w = wfirst + lane; w <= wlast; w += 64) {
        if (w >= p.n_words) break;
        uint32_t x = p.words[w];
        if (w == wlast) {
            const int nb = (int)(g & 3);
            x = nb ? x & ~(0xFFFFFFFFu >> (8 * nb)) : 0u;             // keep the first nb bytes; 0x00 never counts
        }
        c += je_ff_in_word(x);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    return (chunk < (u64)p.n_chunks ? p.ff_prefix[chunk] : p.ff_prefix[p.n_chunks]) + (u64)c;
}

__global__ __launch_bounds__(256) void jpeg_enc_layout_kernel(JpegEncParams p) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= p.n_int) return;
    const JpegEncImage I = p.img[je_image_of_interval(p, i)];
    const u64 g0 = p.int_word[i] * 4, g1 = g0 + p.int_bytes[i];
    const u64 f0 = je_ff_before(p, g0, lane), f1 = je_ff_before(p, g1, lane);
    if (lane == 0) {
        p.int_ff0[i] = f0;
        p.int_outb[i] = p.int_bytes[i] + (uint32_t)(f1 - f0) + ((i - I.int0 < I.n_int - 1) ? 2u : 0u);
    }
}

__global__ __launch_bounds__(256) void jpeg_enc_offsets_kernel(JpegEncParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > p.n) return;
    p.img_off[i] = i < p.n ? p.int_out[p.img[i].int0] : p.int_out[p.n_int];
}

__device__ inline void je_store(const JpegEncParams& p, u64 at, unsigned char v) {
    if (at < p.out_bytes) p.out[at] = v;
}

__global__ __launch_bounds__(256) void jpeg_enc_emit_kernel(JpegEncParams p) {
    __shared__ int red[4];
    const u64 w = (u64)blockIdx.x * JE_CHUNK_WORDS + threadIdx.x;
    const bool live = w < p.n_words && w < p.int_word[p.n_int];
    const uint32_t x = live ? p.words[w] : 0u;
    int total;
    const int before = je_wg_exclusive(je_ff_in_word(x), red, total);
    if (!live) return;
    long long lo = 0, hi = p.n_int;                           // the interval whose words hold w: int_word[lo] <= w < int_word[hi]
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (p.int_word[mid] <= w) lo = mid; else hi = mid;
    }
    const u64 j0 = (w - p.int_word[lo]) * 4, nbytes = p.int_bytes[lo];
    if (j0 >= nbytes) return;                                 // a word between two intervals
    const int im = je_image_of_interval(p, lo);
    const JpegEncImage I = p.img[im];
    const u64 ffb = p.ff_prefix[blockIdx.x] + (u64)before - p.int_ff0[lo];
    u64 at = p.scan_base[im] + (p.int_out[lo] - p.int_out[I.int0]) + j0 + ffb;
    const long long t = lo - I.int0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (j0 + k >= nbytes) break;
        const unsigned char v = (unsigned char)(x >> (24 - 8 * k));
        je_store(p, at++, v);
        if (v == 0xFF) je_store(p, at++, 0);
        if (j0 + k == nbytes - 1 && t < I.n_int - 1) {
            je_store(p, at++, 0xFF);
            je_store(p, at++, (unsigned char)(0xD0 + (t & 7)));
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- prefix sums
// out[i] = sum of in[0..i) for i in [0, n], 64-bit: 1024 elements per workgroup, the workgroups' totals by one workgroup, then added back
#define JE_SCAN_ELEMS 1024
size_t jpeg_enc_scan_groups(long long n) { return (size_t)((n + JE_SCAN_ELEMS - 1) / JE_SCAN_ELEMS) + 1; }

__global__ __launch_bounds__(256) void je_scan_local_kernel(const uint32_t* in, long long n, u64* out, u64* group_tot) {
    __shared__ u64 red[4];
    const long long base = (long long)blockIdx.x * JE_SCAN_ELEMS + (long long)threadIdx.x * 4;
    uint32_t v[4];
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = base + k < n ? in[base + k] : 0u;
        s += v[k];
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u64 incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
    }
    if (lane == 63) red[wv] = incl;
    __syncthreads();
    u64 run = incl - s;
    for (int i = 0; i < wv; ++i) run += red[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 255) group_tot[blockIdx.x] = run;
}

__global__ __launch_bounds__(64) void je_scan_groups_kernel(u64* group_tot, long long groups) {     // one wave: in place, [groups] = everything
    const int lane = threadIdx.x;
    u64 carry = 0;
    for (long long g0 = 0; g0 < groups; g0 += 64) {
        const u64 x = g0 + lane < groups ? group_tot[g0 + lane] : 0ull;
        u64 incl = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 y = __shfl_up(incl, d);
            if (lane >= d) incl += y;
        }
        if (g0 + lane < groups) group_tot[g0 + lane] = carry + incl - x;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) group_tot[groups] = carry;
}

__global__ __launch_bounds__(256) void je_scan_add_kernel(u64* out, long long n, const u64* group_tot, long long groups) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] += group_tot[i / JE_SCAN_ELEMS];
    else if (i == n) out[n] = group_tot[groups];
}

static hipError_t je_prefix_sum(const uint32_t* in, long long n, u64* out, u64* group_tot, hipStream_t stream) {
    const long long groups = (n + JE_SCAN_ELEMS - 1) / JE_SCAN_ELEMS;
    hipLaunchKernelGGL(je_scan_local_kernel, dim3((unsigned)groups), dim3(256), 0, stream, in, n, out, group_tot);
    hipLaunchKernelGGL(je_scan_groups_kernel, dim3(1), dim3(64), 0, stream, group_tot, groups);
    hipLaunchKernelGGL(je_scan_add_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, stream, out, n, (const u64*)group_tot, groups);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------------------------------------- launchers
static bool je_common_ok(const JpegEncParams& p) {
    return p.frames && p.img && p.tab && p.coef && p.n > 0 && p.n_blocks > 0 && p.n_blocks < (1LL << 31) && p.total_bytes > 0 && ((p.hs == 2 && p.vs == 2) || (p.hs == 1 && p.vs == 1)) && p.ri >= 0 &&
           (p.tab_stride == 0 || p.tab_stride == 1);
}
static bool je_entropy_ok(const JpegEncParams& p) {
    return je_common_ok(p) && p.n_int >= p.n && p.n_int < (1LL << 31) && p.blk_bits && p.bit_prefix && p.group_tot && p.int_word && p.int_bytes &&
           p.int_ff0 && p.int_outb && p.int_out && p.img_off;
}

hipError_t launch_jpeg_enc_forward(const JpegEncParams& p, hipStream_t stream) {
    if (!je_common_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jpeg_enc_forward_kernel, dim3((unsigned)((p.n_blocks + JE_BLOCKS - 1) / JE_BLOCKS)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_jpeg_enc_hist(const JpegEncParams& p, hipStream_t stream) {
    if (!je_common_ok(p) || !p.hist) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jpeg_enc_hist_kernel, dim3((unsigned)((p.n_blocks + JE_HIST_WG_BLOCKS - 1) / JE_HIST_WG_BLOCKS)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_jpeg_enc_measure(const JpegEncParams& p, hipStream_t stream) {
    if (!je_entropy_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jpeg_enc_bits_kernel, dim3((unsigned)((p.n_blocks + 3) / 4)), dim3(256), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return je_prefix_sum(p.blk_bits, p.n_blocks, p.bit_prefix, p.group_tot, stream);
}

hipError_t launch_jpeg_enc_pack(const JpegEncParams& p, hipStream_t stream) {
    if (!je_entropy_ok(p) || !p.words || !p.ff_chunk || !p.ff_prefix || p.n_chunks != (long long)((p.n_words + JE_CHUNK_WORDS - 1) / JE_CHUNK_WORDS) ||
        p.n_chunks <= 0 || p.n_chunks >= (1LL << 31))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(jpeg_enc_intervals_kernel, dim3((unsigned)((p.n_int + 1 + 255) / 256)), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(jpeg_enc_pack_kernel, dim3((unsigned)((p.n_blocks + 3) / 4)), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(jpeg_enc_ffcount_kernel, dim3((unsigned)p.n_chunks), dim3(256), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = je_prefix_sum(p.ff_chunk, p.n_chunks, p.ff_prefix, p.group_tot, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_enc_layout_kernel, dim3((unsigned)((p.n_int + 3) / 4)), dim3(256), 0, stream, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = je_prefix_sum(p.int_outb, p.n_int, p.int_out, p.group_tot, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_enc_offsets_kernel, dim3((unsigned)((p.n + 1 + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_jpeg_enc_emit(const JpegEncParams& p, hipStream_t stream) {
    if (!je_entropy_ok(p) || !p.words || !p.ff_prefix || !p.scan_base || !p.out || p.n_chunks <= 0 || p.n_chunks >= (1LL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jpeg_enc_emit_kernel, dim3((unsigned)p.n_chunks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace frp
