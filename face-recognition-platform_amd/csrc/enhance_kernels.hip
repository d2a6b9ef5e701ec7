// Snapshot enhancer for rectangles of the resident frames (frp.h: frp_enhance_pixels, frp_encode_jpeg_enhanced; host side: enhance_api.cpp):
// Pillow's Image.resize(BICUBIC) followed by ImageFilter.UnsharpMask on 8-bit pixels, in Pillow's own integer arithmetic, so the
// pixels equal Pillow's byte for byte (tests/test_gpu_enhance.py against tests/enhance_model.py and Pillow).  The host computes the
// resample taps and the box blur's weights (they need double / float arithmetic); everything here is integer work.
//
// enhance_kernel, 256 threads, one workgroup per ENH_TILE_W x ENH_TILE_H tile of an OUTPUT image, everything between the frame bytes
// and the finished pixels in LDS - per output pixel 3 bytes go to HBM and (ratio^-2 + halo) * 3 come from it, mostly out of L2:
//   A. the source rows and columns the tile's taps reach, as aligned dwords (the pattern of quality_kernels.hip);
//   B. horizontal resample of every staged source row at the tile's output columns (halo included), rounded to 8 bits as Pillow's
//      intermediate image is; an axis that keeps its size has one tap of 2^22 per sample, which is the identity;
//   C. vertical resample of B -> the resampled tile with a halo of 3 (r + 1) pixels per side, one packed dword per pixel;
//   D. the Gaussian blur of UnsharpMask: three box passes along the rows, then three along the columns, every pass rounded to 8 bits.
//      A pass reads index clamp(x + d, first, last) with [first, last] the part of the line that lies INSIDE THE IMAGE - Pillow's edge
//      rule, at the edge of the enhanced crop - so positions outside the image hold values nobody reads, and what a pass computes from
//      a clamped read at the edge of the TILE is wrong only within r + 1 pixels more of that edge per pass: the core is exact;
//   E. unsharp: d = in - blur, |d| > threshold ? clip8(in + d * percent / 100) : in, bytes packed 3 per pixel in LDS;
//   F. the tile's rows to `out`: whole aligned dwords gathered from E's bytes, single bytes where a row's span starts or ends inside
//      a dword (rows of neighbouring tiles and images share those dwords).
// Bounds: A as in quality_kernels.hip (a dword is loaded whole only if it ends at or before total_bytes); every LDS index is clamped to
// the staged rows / columns, whatever the tables hold; every store checks out_bytes.  No scratch: all loops over taps are unrolled.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "frp_internal.h"

namespace frp {

#define EN_EW (ENH_TILE_W + 2 * ENH_MAX_HALO)        // resampled tile + halo
#define EN_EH (ENH_TILE_H + 2 * ENH_MAX_HALO)
#define EN_SR (EN_EH + 6)                            // source rows / columns behind it: (E - 1) * in / out + 5 <= E + 4 when out >= in
#define EN_SC (EN_EW + 6)
#define EN_RAW_DW 64                                 // dwords per staged source row
#define EN_PX (EN_EW * EN_EH)
#define EN_X_DW (EN_SR * EN_RAW_DW + EN_SR * EN_EW)  // A's dwords and B's pixels live together; D's two buffers reuse the space
#define EN_OB_PITCH (ENH_TILE_W * 3)
static_assert((EN_SC * 3 + 3 + 3) / 4 <= EN_RAW_DW, "a staged row at byte phase 0..3");
static_assert(2 * EN_PX <= EN_X_DW && ENH_TILE_H * EN_OB_PITCH <= EN_PX * 4, "buffer reuse");
static_assert(ENH_MAX_TAPS == 5, "EnhanceTap is two 16-byte loads");

__device__ inline int en_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ inline unsigned en_clip8(int v) { return (unsigned)min(max(v, 0), 255); }

// one output of a box pass over packed pixels line[i * stride], i clamped to [lo, hi]
__device__ inline unsigned en_box(const unsigned* line, int stride, int e, int lo, int hi, int r, unsigned ww, unsigned fw) {
    unsigned s0 = 0u, s1 = 0u, s2 = 0u;
#pragma unroll
    for (int d = -ENH_MAX_BOX_R; d <= ENH_MAX_BOX_R; ++d) {
        if (d >= -r && d <= r) {
            const unsigned v = line[en_clamp(e + d, lo, hi) * stride];
            s0 += v & 255u; s1 += (v >> 8) & 255u; s2 += (v >> 16) & 255u;
        }
    }
    const unsigned va = line[en_clamp(e - r - 1, lo, hi) * stride], vb = line[en_clamp(e + r + 1, lo, hi) * stride];
    const unsigned o0 = (ww * s0 + fw * ((va & 255u) + (vb & 255u)) + (1u << 23)) >> 24;
    const unsigned o1 = (ww * s1 + fw * (((va >> 8) & 255u) + ((vb >> 8) & 255u)) + (1u << 23)) >> 24;
    const unsigned o2 = (ww * s2 + fw * (((va >> 16) & 255u) + ((vb >> 16) & 255u)) + (1u << 23)) >> 24;
    return o0 | (o1 << 8) | (o2 << 16);
}

__device__ inline unsigned en_unsharp(int in, int blur, int percent, int threshold) {
    const int d = in - blur;
    if ((d < 0 ? -d : d) <= threshold) return (unsigned)in;
    return en_clip8(in + (int)((long long)d * percent / 100));
}

__global__ __launch_bounds__(256) void enhance_kernel(EnhanceParams p) {
    __shared__ unsigned X[EN_X_DW];
    __shared__ unsigned Rs[EN_PX];
    unsigned* const raw = X;
    unsigned* const hb = X + EN_SR * EN_RAW_DW;
    unsigned* const bufA = X;
    unsigned* const bufB = X + EN_PX;
    const int t = threadIdx.x;
    const int bid = blockIdx.x;
    int lo = 0, hi = p.n;                                    // img[lo].tile0 <= bid < img[hi].tile0
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p.img[mid].tile0 <= bid) lo = mid; else hi = mid;
    }
    const EnhanceImage I = p.img[lo];
    const int tl = bid - I.tile0;
    const int ty = tl / I.tiles_x, tx = tl - ty * I.tiles_x;
    const int ox0 = tx * ENH_TILE_W, oy0 = ty * ENH_TILE_H;  // first output column / row of the tile
    if (ox0 >= I.ow || oy0 >= I.oh) return;                  // (never, with the host's tile counts)
    const int tw = min(ENH_TILE_W, I.ow - ox0), th = min(ENH_TILE_H, I.oh - oy0);
    const int box_r = en_clamp(p.box_r, 0, ENH_MAX_BOX_R);
    const int hl = p.sharpen ? 3 * (box_r + 1) : 0;
    const int ew = tw + 2 * hl, eh = th + 2 * hl;            // the tile with its halo ...
    const int ex0 = ox0 - hl, ey0 = oy0 - hl;                // ... starts here (may lie outside the image)
    const EnhanceTap* const xt = p.taps + I.xtap;
    const EnhanceTap* const yt = p.taps + I.ytap;
    // source columns / rows of the crop behind it: first and count are monotone in the output index
    const int xl = en_clamp(ex0 + ew - 1, 0, I.ow - 1), yl = en_clamp(ey0 + eh - 1, 0, I.oh - 1);
    const int sx0 = en_clamp(xt[max(ex0, 0)].first, 0, I.w - 1), sy0 = en_clamp(yt[max(ey0, 0)].first, 0, I.h - 1);
    const int ncols = en_clamp(xt[xl].first + xt[xl].count - sx0, 1, min(EN_SC, I.w - sx0));
    const int nrows = en_clamp(yt[yl].first + yt[yl].count - sy0, 1, min(EN_SR, I.h - sy0));
    const int nb = 3 * ncols;
    const long long seg0 = (((long long)I.frame * p.H + I.top + sy0) * p.W + I.left + sx0) * 3;   // byte offset of the first staged row's segment

    // ---- A: the staged rows' bytes as aligned dwords
    for (int idx = t; idx < nrows * EN_RAW_DW; idx += 256) {
        const int rr = idx / EN_RAW_DW, d = idx - rr * EN_RAW_DW;
        const long long s = seg0 + (long long)rr * p.W * 3;
        const long long a = (s & ~3LL) + 4 * d;
        unsigned v = 0u;
        if (a < s + nb) {                                    // the dword holds a byte of the segment
            if (a + 4 <= p.total_bytes) {
                v = *reinterpret_cast<const unsigned*>(p.frames + a);
            } else {                                         // the last, partial dword of the whole buffer
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (a + j < p.total_bytes) v |= (unsigned)p.frames[a + j] << (8 * j);
            }
        }
        raw[idx] = v;
    }
    __syncthreads();

    // ---- B: horizontal resample of every staged row at the tile's columns
    for (int idx = t; idx < nrows * ew; idx += 256) {
        const int rr = idx / ew, e = idx - rr * ew;
        const EnhanceTap tp = xt[en_clamp(ex0 + e, 0, I.ow - 1)];
        const int sh = (int)((seg0 + (long long)rr * p.W * 3) & 3);
        const unsigned char* px = reinterpret_cast<const unsigned char*>(raw + rr * EN_RAW_DW) + sh;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
#pragma unroll
        for (int j = 0; j < ENH_MAX_TAPS; ++j) {
            if (j < tp.count) {
                const unsigned char* q = px + 3 * en_clamp(tp.first + j - sx0, 0, ncols - 1);
                const int k = tp.k[j];
                a0 += (int)q[0] * k; a1 += (int)q[1] * k; a2 += (int)q[2] * k;
            }
        }
        hb[idx] = en_clip8(a0 >> 22) | (en_clip8(a1 >> 22) << 8) | (en_clip8(a2 >> 22) << 16);
    }
    __syncthreads();

    // ---- C: vertical resample -> the resampled tile, halo included
    for (int idx = t; idx < eh * ew; idx += 256) {
        const int r = idx / ew, e = idx - r * ew;
        const EnhanceTap tp = yt[en_clamp(ey0 + r, 0, I.oh - 1)];
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
#pragma unroll
        for (int j = 0; j < ENH_MAX_TAPS; ++j) {
            if (j < tp.count) {
                const unsigned v = hb[en_clamp(tp.first + j - sy0, 0, nrows - 1) * ew + e];
                const int k = tp.k[j];
                a0 += (int)(v & 255u) * k; a1 += (int)((v >> 8) & 255u) * k; a2 += (int)((v >> 16) & 255u) * k;
            }
        }
        Rs[idx] = en_clip8(a0 >> 22) | (en_clip8(a1 >> 22) << 8) | (en_clip8(a2 >> 22) << 16);
    }
    __syncthreads();

    unsigned char* const ob = reinterpret_cast<unsigned char*>(bufA);       // E's bytes: bufA is free once D's last pass has read it
    if (p.sharpen) {
        // ---- D: the part of every line that lies inside the image, in tile coordinates
        const int xlo = max(0, -ex0), xhi = min(ew - 1, I.ow - 1 - ex0), ylo = max(0, -ey0), yhi = min(eh - 1, I.oh - 1 - ey0);
        for (int pass = 0; pass < 3; ++pass) {               // along the rows: Rs -> A -> B -> A
            const unsigned* src = pass == 0 ? Rs : pass == 1 ? bufA : bufB;
            unsigned* dst = pass == 1 ? bufB : bufA;
            for (int idx = t; idx < eh * ew; idx += 256) {
                const int r = idx / ew, e = idx - r * ew;
                dst[idx] = en_box(src + r * ew, 1, e, xlo, xhi, box_r, p.ww, p.fw);
            }
            __syncthreads();
        }
        for (int pass = 0; pass < 3; ++pass) {               // along the columns of the core: A -> B -> A -> B
            const unsigned* src = pass == 1 ? bufB : bufA;
            unsigned* dst = pass == 1 ? bufA : bufB;
            for (int idx = t; idx < eh * tw; idx += 256) {
                const int r = idx / tw, e = hl + idx - r * tw;
                dst[r * ew + e] = en_box(src + e, ew, r, ylo, yhi, box_r, p.ww, p.fw);
            }
            __syncthreads();
        }
        // ---- E
        for (int idx = t; idx < th * tw; idx += 256) {
            const int y = idx / tw, x = idx - y * tw;
            const unsigned in = Rs[(y + hl) * ew + x + hl], bl = bufB[(y + hl) * ew + x + hl];
            unsigned char* o = ob + y * EN_OB_PITCH + 3 * x;
            o[0] = (unsigned char)en_unsharp((int)(in & 255u), (int)(bl & 255u), p.percent, p.threshold);
            o[1] = (unsigned char)en_unsharp((int)((in >> 8) & 255u), (int)((bl >> 8) & 255u), p.percent, p.threshold);
            o[2] = (unsigned char)en_unsharp((int)((in >> 16) & 255u), (int)((bl >> 16) & 255u), p.percent, p.threshold);
        }
    } else {
        for (int idx = t; idx < th * tw; idx += 256) {       // (hl == 0: Rs is the tile itself; C's last readers of hb are behind the barrier)
            const int y = idx / tw, x = idx - y * tw;
            const unsigned in = Rs[idx];
            unsigned char* o = ob + y * EN_OB_PITCH + 3 * x;
            o[0] = (unsigned char)(in & 255u); o[1] = (unsigned char)((in >> 8) & 255u); o[2] = (unsigned char)((in >> 16) & 255u);
        }
    }
    __syncthreads();

    // ---- F: per row the aligned dwords that touch its span of 3 * tw bytes
    constexpr int ROW_DW = EN_OB_PITCH / 4 + 1;
    const int span = 3 * tw;
    for (int idx = t; idx < th * ROW_DW; idx += 256) {
        const int y = idx / ROW_DW, d = idx - y * ROW_DW;
        const long long g0 = I.out0 + ((long long)(oy0 + y) * I.ow + ox0) * 3;
        const long long a = (g0 & ~3LL) + 4 * d;
        if (a >= g0 + span) continue;
        const unsigned char* o = ob + y * EN_OB_PITCH;
        const int k0 = (int)(a - g0);                        // byte of the span the dword starts at (< 0: the span starts inside it)
        if (k0 >= 0 && k0 + 4 <= span && a + 4 <= p.out_bytes) {
            *reinterpret_cast<unsigned*>(p.out + a) = (unsigned)o[k0] | ((unsigned)o[k0 + 1] << 8) | ((unsigned)o[k0 + 2] << 16) | ((unsigned)o[k0 + 3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k0 + j >= 0 && k0 + j < span && a + j < p.out_bytes) p.out[a + j] = o[k0 + j];
        }
    }
}

hipError_t launch_enhance(const EnhanceParams& p, hipStream_t stream) {
    if (!p.frames || ((uintptr_t)p.frames & 3) || !p.img || !p.taps || !p.out || ((uintptr_t)p.out & 3) || p.B <= 0 || p.H <= 0 || p.W <= 0 ||
        p.n <= 0 || p.n_tiles < p.n || p.n_taps <= 0 || p.total_bytes != (long long)p.B * p.H * p.W * 3 || p.out_bytes <= 0 ||
        p.box_r < 0 || p.box_r > ENH_MAX_BOX_R || p.percent < 0 || p.threshold < 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(enhance_kernel, dim3((unsigned)p.n_tiles), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace frp
