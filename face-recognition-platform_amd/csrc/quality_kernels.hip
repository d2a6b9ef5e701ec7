// Face quality on the device: the pixel half of FaceService.assess_face_quality (backend/app/services/face_service.py:276-297 -
// cv2.cvtColor(RGB2GRAY), cv2.Laplacian(CV_64F).var(), np.mean / np.std of the grey crop) for rectangles of the frames that are
// already resident in HBM.  Per rectangle four integer sums leave the device (S1 = sum g, S2 = sum g^2, L1 = sum lap, L2 = sum lap^2);
// the variances and scores are a handful of host operations on them (face_service.py: quality_from_sums).  Integers: the result
// does not depend on the summation order and equals a numpy int64 model bit for bit.
//
//   g   = (R*4899 + G*9617 + B*1868 + 8192) >> 14                      (cv2's fixed-point RGB2GRAY)
//   lap = up + down + left + right - 4*centre on g, BORDER_REFLECT_101 at the edges of the CROP: row -1 is row min(1, h-1), row h is
//         row max(h-2, 0), columns alike (a one-pixel-wide crop reflects onto itself, as np.pad(mode="reflect") does)
//
// face_quality_kernel: one workgroup (4 waves) per QUALITY_TILE_H x QUALITY_TILE_W tile of a crop; a block finds its rectangle by a
// binary search in the per-rectangle prefix of tile counts.
//   A. the bytes of the tile's rows, with one column / row of halo where the crop goes on, are fetched as ALIGNED dwords (a frame row
//      is 3*W bytes and a crop starts at byte 3*left: any byte phase) into LDS, each once;
//   B. grey of every staged pixel, once, to a u8 LDS tile with a one-pixel halo;
//   C. halo columns / rows that lie OUTSIDE the crop are copies of the reflected column / row, which is always among the staged ones
//      (column 1 or w-2 belongs to the same tile as column 0 or w-1, or to its halo);
//   D. each lane takes QUALITY_TILE_H / 4 pixels of one column: 8 terms per 32-bit accumulator, where lap^2 <= 1020^2 = 1,040,400 would
//      allow 4,128 - and the sum of a whole wave (512 terms, <= 5.4e8) still fits, so the wave reduction runs on 32 bits too;
//      the four wave sums are widened to 64 bits, added through LDS and stored to the tile's slot with plain vector stores.
// face_quality_reduce_kernel: one wave per rectangle adds the rectangle's slots.
//
// Bounds: every address read is s + k with s the byte offset of a staged row segment [s, s + nb) that lies inside a validated
// rectangle, rounded DOWN to a dword (>= 0, the base is 4-byte aligned) and k < nb + 3; a dword is loaded whole only if it ends at or
// before total_bytes, else its bytes below total_bytes are read one by one (total_bytes need not be a multiple of 4).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "frp_internal.h"

namespace frp {

#define Q_TH QUALITY_TILE_H
#define Q_TW QUALITY_TILE_W
#define Q_RAW_DW 52      // dwords per staged row: (Q_TW + 2) * 3 = 198 bytes at byte phase 0..3 cover at most 51
#define Q_GP 68          // bytes per row of the grey tile (Q_TW + 2 = 66 used)
static_assert(((Q_TW + 2) * 3 + 3 + 3) / 4 <= Q_RAW_DW && Q_TW + 2 <= Q_GP && Q_TW == 64 && Q_TH % 4 == 0, "tile layout");
static_assert((Q_TH / 4) * 64 * 1040400LL < (1LL << 32), "a wave's sum of lap^2 must fit 32 bits");

__global__ __launch_bounds__(256) void face_quality_kernel(QualityParams p) {
    __shared__ unsigned raw[(Q_TH + 2) * Q_RAW_DW];
    __shared__ unsigned char grey[(Q_TH + 2) * Q_GP];
    __shared__ long long red[4][4];
    const int t = threadIdx.x;
    const int bid = blockIdx.x;
    int lo = 0, hi = p.n;                                    // tile_prefix[lo] <= bid < tile_prefix[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p.tile_prefix[mid] <= bid) lo = mid; else hi = mid;
    }
    const int32_t* rc = p.rects + 5 * lo;
    const int f = rc[0], top = rc[1], left = rc[4];
    const int h = rc[3] - top, w = rc[2] - left;
    const int tiles_x = (w + Q_TW - 1) / Q_TW;
    const int tl = bid - p.tile_prefix[lo];
    const int ty = tl / tiles_x, tx = tl - ty * tiles_x;
    const int y0 = ty * Q_TH, x0 = tx * Q_TW;                // first crop row / column of the tile
    const int r0 = max(y0 - 1, 0), r1 = min(y0 + Q_TH + 1, h);   // crop rows staged: the tile's and its halo, where the crop has them
    const int c0 = max(x0 - 1, 0), c1 = min(x0 + Q_TW + 1, w);
    const int nrows = r1 - r0, ncols = c1 - c0, nb = 3 * ncols;
    const long long seg0 = (((long long)f * p.H + top + r0) * p.W + left + c0) * 3;   // byte offset of the first staged row's segment

    // ---- A: the staged rows' bytes as aligned dwords
    for (int idx = t; idx < nrows * Q_RAW_DW; idx += 256) {
        const int rr = idx / Q_RAW_DW, d = idx - rr * Q_RAW_DW;
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

    // ---- B: grey, once per staged pixel; tile coordinates: row = crop row - (y0 - 1), column = crop column - (x0 - 1)
    const int gr0 = r0 - (y0 - 1), gc0 = c0 - (x0 - 1);
    for (int idx = t; idx < nrows * ncols; idx += 256) {
        const int rr = idx / ncols, cc = idx - rr * ncols;
        const int sh = (int)((seg0 + (long long)rr * p.W * 3) & 3);
        const unsigned char* px = reinterpret_cast<const unsigned char*>(raw + rr * Q_RAW_DW) + sh + 3 * cc;
        const int b0 = px[0], b1 = px[1], b2 = px[2];
        const int R = p.rgb_in ? b0 : b2, B = p.rgb_in ? b2 : b0;
        grey[(gr0 + rr) * Q_GP + gc0 + cc] = (unsigned char)((R * 4899 + b1 * 9617 + B * 1868 + 8192) >> 14);
    }
    __syncthreads();

    // ---- C: halo outside the crop = the reflected column / row.  Columns first, over the staged rows; then rows over all columns, the
    // halo ones included (the corners).  Sources are staged pixels, destinations halo positions: no thread reads what another writes.
    for (int idx = t; idx < 2 * nrows; idx += 256) {
        unsigned char* g = grey + (gr0 + (idx >> 1)) * Q_GP;
        if (!(idx & 1)) {
            if (x0 == 0) g[0] = g[1 + min(1, w - 1)];
        } else if (x0 + Q_TW >= w) {
            g[w - x0 + 1] = g[max(w - 2, 0) - x0 + 1];
        }
    }
    __syncthreads();
    for (int idx = t; idx < 2 * (Q_TW + 2); idx += 256) {
        unsigned char* g = grey + (idx >> 1);
        if (!(idx & 1)) {
            if (y0 == 0) g[0] = g[(1 + min(1, h - 1)) * Q_GP];
        } else if (y0 + Q_TH >= h) {
            g[(h - y0 + 1) * Q_GP] = g[(max(h - 2, 0) - y0 + 1) * Q_GP];
        }
    }
    __syncthreads();

    // ---- D: Q_TH / 4 = 8 pixels of one column per lane
    const int cx = t & 63, ry = (t >> 6) * (Q_TH / 4);
    unsigned s1 = 0u, s2 = 0u, l2 = 0u;
    int l1 = 0;
    if (x0 + cx < w) {
#pragma unroll
        for (int i = 0; i < Q_TH / 4; ++i) {
            const int r = ry + i;
            if (y0 + r < h) {
                const unsigned char* g = grey + (r + 1) * Q_GP + cx + 1;
                const int c = g[0];
                const int lap = (int)g[-Q_GP] + (int)g[Q_GP] + (int)g[-1] + (int)g[1] - 4 * c;
                s1 += (unsigned)c;
                s2 += (unsigned)(c * c);
                l1 += lap;
                l2 += (unsigned)(lap * lap);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_xor(s1, off);
        s2 += __shfl_xor(s2, off);
        l1 += __shfl_xor(l1, off);
        l2 += __shfl_xor(l2, off);
    }
    if ((t & 63) == 0) {
        long long* o = red[t >> 6];
        o[0] = s1; o[1] = s2; o[2] = l1; o[3] = l2;
    }
    __syncthreads();
    if (t < 4) p.partials[4LL * bid + t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
}

__global__ __launch_bounds__(64) void face_quality_reduce_kernel(QualityParams p) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int t0 = p.tile_prefix[r], t1 = p.tile_prefix[r + 1];
    long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int s = t0 + lane; s < t1; s += 64) {
        const long long* q = p.partials + 4LL * s;
        a0 += q[0]; a1 += q[1]; a2 += q[2]; a3 += q[3];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a0 += __shfl_xor(a0, off);
        a1 += __shfl_xor(a1, off);
        a2 += __shfl_xor(a2, off);
        a3 += __shfl_xor(a3, off);
    }
    if (lane < 4) p.sums[4LL * r + lane] = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : a3;
}

hipError_t launch_face_quality(const QualityParams& p, hipStream_t stream) {
    if (!p.frames || ((uintptr_t)p.frames & 3) || !p.rects || !p.tile_prefix || !p.partials || !p.sums || p.B <= 0 || p.H <= 0 || p.W <= 0 ||
        p.n <= 0 || p.n_tiles < p.n || p.total_bytes != (long long)p.B * p.H * p.W * 3)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(face_quality_kernel, dim3((unsigned)p.n_tiles), dim3(256), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(face_quality_reduce_kernel, dim3((unsigned)p.n), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace frp
