// YUV 4:2:0 ingest (frp.h: frp_upload_yuv): 8-bit NV12 / NV21 / I420 / YV12 surfaces, as every video decoder emits them, -> the packed
// BGR frames the pipeline keeps resident.  Exact integer arithmetic, chroma replicated (pixel (x, y) takes the sample at (x >> 1, y >> 1)):
//     y = max(0, Y - yoff) * cy      R = clamp((y + cvr * v + rnd) >> sh)      G = clamp((y - cvg * v - cug * u + rnd) >> sh)
//     B = clamp((y + cub * u + rnd) >> sh)                        with u = U - 128, v = V - 128, >> arithmetic, int32 throughout
// (the three matrices of frp.h are three sets of these constants, ingest_api.cpp: kYuvCoef; libjpeg's full-range rule
// Y + ((c * v + 32768) >> 16) is the same expression with cy = 65536: Y << 16 carries no bits below the shift).
// An HBM-bound pass: 1.5 bytes read and 3 written per pixel.  A thread takes two rows, so every chroma sample is loaded once.
//   fast path     16 pixels x 2 rows per thread: a 16-byte load per luma row, chroma as one 16-byte load (semi-planar) or two 8-byte loads
//                 (planar), three 16-byte stores per row.  Needs W % 16 == 0 and every plane address and pitch aligned to its load
//                 (16 bytes; 8 for planar chroma); the resident rows are packed at W * 3, a multiple of 48, so the stores are aligned too.
//   general path  2 pixels x 2 rows per thread (one chroma sample), byte accesses: any even size, any pitch, any alignment.
// The host picks one path per launch (launch_yuv_to_bgr's caller: ingest_api.cpp).  Planes are found through a per-frame table of device
// addresses, so frames may lie anywhere - the caller's decoder surfaces or the packed staging copy of host planes.  Byte offsets are
// 64-bit (32 frames of 4K are more than 2^31 bytes of output); the index inside one frame is 32-bit (the host bounds W * H).
#include "frp_internal.h"

namespace frp {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));      // native vectors: one _dwordx4 / _dwordx2 access each
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));      // (HIP's uint4 is a struct: its stores came out as 12-byte pieces)
// The plane addresses come out of the table, where the compiler cannot see that they are global memory: said here, the loads are
// global_load_* and not flat_load_*.
template <class T>
__device__ __forceinline__ T load_global(const uint8_t* p) { return *(const __attribute__((address_space(1))) T*)(uintptr_t)p; }
struct Chroma { int r, g, b; };     // the chroma terms of R, G, B with the rounding constant folded in: shared by the 2 x 2 pixels of a sample

__device__ __forceinline__ Chroma yuv_chroma(const YuvCoef& k, int U, int V) {
    const int u = U - 128, v = V - 128;
    return {k.cvr * v + k.rnd, -k.cvg * v - k.cug * u + k.rnd, k.cub * u + k.rnd};
}
// clamp((x) >> sh) to 0 .. 255, with the clamp applied BEFORE the shift: x into 0 .. (256 << sh) - 1, then a shift of a non-negative number -
// the same value for every x.  Written shift-then-clamp, hipcc fuses two neighbouring channels into one v_ashr_pk_u8_i32 (gfx950: shift,
// saturate, pack two bytes) and ORs the further bytes of the word on top, but the instruction leaves the upper half of its destination
// as it was: bytes 2 and 3 of such a word came out OR-ed with stale bits on the device (every pixel at x % 4 == 2 of the fast path).
__device__ __forceinline__ uint32_t shift_clamp8(int x, int sh) { return (uint32_t)min(max(x, 0), (256 << sh) - 1) >> sh; }
// -> B | G << 8 | R << 16
__device__ __forceinline__ uint32_t yuv_pixel(const YuvCoef& k, int Y, const Chroma& c) {
    const int y = max(0, Y - k.yoff) * k.cy;
    return shift_clamp8(y + c.b, k.sh) | shift_clamp8(y + c.g, k.sh) << 8 | shift_clamp8(y + c.r, k.sh) << 16;
}

template <bool SEMI>
__global__ __launch_bounds__(256) void yuv_fast_kernel(YuvParams p) {
    const uint32_t strips = (uint32_t)p.W >> 4;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t ry = t / strips, sx = t - ry * strips;          // row pair, 16-pixel strip
    if (ry >= ((uint32_t)p.H >> 1)) return;
    const uint32_t b = blockIdx.y;
    const uint8_t* const* planes = p.tab + 3 * (size_t)b;
    const uint8_t* yp = planes[0] + (int64_t)(2 * ry) * p.y_pitch + 16 * sx;
    u32x4 yw[2];
    yw[0] = load_global<u32x4>(yp);
    yw[1] = load_global<u32x4>(yp + p.y_pitch);
    Chroma c[8];
    if (SEMI) {
        const u32x4 q = load_global<u32x4>(planes[1] + (int64_t)ry * p.c_pitch + 16 * sx);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t pair = (w[i >> 1] >> (16 * (i & 1))) & 0xffffu;      // first byte in the low half
            c[i] = yuv_chroma(p.k, (int)((pair >> p.ush) & 255u), (int)((pair >> (8 - p.ush)) & 255u));
        }
    } else {
        const int64_t co = (int64_t)ry * p.c_pitch + 8 * sx;
        const u32x2 qu = load_global<u32x2>(planes[1] + co), qv = load_global<u32x2>(planes[2] + co);
        const uint32_t wu[2] = {qu.x, qu.y}, wv[2] = {qv.x, qv.y};
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = yuv_chroma(p.k, (int)((wu[i >> 2] >> (8 * (i & 3))) & 255u), (int)((wv[i >> 2] >> (8 * (i & 3))) & 255u));
    }
    uint8_t* out = p.frames + (((int64_t)b * p.H + 2 * ry) * p.W + 16 * sx) * 3;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t w[4] = {yw[r].x, yw[r].y, yw[r].z, yw[r].w};
        uint32_t o[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) o[j] = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t px = yuv_pixel(p.k, (int)((w[i >> 2] >> (8 * (i & 3))) & 255u), c[i >> 1]);
            const int at = 3 * i, word = at >> 2, sh = 8 * (at & 3);       // 3 bytes at byte `at` of the 48: they may straddle two words
            o[word] |= px << sh;
            if (sh > 8) o[word + 1] |= px >> (32 - sh);
        }
        u32x4* dst = (u32x4*)(out + (int64_t)r * p.W * 3);
        dst[0] = u32x4{o[0], o[1], o[2], o[3]};
        dst[1] = u32x4{o[4], o[5], o[6], o[7]};
        dst[2] = u32x4{o[8], o[9], o[10], o[11]};
    }
}

template <bool SEMI>
__global__ __launch_bounds__(256) void yuv_general_kernel(YuvParams p) {
    const uint32_t cw = (uint32_t)p.W >> 1;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t cy = t / cw, cx = t - cy * cw;                  // the chroma sample = the 2 x 2 pixels of this thread
    if (cy >= ((uint32_t)p.H >> 1)) return;
    const uint32_t b = blockIdx.y;
    const uint8_t* const* planes = p.tab + 3 * (size_t)b;
    int U, V;
    if (SEMI) {
        const uint8_t* q = planes[1] + (int64_t)cy * p.c_pitch + 2 * cx;
        U = load_global<uint8_t>(q + (p.ush >> 3));
        V = load_global<uint8_t>(q + 1 - (p.ush >> 3));
    } else {
        const int64_t co = (int64_t)cy * p.c_pitch + cx;
        U = load_global<uint8_t>(planes[1] + co);
        V = load_global<uint8_t>(planes[2] + co);
    }
    const Chroma c = yuv_chroma(p.k, U, V);
    const uint8_t* yp = planes[0] + (int64_t)(2 * cy) * p.y_pitch + 2 * cx;
    uint8_t* out = p.frames + (((int64_t)b * p.H + 2 * cy) * p.W + 2 * cx) * 3;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t px = yuv_pixel(p.k, load_global<uint8_t>(yp + (int64_t)r * p.y_pitch + i), c);
            uint8_t* d = out + (int64_t)r * p.W * 3 + 3 * i;
            d[0] = (uint8_t)px;
            d[1] = (uint8_t)(px >> 8);
            d[2] = (uint8_t)(px >> 16);
        }
    }
}

}  // namespace

// p.tab: [B][3] device addresses Y, U (or the interleaved plane), V; `fast`: the caller has checked the fast path's conditions (above)
hipError_t launch_yuv_to_bgr(const YuvParams& p, bool semi_planar, bool fast, hipStream_t stream) {
    const uint64_t per_frame = fast ? (uint64_t)(p.W >> 4) * (uint64_t)(p.H >> 1) : (uint64_t)(p.W >> 1) * (uint64_t)(p.H >> 1);
    if (p.B <= 0 || p.B > 65535 || per_frame == 0 || per_frame > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((per_frame + 255) / 256), (unsigned)p.B), block(256);
    if (fast) {
        if (semi_planar) hipLaunchKernelGGL(yuv_fast_kernel<true>, grid, block, 0, stream, p);
        else hipLaunchKernelGGL(yuv_fast_kernel<false>, grid, block, 0, stream, p);
    } else {
        if (semi_planar) hipLaunchKernelGGL(yuv_general_kernel<true>, grid, block, 0, stream, p);
        else hipLaunchKernelGGL(yuv_general_kernel<false>, grid, block, 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace frp
