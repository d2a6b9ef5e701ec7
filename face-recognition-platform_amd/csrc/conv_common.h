// Device helpers shared by the MFMA convolution kernels, and the host side of their launch (conv_launch: every family's launcher ends there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "frp_internal.h"

namespace frp {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

#define CONV_NS 3            // LDS ring stages
#define CONV_OOB 0x80000000u // buffer offset beyond any tensor (< 2 GiB each): reads as zero

__device__ __forceinline__ int lds_off(int row, int chunk) {
    return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

// one LDS-DMA piece: 64 lanes x 16 B from per-lane buffer offsets to lds_base + lane*16.
// (kept in a __device__ function: the builtin does not exist for the host pass)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned char* lds_base, unsigned voffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_base, 16, voffset, 0, 0, 0);
}

// ... with a scalar byte offset added to the source address (not part of the range check)
__device__ __forceinline__ void dma16s(__amdgpu_buffer_rsrc_t rsrc, unsigned char* lds_base, unsigned voffset, int soffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_base, 16, voffset, soffset, 0, 0);
}
// raw buffer descriptor of `bytes` bytes at ptr (stride 0; the flags word: 32-bit data format, offsets >= bytes read as zero)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t conv_rsrc(const void* ptr, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), 0, bytes, 0x00020000);
}

// (device-only constructs must live in __device__ functions: written directly in the __global__
// template body they make the HOST pass drop the kernel stub without a diagnostic)
__device__ __forceinline__ void keep_alive(floatx16 v) { asm volatile("" ::"v"(v)); }
// Half-wave exchange: lane<32 ends up with this pixel's couts [lo | upper lane's lo] (16 contiguous
// bytes), lane>=32 with [lower lane's hi | hi]: two 8-byte stores per lane become one 16-byte store
// (the epilogue store tail is issue-bound, not bandwidth-bound).
__device__ __forceinline__ void swap_halves(unsigned& a, unsigned& b) {
    auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0];
    b = r[1];
}
// diagnostic stamps (conv_bench only, p.stamps != null): 100 MHz wall clock per workgroup phase,
// written to a buffer nothing else reads.  Lab build only: the shipped kernels carry neither the tests of the stamp pointer nor
// the ~12 scalar registers they keep spilled (-0.3 % of a step; the lab library's kernels are otherwise the shipped ones).
__device__ __forceinline__ void stamp(unsigned long long* buf, int slot) {
#ifndef FRP_LAB
    (void)buf; (void)slot;
    return;
#endif
    if (buf && threadIdx.x == 0) buf[(long)blockIdx.x * 8 + slot] = __builtin_amdgcn_s_memrealtime();
}
// keeps hipcc from hoisting the loads of every epilogue slice above the first one (which
// would need several hundred live registers)
__device__ __forceinline__ void sched_fence() { __builtin_amdgcn_sched_barrier(0); }

static int device_cu_count(int dev) {
    static int n_cu[64] = {};
    if (!n_cu[dev]) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
        n_cu[dev] = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return n_cu[dev];
}
// the device the calling thread launches on, and its CU count
static inline hipError_t conv_device(int* dev, int* ncu) {
    if (hipGetDevice(dev) != hipSuccess || *dev < 0 || *dev >= 64) return hipErrorInvalidDevice;
    *ncu = device_cu_count(*dev);
    return *ncu > 0 ? hipSuccess : hipErrorInvalidDevice;
}

// Small-M rule shared by the conv launchers: quarter tiles (128 pixels x 64 couts, two workgroups per CU) when the default
// tiling would leave at least half of the CUs without a tile - small pyramid scales, a handful of faces, single images.
// With the image count on the device (n_dev) the decision - like the grid - goes by the capacity.  Same k order: bit-identical
// to the default tiles of the same kernel family.
static inline bool conv_small_m(const ConvParams& p, long default_tiles, int ncu) {
    if (p.small_m < 0 || p.ksplit != 1 || p.out2 || (p.flags & (FRP_FLAG_F8 | FRP_FLAG_OUT_FP8 | FRP_FLAG_OUT_F32))) return false;
    if (p.small_m > 0) return true;
    return ncu > 0 && default_tiles * 2 <= ncu;
}

// Weight prefetch of a quarter-tile launch (ConvParams::pf_ptr): workgroup k of the n_pf extra ones (k = blockIdx - workers; round-robin
// dispatch puts workgroup b on XCD b % 8) pulls its share of the next launch's weights through the L2 of ITS XCD - every XCD reads the
// whole region, in n_pf / 8 slices.  Read-only, results unused: nothing to synchronise with.
#define CONV_PF_WGS 64
__device__ __forceinline__ void conv_prefetch_weights(const ConvParams& p, int k, int n_pf, int nthreads) {
    const int per_xcd = n_pf >> 3;
    if (per_xcd <= 0 || !p.pf_ptr) return;
    const int q = k >> 3;                                            // slice index within this XCD's workgroups
    // at most 3 MiB (an XCD's L2 holds 4): the head of a larger tensor (stage 4's 4.7 MB; the FC's 25.7 MB would only evict itself)
    const unsigned n16 = (p.pf_bytes < (3u << 20) ? p.pf_bytes : (3u << 20)) >> 4;
    const unsigned lo = (unsigned)((unsigned long long)n16 * q / per_xcd), hi = (unsigned)((unsigned long long)n16 * (q + 1) / per_xcd);
    const uint4* src = reinterpret_cast<const uint4*>(p.pf_ptr);
    unsigned acc = 0;
    for (unsigned i = lo + threadIdx.x; i < hi; i += nthreads) {
        const uint4 v = src[i];
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x9e3779b9u && p.stamps) p.stamps[0] = acc;          // (keeps the loads; never true in practice, harmless if it is)
}
// The grid of the two direct families (the generic and the lean kernel; QUARTER: their 128-pixel tiles, two workgroups per CU).
template <bool QUARTER>
static void conv_direct_grid(ConvParams& p, unsigned& grid, long slots) {
    p.n_workers = 0;
    // a launch of at most 128 tiles (a call of up to ~20 faces: where the latency of ONE call is what counts) leaves three quarters
    // of the slots empty: 64 more workgroups warm the L2s for the next launch.  Larger quarter-tile launches (config 4's ~36 faces
    // on two lanes) keep their spare CUs for the other lane's kernels: there the prefetchers cost 4 % of the throughput.
    if (QUARTER && p.pf_ptr && p.pf_bytes >= 4096 && grid <= 128 && (long)grid + CONV_PF_WGS <= slots) {
        p.n_workers = (int)grid;
        grid += CONV_PF_WGS;
    }
    if (grid > 256) p.stamps = nullptr;                                // (the diagnostic stamp buffer holds 256 workgroups)
}

// The launch of every conv kernel family: a persistent grid of `per_cu` workgroups per CU, or one per tile where there are fewer.
// Kern's dynamic LDS limit is raised to lds_attr once per device (per instantiation, so per kernel: whenever a launch needs more
// than was asked for so far - the Winograd launchers ask for the 160 KiB of a CU at once, the others for their one size);
// `grid_rule` (conv_direct_grid) may add workgroups and edit the parameters once the grid is known.
template <auto Kern>
static hipError_t conv_launch(int lds_attr, int lds, long ntiles, int per_cu, int block, ConvParams& p, hipStream_t stream,
                              void (*grid_rule)(ConvParams&, unsigned&, long) = nullptr) {
    static int attr_lds[64] = {};
    int dev = 0, ncu = 0;
    hipError_t e = conv_device(&dev, &ncu);
    if (e != hipSuccess) return e;
    if (attr_lds[dev] < lds) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_attr);
        if (e != hipSuccess) return e;
        attr_lds[dev] = lds_attr;
    }
    if (ntiles <= 0 || ntiles > 0x7fffffffL) return hipErrorInvalidValue;
    const long slots = (long)ncu * per_cu;
    unsigned grid = (unsigned)(ntiles < slots ? ntiles : slots);
    if (grid_rule) grid_rule(p, grid, slots);
    hipLaunchKernelGGL(Kern, dim3(grid), dim3(block), lds, stream, p);
    return hipGetLastError();
}

// q = m / d, r = m % d for 0 <= m < 2^24 via a float reciprocal and one correction step
// (an integer division costs ~40 instructions; the prologue needs two per pixel row)
__device__ __forceinline__ void fast_divmod(int m, int d, float inv_d, int& q, int& r) {
    q = (int)((float)m * inv_d);
    r = m - q * d;
    if (r < 0) { --q; r += d; }
    if (r >= d) { ++q; r -= d; }
}

// ---------------------------------------------------------------------------------------------------------------
// The frame of the persistent conv kernels: which tiles a workgroup computes, how many images exist, which taps of a pixel
// lie inside the image, and the per-tile epilogue parameters in LDS.  tests/test_conv_frame_host.py holds the first three on the host.

// Tile walk of workgroup b of the G that walk a list of n_tiles tiles: t0, t0 + tstep, ... < t1 (nothing when t0 >= t1).
// Workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share an L2).  XCD x takes the contiguous chunk
// [x*T/8, (x+1)*T/8) of the tile list and its G/8 workgroups walk it INTERLEAVED (workgroup j: chunk + j, + j + G/8, ...): at any
// moment the workgroups of one L2 work on G/8 consecutive tiles - a band of neighbouring image rows whose row patches are the same
// lines, both cout tiles of a pixel tile, the k-slices of one split-K tile - fetched once per L2 instead of once per workgroup
// several tiles apart.  Grids that are no multiple of 8 (fewer tiles than CUs) take contiguous ranges.
struct TileWalk { int t0, t1, tstep; };
__host__ __device__ __forceinline__ TileWalk conv_tile_walk(int n_tiles, int G, unsigned b) {
    if ((G & 7) == 0) {
        const int x = b & 7, j = b >> 3, per = G >> 3;
        const int cs = (int)((long)x * n_tiles / 8), ce = (int)((long)(x + 1) * n_tiles / 8);
        return {cs + j, ce, per};
    }
    return {(int)((long)b * n_tiles / G), (int)((long)(b + 1) * n_tiles / G), 1};
}

// Images that really exist when the count is known on the device only (threshold mode): the value read from ConvParams::n_dev,
// held inside the capacity N the buffers and the grid were sized for.
__host__ __device__ __forceinline__ int conv_image_count(int n_dev, int N) { return n_dev < 0 ? 0 : (n_dev > N ? N : n_dev); }

// 9-bit tap mask of output pixel (oy, ox): bit kh*3+kw set <=> tap (kh, kw) of its window lies inside the H x W input
// (KS = 1: the one tap is bit 0).  The reference form, which no kernel calls: conv_mfma.hip spells it out itself (see there); the host
// test checks this function and conv_tap_mask_s1, not the kernels' copies.
__host__ __device__ __forceinline__ unsigned conv_tap_mask(int oy, int ox, int H, int W, int stride, int pad, int KS) {
    const int y0 = oy * stride - pad, x0 = ox * stride - pad;
    unsigned ym = 0, xm = 0, mask = 0;      // 3-bit validity of y0+{0,1,2}, x0+{0,1,2}
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        ym |= ((unsigned)(y0 + d) < (unsigned)H ? 1u : 0u) << d;
        xm |= ((unsigned)(x0 + d) < (unsigned)W ? 1u : 0u) << d;
    }
    if (KS == 1) { ym &= 1u; xm &= 1u; }
#pragma unroll
    for (int d = 0; d < 3; ++d) mask |= ((ym >> d) & 1u) ? (xm << (3 * d)) : 0u;
    return mask;
}
// ... of a 3x3 stride-1 pad-1 window (the row-patch kernels): the centre row and column always exist
__host__ __device__ __forceinline__ unsigned conv_tap_mask_s1(int oy, int ox, int H, int W) {
    const unsigned ym = (oy > 0 ? 1u : 0u) | 2u | (oy < H - 1 ? 4u : 0u);
    const unsigned xm = (ox > 0 ? 1u : 0u) | 2u | (ox < W - 1 ? 4u : 0u);
    unsigned mask = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) mask |= ((ym >> d) & 1u) ? (xm << (3 * d)) : 0u;
    return mask;
}

// Per-tile epilogue parameters in LDS (behind the operand rings): bias (1 or 9 border classes, class-major [9][TC]), PReLU slope
// [TC] and - F8 - weight scale x input scale [TC] of the tile's TC couts from c0.  A kernel fetches them into registers at the
// start of the tile's first k-step and stores them at its end, so the epilogue reads them with short LDS latencies instead of
// serialising on global loads.  t: the thread's index among the workgroup's THREADS; border: FRP_FLAG_BORDER_BIAS of the launch.
// (conv_mfma.hip spells the same two steps out itself: tests/test_kernel_resources_host.py, see there.)
template <int TC, int THREADS, bool F8>
struct EpiParamCache {
    static constexpr int PPT = (9 * TC + THREADS - 1) / THREADS;   // bias values per thread
    float pb[PPT], ps = 0.f, pw = 0.f;
    __device__ __forceinline__ void fetch(const ConvParams& p, int c0, int t, bool border) {
        const int nb = (border ? 9 : 1) * TC;
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int idx = t + q * THREADS;
            const int cls = idx / TC, co = c0 + (idx - cls * TC);
            pb[q] = (idx < nb && co < p.Cout) ? p.bias[(long)cls * p.Cout + co] : 0.f;
        }
        if (p.act == FRP_ACT_PRELU && t < TC) ps = (c0 + t < p.Cout) ? p.slope[c0 + t] : 0.f;
        if (F8 && t < TC) pw = (c0 + t < p.Cout) ? p.wscale[c0 + t] * p.in_scale : 0.f;
    }
    __device__ __forceinline__ void store(float* lds_bias, float* lds_slope, float* lds_wscale, int t) const {
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int idx = t + q * THREADS;
            if (idx < 9 * TC) lds_bias[idx] = pb[q];
        }
        if (t < TC) lds_slope[t] = ps;
        if (F8 && t < TC) lds_wscale[t] = pw;
    }
};

// ---------------------------------------------------------------------------------------------------------------
// THE epilogue arithmetic of every conv / stem kernel: one lane's share of one 32-pixel x 32-cout accumulator block
// (layout of v_mfma_f32_32x32x16: lane = pixel fr of the block, registers 4g..4g+3 = couts 8g + 4*fh .. +3).  Bit-identity
// between the kernel families rests on these being the only definition: accumulator (x weight scale) + bias, + residual,
// ReLU / PReLU in fp32, ONE conversion to fp16 (or fp8), then the half-wave exchange into store chunks.  Stores, addresses,
// range checks and ablation switches stay with the kernels; so does the ORDER in which a kernel calls the pieces (all four
// groups' values before any conversion, or group by group): the register allocation follows it.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// border class 0..8 of output pixel (oy, ox): row of the 9-class bias table (FRP_FLAG_BORDER_BIAS)
__device__ __forceinline__ int epi_border_class(int oy, int ox, int Ho, int Wo) {
    return ((oy == 0) ? 0 : (oy == Ho - 1) ? 2 : 1) * 3 + ((ox == 0) ? 0 : (ox == Wo - 1) ? 2 : 1);
}

// residual: one 16-byte chunk in the STORE layout (couts 16q + 8*fh .. +7 of this lane's pixel; from a global load, a buffer
// load or LDS) -> groups 2q, 2q + 1 in the accumulator layout: the same half-wave exchange as for the stores (it is its own inverse)
__device__ __forceinline__ void epi_residual(u32x4 c, half4& g0, half4& g1) {
    unsigned x = c.x, y = c.y, z = c.z, w = c.w;
    swap_halves(x, z);
    swap_halves(y, w);
    union { unsigned u[2]; half4 h; } lo, hi;
    lo.u[0] = x; lo.u[1] = y; hi.u[0] = z; hi.u[1] = w;
    g0 = lo.h;
    g1 = hi.h;
}
__device__ __forceinline__ void epi_residual(const uint4& c, half4& g0, half4& g1) { epi_residual(u32x4{c.x, c.y, c.z, c.w}, g0, g1); }

// value of group g, written to v[o .. o+3].  V = floatx4 (o = 0) where a kernel converts group by group; V = floatx16 (o = 4g: the
// accumulator layout) where it finishes a block's four groups first - the other choice costs either kind of kernel registers
// (tests/test_kernel_resources_host.py).  bias / slope / wscale: rows of the LDS parameter cache (or registers of the caller), read
// at [cl .. cl+3], the group's couts - the slope only under PReLU.
//   ACT: FRP_ACT_* or -1 = run-time `act`;  RES: 0 / 1 or -1 = run-time `has_res`;  WS: the accumulator is first multiplied by wscale
template <int ACT, int RES, bool WS = false, typename V>
__device__ __forceinline__ void epi_value(V& v, int o, const floatx16& acc, int g, const float* bias, const float* slope, int cl,
                                          half4 res = half4{}, int act_rt = FRP_ACT_NONE, bool res_rt = false, const float* wscale = nullptr) {
    const int act = ACT < 0 ? act_rt : ACT;
    const bool has_res = RES < 0 ? res_rt : RES != 0;
    const floatx4 b4 = *reinterpret_cast<const floatx4*>(bias + cl);
    if constexpr (WS) {
        const floatx4 w4 = *reinterpret_cast<const floatx4*>(wscale + cl);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[o + e] = acc[4 * g + e] * w4[e] + b4[e];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[o + e] = acc[4 * g + e] + b4[e];
    }
    if (has_res) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[o + e] += (float)res[e];
    }
    if (act == FRP_ACT_RELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[o + e] = fmaxf(v[o + e], 0.f);
    } else if (act == FRP_ACT_PRELU) {
        const floatx4 s4 = *reinterpret_cast<const floatx4*>(slope + cl);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[o + e] = v[o + e] > 0.f ? v[o + e] : v[o + e] * s4[e];
    }
}
__device__ __forceinline__ floatx4 epi_group(const floatx16& v, int g) { return floatx4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]}; }

// pack: the one conversion to fp16 (of v[o .. o+3]) ...
template <typename V>
__device__ __forceinline__ half4 epi_half4(const V& v, int o = 0) {
    half4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = (_Float16)v[o + e];
    return h;
}
// ... and the half-wave exchange of groups 2q, 2q + 1 (as packed dwords) into the lane's store chunk q: couts 16q + 8*fh .. +7
__device__ __forceinline__ u32x4 epi_chunk(const unsigned (&a)[2], const unsigned (&b)[2]) {
    unsigned a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
    swap_halves(a0, b0);
    swap_halves(a1, b1);
    return u32x4{a0, a1, b0, b1};
}
__device__ __forceinline__ u32x4 epi_chunk(half4 a, half4 b) {
    union { half4 h; unsigned u[2]; } x, y;
    x.h = a;
    y.h = b;
    return epi_chunk(x.u, y.u);
}
// the fp8 sibling (OCP E4M3: value / out_scale, clamped to +-448): a lane packs its 4-cout runs into dwords, exchanges half-waves
// like the fp16 path and stores 8 consecutive couts (8 bytes) per (32-cout block, half)
__device__ __forceinline__ int pack_fp8x4(const floatx16& v, int o, float inv_scale) {
    float a[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = fminf(fmaxf(v[o + e] * inv_scale, -448.f), 448.f);
    int d = __builtin_amdgcn_cvt_pk_fp8_f32(a[0], a[1], 0, false);
    return __builtin_amdgcn_cvt_pk_fp8_f32(a[2], a[3], d, true);
}
// (in place: afterwards (a, b) is the lane's chunk q)
__device__ __forceinline__ void epi_chunk8(unsigned& a, unsigned& b) { swap_halves(a, b); }

// ---------------------------------------------------------------------------------------------------------------
// Tile epilogue of the tiled kernels (generic, row-patch, Winograd): the pixel loop around the pieces above - bias / 9-class
// border bias from the LDS parameter cache, residual, activation, then fp16 (16-byte stores) or fp32 output.
//
// FULL tiles (the common case) run a copy specialised at compile time on (activation, residual): with the flags
// as run-time values the compiler kept ~70 uniform branches and ~90 s_nops in every epilogue (it does not unswitch
// a body this large), a quarter of its instructions.  Ragged tiles and fp32 output take the generic copy.
//   ACT: FRP_ACT_* or -1 = run-time p.act;  RES: 0 / 1 or -1 = run-time.
template <int MP, int MC, int TC, bool FULL, int ACT, int RES, bool OVER = false>
__device__ __forceinline__ void conv_epilogue_body(const ConvParams& p, floatx16 (&acc)[MP][MC], const uint4 (&rres)[MP][MC][2],
                                                   const float* lds_bias, const float* lds_slope, int m0, int c0, int prow0,
                                                   int crow0, int fr, int fh, int HoWo, float inv_howo, float inv_wo,
                                                   int ps = 1, int po = 0, int m_over = 0) {
    // (ps, po): lane row r of the tile holds output pixel m0 + r * ps + po: (1, 0) in the direct kernels, (2, parity) in
    // the Winograd kernel, whose lanes own pixel PAIRS (conv3x3_wino.hip).  OVER (MP = 1; the Winograd kernel's 2-D tiles):
    // the lane's pixel is m_over + po instead, and does not exist when m_over < 0.
    const bool border = p.flags & FRP_FLAG_BORDER_BIAS;
    const bool out32 = (ACT < 0) && (p.flags & FRP_FLAG_OUT_F32);
    const bool has_res = RES < 0 ? p.res != nullptr : RES != 0;
    half4 r4[MP][MC][4];
    bool mok[MP];
    long obase[MP];
    int cls[MP];
#pragma unroll
    for (int i = 0; i < MP; ++i) {
        const int mraw = OVER ? (m_over >= 0 ? m_over + po : p.M) : m0 + (prow0 + i * 32 + fr) * ps + po;
        mok[i] = FULL || mraw < p.M;
        const int m = mok[i] ? mraw : 0;
        cls[i] = 0;
        if (border) {
            int n, rem, oy, ox;
            fast_divmod(m, HoWo, inv_howo, n, rem);
            fast_divmod(rem, p.Wo, inv_wo, oy, ox);
            cls[i] = epi_border_class(oy, ox, p.Ho, p.Wo);
        }
        obase[i] = (long)m * p.Cout;
        if (has_res) {
#pragma unroll
            for (int j = 0; j < MC; ++j)
#pragma unroll
                for (int q = 0; q < 2; ++q) epi_residual(rres[i][j][q], r4[i][j][2 * q], r4[i][j][2 * q + 1]);
        }
    }
#pragma unroll
    for (int i = 0; i < MP; ++i) {
#pragma unroll
        for (int j = 0; j < MC; ++j) {
            floatx16 v;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                epi_value<ACT, RES>(v, 4 * g, acc[i][j], g, lds_bias + cls[i] * TC, lds_slope, crow0 + j * 32 + 8 * g + 4 * fh, r4[i][j][g], p.act, has_res);
            if (out32) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = c0 + crow0 + j * 32 + 8 * g + 4 * fh;
                    if (FULL || (mok[i] && co < p.Cout))
                        *reinterpret_cast<floatx4*>(reinterpret_cast<float*>(p.out) + obase[i] + co) = epi_group(v, g);
                }
            } else {
                half4 h[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) h[g] = epi_half4(v, 4 * g);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const u32x4 o = epi_chunk(h[2 * q], h[2 * q + 1]);
                    const int co = c0 + crow0 + j * 32 + 16 * q + 8 * fh;   // 8 consecutive couts
                    if (FULL || (mok[i] && co < p.Cout)) *reinterpret_cast<u32x4*>(reinterpret_cast<_Float16*>(p.out) + obase[i] + co) = o;
                }
            }
        }
    }
}

template <int MP, int MC, int TC>
__device__ __forceinline__ void conv_epilogue(const ConvParams& p, floatx16 (&acc)[MP][MC], const uint4 (&rres)[MP][MC][2],
                                              const float* lds_bias, const float* lds_slope, int m0, int c0, int TP, int prow0,
                                              int crow0, int fr, int fh, int HoWo, float inv_howo, float inv_wo,
                                              int ps = 1, int po = 0) {
#define FRP_EPI(FULL_, ACT_, RES_) \
    conv_epilogue_body<MP, MC, TC, FULL_, ACT_, RES_>(p, acc, rres, lds_bias, lds_slope, m0, c0, prow0, crow0, fr, fh, HoWo, inv_howo, inv_wo, ps, po)
    const bool full = m0 + TP <= p.M && c0 + TC <= p.Cout;
    if (!full) { FRP_EPI(false, -1, -1); return; }
    if (p.flags & FRP_FLAG_OUT_F32) { FRP_EPI(true, -1, -1); return; }
    const bool has_res = p.res != nullptr;
    if (p.act == FRP_ACT_PRELU) { if (has_res) FRP_EPI(true, FRP_ACT_PRELU, 1); else FRP_EPI(true, FRP_ACT_PRELU, 0); }
    else if (p.act == FRP_ACT_RELU) { if (has_res) FRP_EPI(true, FRP_ACT_RELU, 1); else FRP_EPI(true, FRP_ACT_RELU, 0); }
    else { if (has_res) FRP_EPI(true, FRP_ACT_NONE, 1); else FRP_EPI(true, FRP_ACT_NONE, 0); }
#undef FRP_EPI
}

// ---------------------------------------------------------------------------------------------------------------
// Epilogue with fp8 outputs (BASELINE config 5).  WS: the accumulator is first multiplied by lds_wscale[cout] (fp8
// weights x fp8 input: per-cout weight scale x input-tensor scale).  Outputs: fp16 to p.out unless FRP_FLAG_OUT_FP8;
// OCP E4M3 bytes to p.out when FRP_FLAG_OUT_FP8, else to p.out2 when set.
template <int MP, int MC, int TC, bool FULL, int ACT, int RES, bool WS>
__device__ __forceinline__ void conv_epilogue8_body(const ConvParams& p, floatx16 (&acc)[MP][MC], const uint4 (&rres)[MP][MC][2],
                                                    const float* lds_bias, const float* lds_slope, const float* lds_wscale, int m0,
                                                    int c0, int prow0, int crow0, int fr, int fh, int HoWo, float inv_howo, float inv_wo) {
    const bool border = p.flags & FRP_FLAG_BORDER_BIAS;
    const bool out8 = p.flags & FRP_FLAG_OUT_FP8;
    unsigned char* dst8 = reinterpret_cast<unsigned char*>(out8 ? p.out : p.out2);
    const float inv_os = 1.0f / p.out_scale;
    const bool has_res = RES < 0 ? p.res != nullptr : RES != 0;
#pragma unroll
    for (int i = 0; i < MP; ++i) {
        const int mraw = m0 + prow0 + i * 32 + fr;
        const bool mok = FULL || mraw < p.M;
        const int m = mok ? mraw : 0;
        int cls = 0;
        if (border) {
            int n, rem, oy, ox;
            fast_divmod(m, HoWo, inv_howo, n, rem);
            fast_divmod(rem, p.Wo, inv_wo, oy, ox);
            cls = epi_border_class(oy, ox, p.Ho, p.Wo);
        }
        const long obase = (long)m * p.Cout;
#pragma unroll
        for (int j = 0; j < MC; ++j) {
            half4 r4[4];
            if (has_res) {
#pragma unroll
                for (int q = 0; q < 2; ++q) epi_residual(rres[i][j][q], r4[2 * q], r4[2 * q + 1]);
            }
            floatx16 v;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                epi_value<ACT, RES, WS>(v, 4 * g, acc[i][j], g, lds_bias + cls * TC, lds_slope, crow0 + j * 32 + 8 * g + 4 * fh, r4[g], p.act, has_res, lds_wscale);
            if (!out8) {                      // fp16 primary output
                half4 h[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) h[g] = epi_half4(v, 4 * g);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const u32x4 o = epi_chunk(h[2 * q], h[2 * q + 1]);
                    const int co = c0 + crow0 + j * 32 + 16 * q + 8 * fh;
                    if (FULL || (mok && co < p.Cout)) *reinterpret_cast<u32x4*>(reinterpret_cast<_Float16*>(p.out) + obase + co) = o;
                }
            }
            if (dst8) {                       // fp8 output (primary or copy)
                unsigned d[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) d[g] = (unsigned)pack_fp8x4(v, 4 * g, inv_os);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    epi_chunk8(d[2 * q], d[2 * q + 1]);         // -> couts 16q + 8fh .. +7 of this pixel
                    const int co = c0 + crow0 + j * 32 + 16 * q + 8 * fh;
                    if (FULL || (mok && co < p.Cout)) *reinterpret_cast<uint2*>(dst8 + obase + co) = make_uint2(d[2 * q], d[2 * q + 1]);
                }
            }
        }
    }
}

template <int MP, int MC, int TC, bool WS>
__device__ __forceinline__ void conv_epilogue8(const ConvParams& p, floatx16 (&acc)[MP][MC], const uint4 (&rres)[MP][MC][2],
                                               const float* lds_bias, const float* lds_slope, const float* lds_wscale, int m0, int c0,
                                               int TP, int prow0, int crow0, int fr, int fh, int HoWo, float inv_howo, float inv_wo) {
#define FRP_EPI8(FULL_, ACT_, RES_) \
    conv_epilogue8_body<MP, MC, TC, FULL_, ACT_, RES_, WS>(p, acc, rres, lds_bias, lds_slope, lds_wscale, m0, c0, prow0, crow0, fr, fh, HoWo, inv_howo, inv_wo)
    const bool full = m0 + TP <= p.M && c0 + TC <= p.Cout;
    if (!full || !WS) { FRP_EPI8(false, -1, -1); return; }        // ragged tiles, and fp16 kernels that add an fp8 copy
    const bool has_res = p.res != nullptr;
    if (p.act == FRP_ACT_PRELU) { if (has_res) FRP_EPI8(true, FRP_ACT_PRELU, 1); else FRP_EPI8(true, FRP_ACT_PRELU, 0); }
    else { if (has_res) FRP_EPI8(true, FRP_ACT_NONE, 1); else FRP_EPI8(true, -1, 0); }
#undef FRP_EPI8
}

// residual of a tile in the STORE layout (16-byte chunks: couts 16q + 8*fh .. +7 of this lane's pixel), from clamped -
// always valid - addresses; consumed by conv_epilogue
template <int MP, int MC>
__device__ __forceinline__ void conv_residual_loads(const ConvParams& p, uint4 (&rres)[MP][MC][2], int m0, int c0, int prow0, int crow0,
                                                    int fr, int fh, int HoWo, float inv_howo, float inv_wo, int ps = 1, int po = 0) {
    const bool up2 = p.flags & FRP_FLAG_RES_UP2;
#pragma unroll
    for (int i = 0; i < MP; ++i) {
        const int mraw = m0 + (prow0 + i * 32 + fr) * ps + po;
        const int m = mraw < p.M ? mraw : 0;
        long ridx = (long)m * p.Cout;
        if (up2) {
            int n, rem, oy, ox;
            fast_divmod(m, HoWo, inv_howo, n, rem);
            fast_divmod(rem, p.Wo, inv_wo, oy, ox);
            ridx = (((long)n * p.Hr + (oy >> 1)) * p.Wr + (ox >> 1)) * p.Cout;
        }
#pragma unroll
        for (int j = 0; j < MC; ++j)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int co = c0 + crow0 + j * 32 + 16 * q + 8 * fh;
                rres[i][j][q] = *reinterpret_cast<const uint4*>(p.res + ridx + (co < p.Cout ? co : 0));
            }
    }
}

__device__ __forceinline__ void wait_lgkmcnt0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// In front of a k-step's barrier: every fragment read of the step before must have RETURNED before another wave, released by
// this barrier, fires the LDS-DMA that restages the ring slot it read (write after read).  The source order alone does not
// give that: the compiler sinks the last MFMA group of a step - and with it the lgkmcnt wait that retires its reads - below
// the barrier, and under LDS load (two workgroups per CU, 2 reads per MFMA: the quarter-tile configurations) a read issued
// before the barrier lost the race against a DMA from L2 issued after it: one wave with one stale 8-row piece, one launch in
// four (tools/quarter_check.py).  FRP_WAR_RELAXED builds leave the wait out (A/B of its cost).
__device__ __forceinline__ void retire_lds_reads() {
#ifndef FRP_WAR_RELAXED
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

}  // namespace frp
