// Device-only helpers of the entropy decode kernels (jpeg_kernels.hip: jpeg_huffman_kernel, jpeg_selfsync.hip: jss_*): the table load into
// LDS and the workgroup prefix sum.  Force-inlined into each kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_entropy.h"

namespace frp {

// Image b's six tables and the zig-zag order -> LDS, by a workgroup of at least 64 threads (dwords: the struct is a multiple of 4 bytes);
// the caller's barrier follows.  (In LDS because both are indexed per lane: from constant memory every symbol waited a vector-memory round
// trip.)
template <int WG>
__device__ __forceinline__ void load_entropy_tables(const JpegHuffTableDev* tables, int b, JpegHuffTableDev* tab, uint8_t* zz) {
    const unsigned* src = reinterpret_cast<const unsigned*>(tables + (long)b * 6);
    unsigned* dst = reinterpret_cast<unsigned*>(tab);
    for (int i = threadIdx.x; i < (int)(6 * sizeof(JpegHuffTableDev) / 4); i += WG) dst[i] = src[i];
    if (WG == 64 || threadIdx.x < 64) zz[threadIdx.x] = kJpegZigZag[threadIdx.x];
}

// Inclusive prefix sum of v over the WG threads of a workgroup through sc[WG] (LDS): -> this thread's sum, `total` = the last thread's.
// Sums wrap in 32 bits.  Every thread of the workgroup calls it (its barriers lie outside any branch); sc is free again on return.
template <int WG>
__device__ __forceinline__ uint32_t wg_inclusive_scan(uint32_t* sc, uint32_t v, uint32_t& total) {
    const int t = threadIdx.x;
    sc[t] = v;
    __syncthreads();
    for (int d = 1; d < WG; d <<= 1) {
        const uint32_t add = t >= d ? sc[t - d] : 0u;
        __syncthreads();
        sc[t] += add;
        __syncthreads();
    }
    const uint32_t sum = sc[t];
    total = sc[WG - 1];
    __syncthreads();
    return sum;
}

}  // namespace frp
