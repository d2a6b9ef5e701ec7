// Entropy decoding on the device for JPEG scans WITHOUT restart markers: the self-synchronising decoder (the algorithm and what every
// thread runs: jpeg_selfsync.h; the host's part: ingest_api.cpp: decode_selfsync; table load and prefix sum: jpeg_entropy_dev.h).  A scan
// is ONE serial bit stream; it is cut into subsequences of S raw bytes, one thread each, JSS_WG of them per workgroup:
//   jss_sync_kernel, launch 0   every thread decodes its subsequence from the guessed state (byte boundary, block 0 of an MCU, DC next),
//                               then the workgroup iterates entry(t) = exit(t - 1) over the exit states it holds in LDS - a thread whose
//                               entry changed decodes again - until a round changes nothing (at most JSS_WG rounds: round r leaves
//                               threads 0 .. r final);
//   jss_sync_kernel, launch k   the same rounds, thread 0 entering with the exit of the workgroup before it AS THE PREVIOUS LAUNCH LEFT IT
//                               (double-buffered in wgx: no workgroup waits for another; the ordering is the kernel boundary).  Launch k
//                               leaves workgroups 0 .. k final; the host launches again while a launch reports a round with a change.
//   jss_count_kernel            exclusive prefix sums of the blocks completed = every subsequence's first block; the image's block sum
//   jss_write_kernel            every thread decodes once more from its final entry and scatters coefficients (the DC DIFFERENCE at 0)
//   jss_dc_kernel               per component the running sum of the differences in scan order
// At the fix-point every entry is the exit of the subsequence before it, and the first one's is the true start: by induction the states
// are those of the serial decode - there is no heuristic acceptance.  Every loop is bounded (symbols by the bits of the range, rounds by
// JSS_WG, chunks by the array's length) and no workgroup spins on another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frp_internal.h"
#include "jpeg_entropy_dev.h"

namespace frp {

namespace {

__global__ __launch_bounds__(JSS_WG) void jss_sync_kernel(JpegSelfsyncParams p, int k) {
    __shared__ JpegHuffTableDev tab[6];
    __shared__ uint8_t zz[64];
    __shared__ JssState ex[JSS_WG + 1];          // ex[t + 1] = exit of thread t; ex[0] = what thread 0 enters with
    const int b = blockIdx.y, t = threadIdx.x;
    const uint32_t* im = p.img + 4 * b;
    const uint32_t n_bytes = im[1], n_sub = im[2], sub0 = im[3];
    const uint32_t first = blockIdx.x * JSS_WG;
    if (first >= n_sub) return;
    const uint32_t m = n_sub - first < JSS_WG ? n_sub - first : JSS_WG;          // live threads
    const uint32_t wg = sub0 / JSS_WG + blockIdx.x;
    JssState* wg_in = p.wgx + (size_t)(k & 1) * p.n_wg_all;
    JssState* wg_out = p.wgx + (size_t)((k & 1) ^ 1) * p.n_wg_all;
    if (k > 0 && blockIdx.x == 0) {              // final since launch 0: hands its exit on
        if (t == 0) wg_out[wg] = p.exit_[sub0 + m - 1];
        return;
    }
    load_entropy_tables<JSS_WG>(p.tables, b, tab, zz);
    const uint8_t* scan = p.scan + im[0];
    const uint32_t i = first + t, gi = sub0 + i;
    const bool live = (uint32_t)t < m;
    uint32_t end_bit = 0, done = 0;
    JssState entry = 0, exit_state = 0;
    if (live) end_bit = jss_start(scan, n_bytes, i + 1, n_sub, (uint32_t)p.S) * 8u;
    __syncthreads();
    if (k == 0) {
        if (live) {
            entry = jss_pack(jss_start(scan, n_bytes, i, n_sub, (uint32_t)p.S) * 8u, 0, 0);
            jss_decode<false>(scan, n_bytes, tab, zz, p.g, entry, end_bit, nullptr, 0, &exit_state, &done);
        }
        if (t == 0) ex[0] = entry;               // (the first subsequence of a workgroup keeps its guess in this launch; the image's first one: the truth)
    } else {
        if (live) { entry = p.entry[gi]; exit_state = p.exit_[gi]; done = p.cnt[gi]; }
        if (t == 0) ex[0] = wg_in[wg - 1];
    }
    if (live) ex[t + 1] = exit_state;
    int with_change = 0;
    for (int r = 0; r < JSS_WG; ++r) {
        __syncthreads();
        const JssState ne = ex[t];
        const bool ch = live && ne != entry;
        __syncthreads();                         // everyone has read its predecessor's exit before anyone replaces its own
        if (ch) {
            entry = ne;
            jss_decode<false>(scan, n_bytes, tab, zz, p.g, entry, end_bit, nullptr, 0, &exit_state, &done);
            ex[t + 1] = exit_state;
        }
        if (!__syncthreads_or(ch ? 1 : 0)) break;
        ++with_change;
    }
    if (live && (k == 0 || with_change)) { p.entry[gi] = entry; p.exit_[gi] = exit_state; p.cnt[gi] = done; }
    if ((uint32_t)t == m - 1) wg_out[wg] = exit_state;
    if (t == 0 && with_change) atomicMax(p.rounds + b, with_change);
}

// one workgroup per image, chunks of JSS_WG subsequences: inclusive scan of a chunk in LDS + the running sum of the chunks before
__global__ __launch_bounds__(JSS_WG) void jss_count_kernel(JpegSelfsyncParams p) {
    __shared__ uint32_t sc[JSS_WG];
    const int b = blockIdx.x, t = threadIdx.x;
    const uint32_t* im = p.img + 4 * b;
    const uint32_t n_sub = im[2], sub0 = im[3];
    uint32_t running = 0;
    for (uint32_t c0 = 0; c0 < n_sub; c0 += JSS_WG) {
        const uint32_t i = c0 + t;
        const uint32_t v = i < n_sub ? p.cnt[sub0 + i] : 0u;
        uint32_t sum;
        const uint32_t incl = wg_inclusive_scan<JSS_WG>(sc, v, sum);
        if (i < n_sub) p.base[sub0 + i] = running + incl - v;
        running += sum;
    }
    if (t == 0) {
        int32_t* st = p.stats + 4 * b;
        st[0] = (int32_t)n_sub;
        st[2] = (int32_t)(running < p.g.total ? running : p.g.total);
        if (running < p.g.total) atomicOr(st + 3, 1);          // the scan ends before the image's last block
    }
}

__global__ __launch_bounds__(JSS_WG) void jss_write_kernel(JpegSelfsyncParams p) {
    __shared__ JpegHuffTableDev tab[6];
    __shared__ uint8_t zz[64];
    const int b = blockIdx.y, t = threadIdx.x;
    const uint32_t* im = p.img + 4 * b;
    const uint32_t n_bytes = im[1], n_sub = im[2], sub0 = im[3];
    if (blockIdx.x * JSS_WG >= n_sub) return;
    load_entropy_tables<JSS_WG>(p.tables, b, tab, zz);
    __syncthreads();
    const uint32_t i = blockIdx.x * JSS_WG + t;
    if (i >= n_sub) return;
    const uint8_t* scan = p.scan + im[0];
    const uint32_t blk0 = p.base[sub0 + i];
    if (blk0 >= p.g.total) return;               // pad bits and bytes behind the last block
    const uint32_t end_bit = jss_start(scan, n_bytes, i + 1, n_sub, (uint32_t)p.S) * 8u;
    // (every coefficient write is to a block below g.total: jss_decode<true>)
    if (jss_decode<true>(scan, n_bytes, tab, zz, p.g, p.entry[sub0 + i], end_bit, p.coef + (long)b * p.coef_per_image, blk0, nullptr, nullptr))
        atomicOr(p.stats + 4 * b + 3, 1);
}

// one workgroup per (component, image): the running sum of the DC differences in scan order, in chunks of JSS_WG blocks; accumulated in
// 32 bits and stored as int16, as the host decoder does
__global__ __launch_bounds__(JSS_WG) void jss_dc_kernel(JpegSelfsyncParams p) {
    __shared__ uint32_t sc[JSS_WG];
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    int16_t* coef = p.coef + (long)b * p.coef_per_image;
    const uint32_t nb = p.g.total / (uint32_t)p.g.bpm * (uint32_t)(p.g.hs[c] * p.g.vs[c]);
    uint32_t running = 0;
    for (uint32_t c0 = 0; c0 < nb; c0 += JSS_WG) {
        const uint32_t kk = c0 + t;
        int16_t* d = kk < nb ? coef + jss_dc_addr(p.g, c, kk) : nullptr;
        uint32_t sum;
        const uint32_t incl = wg_inclusive_scan<JSS_WG>(sc, d ? (uint32_t)(int32_t)*d : 0u, sum);
        if (d) *d = (int16_t)(int32_t)(running + incl);
        running += sum;
    }
}

bool params_ok(const JpegSelfsyncParams& p) {
    return p.B > 0 && p.B <= 65535 && p.S >= 16 && p.S <= 1024 && p.S % 16 == 0 && p.max_sub > 0 && p.n_wg_all > 0 && p.scan && p.img && p.tables &&
           p.entry && p.exit_ && p.wgx && p.cnt && p.base && p.rounds && p.stats && p.coef && p.g.components >= 1 && p.g.components <= 3 &&
           p.g.bpm >= 1 && p.g.bpm <= 6 && p.g.mcus_x > 0 && p.g.total > 0;
}

}  // namespace

hipError_t launch_jpeg_selfsync_round(const JpegSelfsyncParams& p, int k, hipStream_t stream) {
    if (!params_ok(p) || k < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jss_sync_kernel, dim3((p.max_sub + JSS_WG - 1) / JSS_WG, (unsigned)p.B), dim3(JSS_WG), 0, stream, p, k);
    return hipGetLastError();
}

hipError_t launch_jpeg_selfsync_finish(const JpegSelfsyncParams& p, hipStream_t stream) {
    if (!params_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jss_count_kernel, dim3((unsigned)p.B), dim3(JSS_WG), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(jss_write_kernel, dim3((p.max_sub + JSS_WG - 1) / JSS_WG, (unsigned)p.B), dim3(JSS_WG), 0, stream, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(jss_dc_kernel, dim3((unsigned)p.g.components, (unsigned)p.B), dim3(JSS_WG), 0, stream, p);
    return hipGetLastError();
}

}  // namespace frp
