// Greedy gallery clustering on the device (frp.h: frp_gallery_cluster; the reference's sweep: face_service.py:552-585).  The sweep
// runs in POSITIONS: order[p] is the gallery row of the p-th name, seed_pos[p] the position of the seed that took p (-1: unassigned).
// One tile of the sweep (host loop: cluster_api.cpp) is
//   pick     the first `tile` unassigned positions at or after the cursor -> cand[], their count, the next cursor
//   stage    the candidates' rows as queries (fp16 route: widened to float32 for normalize_rows_kernel; exact route: float64 copies)
//   scores   the matcher's per-tile kernel with its all_scores epilogue / gallery_distances_kernel, unchanged (match.hip)
//   resolve  which candidates are seeds: c_t is one iff no earlier seed of the tile passed it (one wave, 64-bit masks)
//   assign   every unassigned position takes the first seed of the tile, in tile order, that passes it
// pass(s, p) always has the seed as the query and p's gallery row as the column: the fp16 scores are not symmetric.
//   fp16 rows:  score[s][order[p]] >= min_cos in float32;   exact rows:  dist[s][order[p]] <= max_dist in float64;   a NaN never passes.
// Flags, counts and labels are written with ordinary vector stores; cross-lane work is __ballot and __shfl.
#include <hip/hip_runtime.h>

#include "frp_internal.h"

namespace frp {

template <typename T> __device__ inline bool cluster_pass(T v, T bound);
template <> __device__ inline bool cluster_pass<float>(float v, float bound) { return v >= bound; }      // a cosine at or above the bound
template <> __device__ inline bool cluster_pass<double>(double v, double bound) { return v <= bound; }   // a distance at or below it

// One workgroup of four waves walks forward from the cursor, 256 positions a step, and stops once it has `tile` candidates: over a
// whole sweep the cursor only moves forward, so all picks together read seed_pos once.
__global__ __launch_bounds__(256) void cluster_pick_kernel(const int32_t* __restrict__ seed_pos, int n, int tile, int32_t* __restrict__ ctl) {
    __shared__ int wcnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cursor = ctl[CLUSTER_CTL_CURSOR];
    int found = 0;          // the same in every thread
    for (int base = cursor; base < n && found < tile; base += 256) {
        const int p = base + (int)threadIdx.x;
        const bool un = p < n && seed_pos[p] < 0;
        const unsigned long long b = __ballot(un);
        if (lane == 0) wcnt[wave] = __popcll(b);
        __syncthreads();          // (every thread has read the cursor before the first of these: it is written behind one)
        int k = found + __popcll(b & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) k += wcnt[w];
        if (un && k < tile) {
            ctl[CLUSTER_CTL_CAND + k] = p;
            if (k == tile - 1) ctl[CLUSTER_CTL_CURSOR] = p + 1;
        }
        found += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ctl[CLUSTER_CTL_COUNT] = found < tile ? found : tile;
        if (found < tile) ctl[CLUSTER_CTL_CURSOR] = n;
    }
}

// the candidates' unit fp16 gallery rows, widened: what gallery_get().astype(float32) hands to the normaliser on the host route
__global__ __launch_bounds__(64) void cluster_stage_f16_kernel(const _Float16* __restrict__ gallery, const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ ctl, float* __restrict__ out) {
    const int t = blockIdx.x;
    if (t >= ctl[CLUSTER_CTL_COUNT]) return;
    const _Float16* src = gallery + (long)order[ctl[CLUSTER_CTL_CAND + t]] * FRP_EMB_DIM;
    for (int i = threadIdx.x; i < FRP_EMB_DIM; i += 64) out[(long)t * FRP_EMB_DIM + i] = (float)src[i];
}

// the candidates' float64 rows as enrolled: the query block of gallery_distances_kernel
__global__ __launch_bounds__(64) void cluster_stage_f64_kernel(const double* __restrict__ rows, const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ ctl, double* __restrict__ out) {
    const int t = blockIdx.x;
    if (t >= ctl[CLUSTER_CTL_COUNT]) return;
    const double* src = rows + (long)order[ctl[CLUSTER_CTL_CAND + t]] * FRP_EMB_DIM;
    for (int i = threadIdx.x; i < FRP_EMB_DIM; i += 64) out[(long)t * FRP_EMB_DIM + i] = src[i];
}

// One wave.  Lane t forms A[t], the set of candidates u that candidate t passes; then 64 uniform steps decide the seeds in tile
// order.  Seeds label themselves here, whatever their own score is (a zero or NaN row is a cluster of one).
template <typename T>
__global__ __launch_bounds__(64) void cluster_resolve_kernel(const T* __restrict__ score, long N, const int32_t* __restrict__ order, T bound,
                                                             int32_t* __restrict__ ctl, int32_t* __restrict__ seed_pos) {
    const int lane = threadIdx.x;
    const int count = ctl[CLUSTER_CTL_COUNT];
    if (count <= 0) return;
    unsigned long long a = 0;
    if (lane < count)
        for (int u = 0; u < count; ++u)
            if (cluster_pass<T>(score[(long)lane * N + order[ctl[CLUSTER_CTL_CAND + u]]], bound)) a |= 1ull << u;
    const int lo = (int)(unsigned)a, hi = (int)(unsigned)(a >> 32);
    unsigned long long seeds = 0, taken = 0;
    for (int t = 0; t < count; ++t) {
        const unsigned long long at = (unsigned long long)(unsigned)__shfl(lo, t) | ((unsigned long long)(unsigned)__shfl(hi, t) << 32);
        if (!((taken >> t) & 1ull)) { seeds |= 1ull << t; taken |= at; }
    }
    if (lane < count && ((seeds >> lane) & 1ull)) {
        const int p = ctl[CLUSTER_CTL_CAND + lane];
        seed_pos[p] = p;
    }
    if (lane == 0) {
        ctl[CLUSTER_CTL_SEEDS_LO] = (int)(unsigned)seeds;
        ctl[CLUSTER_CTL_SEEDS_HI] = (int)(unsigned)(seeds >> 32);
        ctl[CLUSTER_CTL_NCLUSTERS] += __popcll(seeds);
    }
}

// A grid over positions: an unassigned one reads the seeds' scores of its own gallery row, in tile order, and takes the first that passes.
template <typename T>
__global__ __launch_bounds__(256) void cluster_assign_kernel(const T* __restrict__ score, long N, const int32_t* __restrict__ order, int n, T bound,
                                                             const int32_t* __restrict__ ctl, int32_t* __restrict__ seed_pos) {
    const int p = blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= n || seed_pos[p] >= 0) return;
    unsigned long long seeds = (unsigned long long)(unsigned)ctl[CLUSTER_CTL_SEEDS_LO] | ((unsigned long long)(unsigned)ctl[CLUSTER_CTL_SEEDS_HI] << 32);
    const long row = order[p];
    while (seeds) {
        const int t = __ffsll((long long)seeds) - 1;
        seeds &= seeds - 1;
        if (cluster_pass<T>(score[(long)t * N + row], bound)) {
            seed_pos[p] = ctl[CLUSTER_CTL_CAND + t];
            return;
        }
    }
}

static bool cluster_args_ok(const ClusterParams& p) {
    return p.order && p.seed_pos && p.ctl && p.n > 0 && p.N > 0 && p.tile >= 1 && p.tile <= CLUSTER_MAX_TILE;
}

hipError_t launch_cluster_pick(const ClusterParams& p, hipStream_t stream) {
    if (!cluster_args_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_pick_kernel, dim3(1), dim3(256), 0, stream, (const int32_t*)p.seed_pos, p.n, p.tile, p.ctl);
    return hipGetLastError();
}

hipError_t launch_cluster_stage_f16(const ClusterParams& p, const _Float16* gallery, float* out, hipStream_t stream) {
    if (!cluster_args_ok(p) || !gallery || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_stage_f16_kernel, dim3(p.tile), dim3(64), 0, stream, gallery, p.order, (const int32_t*)p.ctl, out);
    return hipGetLastError();
}

hipError_t launch_cluster_stage_f64(const ClusterParams& p, const double* rows, double* out, hipStream_t stream) {
    if (!cluster_args_ok(p) || !rows || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_stage_f64_kernel, dim3(p.tile), dim3(64), 0, stream, rows, p.order, (const int32_t*)p.ctl, out);
    return hipGetLastError();
}

template <typename T>
static hipError_t cluster_sweep(const ClusterParams& p, const T* score, T bound, hipStream_t stream) {
    if (!cluster_args_ok(p) || !score) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_resolve_kernel<T>, dim3(1), dim3(64), 0, stream, score, p.N, p.order, bound, p.ctl, p.seed_pos);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cluster_assign_kernel<T>, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, stream, score, p.N, p.order, p.n, bound,
                       (const int32_t*)p.ctl, p.seed_pos);
    return hipGetLastError();
}

hipError_t launch_cluster_sweep_cos(const ClusterParams& p, const float* score, float min_cos, hipStream_t stream) {
    return cluster_sweep<float>(p, score, min_cos, stream);
}

hipError_t launch_cluster_sweep_dist(const ClusterParams& p, const double* dist, double max_dist, hipStream_t stream) {
    return cluster_sweep<double>(p, dist, max_dist, stream);
}

}  // namespace frp
