// Face tracks: the device step between the detector and the embedder that decides which detections belong to a face identified
// before, hands the embedder only the others, and gives the rest their cached result (frp.h: frp_track_config; the written form of
// the semantics and the reference of every test: tracks.TrackModel).
//
// Four launches per pass, stream-ordered:
//   track_associate_kernel  one wave per stream that occurs in the batch (+ one for the frames of stream -1).  The stream's entry
//                           list lives in LDS (two lists: the frame's old one and the one being built), two entries per lane.  Per
//                           detection, in detector order: IoU against the lane's two entries by the NMS kernels' own function (box_nms.h:
//                           box_iou1, a = the detection, b = the entry; +1-pixel areas, fp32, one rounding per operation - the file
//                           is built with -ffp-contract=off, as every file that includes that header),
//                           the candidates (unclaimed, iou >= iou_min: a NaN fails) keyed (iou bits << 8) | (255 - entry) and reduced
//                           with a cross-lane max - a total order: largest IoU, then lowest entry.  Everything else of a frame (ids,
//                           the new list, the slots' outputs) is lane-parallel behind that serial loop, ordered by ballots.
//   track_compact_kernel    one block, the twin of compact_faces_kernel: face_slot / nfaces of the EMBEDDED slots, frame-major, and
//                           every embedded slot's compact position; one thread adds the pass's counts to the two 64-bit totals.
//   (align, embedder, l2norm, matcher run on that list)
//   track_resolve_kernel    one block per slot: emb / idx / cos from the slot's source into the per-slot [B][K] arrays.
//   track_store_kernel      one block per row of every touched stream's new table half: the same copy from the row's source.
//
// A source is always a ROOT: a row of the stream's old half, or a slot of this batch that is embedded in this pass - a reused slot
// and a row inherit the source of the entry they came from, never point at another reused slot.
//
// No launch reads memory that another workgroup of the same launch writes:
//   associate  workgroup s reads header s and the old half of stream s (`cur`), the batch's boxes / counts / streams; it writes header
//              s, plan s, rows of the OTHER half of stream s and the slots of its own frames (every frame has exactly one stream).
//   compact    one workgroup.
//   resolve    reads slot descriptors, compact positions, the compact results, plans and OLD halves; writes the per-slot arrays only.
//   store      reads the descriptors the associate launch left in the NEW rows and the sources above; workgroup (row, stream) writes
//              that row's embedding and idx / cos in the new half - which nothing in the launch reads: sources are old rows and
//              compact results.  The halves swap in the header, so the next pass reads what this one stored.
//
// A few hundred KB per pass: latency-bound, nothing here is tuned beyond keeping the serial loop short.  No scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "box_nms.h"
#include "frp.h"
#include "frp_internal.h"

namespace frp {

#define TK_T FRP_TRACK_SLOTS
static_assert(TK_T == 128 && FRP_MAX_FACES_CAP <= TK_T, "two entries, and two detections, per lane of one wave");

struct TkItem {      // the working form of an entry (LDS)
    float x1, y1, x2, y2;
    int32_t id, age, missed, src;
};

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

__device__ __forceinline__ unsigned long long tk_key(float ex1, float ey1, float ex2, float ey2, float ea, float dx1, float dy1, float dx2,
                                                     float dy2, float da, float iou_min, int e) {
    const float iou = box_iou1(dx1, dy1, dx2, dy2, da, ex1, ey1, ex2, ey2, ea);      // a = the detection, b = the entry: tracks.iou's order
    return iou >= iou_min ? (((unsigned long long)__float_as_uint(iou) << 8) | (unsigned long long)(255 - e)) : 0ull;
}

__global__ __launch_bounds__(64) void track_associate_kernel(TrackParams p) {
    __shared__ TkItem lists[2][TK_T];
    const int lane = threadIdx.x;
    const int K = p.K;
    const bool tracked = (int)blockIdx.x < p.n_present;
    const int s = tracked ? p.present[blockIdx.x] : -1;
    const unsigned long long lt = (1ull << lane) - 1ull;

    int n_old = 0, next_id = 0, old_half = 0;
    if (tracked) {
        const TrackHeader hd = p.hdr[s];
        n_old = min(max(hd.n, 0), TK_T);
        next_id = hd.next_id;
        old_half = hd.cur & 1;
        const TrackEntry* src = p.meta + ((long)s * 2 + old_half) * TK_T;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int e = lane + 64 * t;
            if (e < n_old) {
                const float4 bx = ((const float4*)(src + e))[0], st = ((const float4*)(src + e))[1];      // box; id, age, missed, -
                lists[0][e] = TkItem{bx.x, bx.y, bx.z, bx.w, __float_as_int(st.x), __float_as_int(st.y), __float_as_int(st.z), -1 - e};
            }
        }
    }
    __syncthreads();

    int cur = 0;
    for (int b = 0; b < p.B; ++b) {
        if (p.streams[b] != s) continue;                     // uniform
        const int n = min(max(p.counts[b], 0), K);
        const float* fb = p.boxes + (long)b * K * 4;
        int w0 = -1, w1 = -1;                                // the entry detections `lane` and `lane + 64` took
        bool c0 = false, c1 = false;                         // entries `lane` and `lane + 64` are claimed
        if (tracked) {
            const TkItem* L = lists[cur];
            const bool v0 = lane < n_old, v1 = lane + 64 < n_old;
            float ax1 = 0.f, ay1 = 0.f, ax2 = 0.f, ay2 = 0.f, bx1 = 0.f, by1 = 0.f, bx2 = 0.f, by2 = 0.f;
            if (v0) { ax1 = L[lane].x1; ay1 = L[lane].y1; ax2 = L[lane].x2; ay2 = L[lane].y2; }
            if (v1) { bx1 = L[lane + 64].x1; by1 = L[lane + 64].y1; bx2 = L[lane + 64].x2; by2 = L[lane + 64].y2; }
            const float aa = box_area1(ax1, ay1, ax2, ay2), ba = box_area1(bx1, by1, bx2, by2);
            for (int j = 0; j < n; ++j) {                    // the serial part
                const float dx1 = fb[4 * j], dy1 = fb[4 * j + 1], dx2 = fb[4 * j + 2], dy2 = fb[4 * j + 3];
                const float da = box_area1(dx1, dy1, dx2, dy2);
                unsigned long long k0 = 0ull, k1 = 0ull;
                if (v0 && !c0) k0 = tk_key(ax1, ay1, ax2, ay2, aa, dx1, dy1, dx2, dy2, da, p.iou_min, lane);
                if (v1 && !c1) k1 = tk_key(bx1, by1, bx2, by2, ba, dx1, dy1, dx2, dy2, da, p.iou_min, lane + 64);
                const unsigned long long best = wave_max_u64(k0 > k1 ? k0 : k1);
                const int w = best ? 255 - (int)(best & 255ull) : -1;
                if (w == lane) c0 = true;
                if (w == lane + 64) c1 = true;
                if (j == lane) w0 = w;
                if (j == lane + 64) w1 = w;
            }
        }
        // ---- lane-parallel: the detections' ids and outputs, the new list
        const bool d0 = lane < n, d1 = lane + 64 < n;
        const unsigned long long u0 = __ballot(d0 && w0 < 0), u1 = __ballot(d1 && w1 < 0);
        const int nu0 = __popcll(u0);
        TkItem* N = lists[cur ^ 1];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int d = lane + 64 * t;
            if (d >= K) continue;
            const long slot = (long)b * K + d;
            const int w = t ? w1 : w0;
            int id = -1, age = 0, reused = 0, src = FRP_TRACK_DEAD;
            if (d < n) {
                src = (int)slot;
                if (tracked) {
                    if (w >= 0) {
                        const TkItem o = lists[cur][w];
                        id = o.id;
                        const int a = o.age + 1;
                        if (a < p.refresh && !p.stale) { reused = 1; age = a; src = o.src; }
                    } else {
                        id = next_id + (t ? nu0 + __popcll(u1 & lt) : __popcll(u0 & lt));
                    }
                    N[d] = TkItem{fb[4 * d], fb[4 * d + 1], fb[4 * d + 2], fb[4 * d + 3], id, age, 0, src};
                }
            }
            p.track_id[slot] = id; p.reused[slot] = reused; p.age[slot] = age; p.src[slot] = src;
        }
        if (!tracked) continue;
        next_id += nu0 + __popcll(u1);
        // the unclaimed old entries behind the detections, in their old order, while missed <= max_missed; cut at T
        bool keep0 = false, keep1 = false;
        if (lane < n_old && !c0) keep0 = lists[cur][lane].missed + 1 <= p.max_missed;
        if (lane + 64 < n_old && !c1) keep1 = lists[cur][lane + 64].missed + 1 <= p.max_missed;
        const unsigned long long m0 = __ballot(keep0), m1 = __ballot(keep1);
        const int q0 = n + __popcll(m0 & lt), q1 = n + __popcll(m0) + __popcll(m1 & lt);
        if (keep0 && q0 < TK_T) { TkItem r = lists[cur][lane]; r.missed += 1; r.age += 1; N[q0] = r; }
        if (keep1 && q1 < TK_T) { TkItem r = lists[cur][lane + 64]; r.missed += 1; r.age += 1; N[q1] = r; }
        n_old = min(n + __popcll(m0) + __popcll(m1), TK_T);
        cur ^= 1;
        __syncthreads();
    }

    if (!tracked) return;
    // ---- the stream's new half: metadata and source descriptors (embeddings, idx, cos: track_store_kernel), then the swap
    const int new_half = old_half ^ 1;
    TrackEntry* dst = p.meta + ((long)s * 2 + new_half) * TK_T;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int e = lane + 64 * t;
        if (e < n_old) {
            const TkItem r = lists[cur][e];
            float4* o = (float4*)(dst + e);          // (three 16-byte stores; a TrackEntry temporary would live in scratch)
            o[0] = make_float4(r.x1, r.y1, r.x2, r.y2);
            o[1] = make_float4(__int_as_float(r.id), __int_as_float(r.age), __int_as_float(r.missed), __int_as_float(-1));
            o[2] = make_float4(0.f, __int_as_float(r.src), 0.f, 0.f);
        }
    }
    if (lane == 0) {
        p.hdr[s] = TrackHeader{next_id, n_old, new_half, 0};
        p.plan[s] = TrackPlan{old_half, n_old};
    }
}

// slot descriptors -> face_slot[n] (frame-major), nfaces, pos[slot]; the pass's counts onto the totals.  One block.
__global__ __launch_bounds__(256) void track_compact_kernel(TrackParams p) {
    __shared__ int offs[1024 + 1];
    __shared__ int reu[1024];
    const int K = p.K;
    for (int b = threadIdx.x; b < p.B; b += blockDim.x) {
        int ne = 0, nr = 0;
        for (int k = 0; k < K; ++k) {
            const int src = p.src[(long)b * K + k];
            if (src == FRP_TRACK_DEAD) continue;
            if (p.reused[(long)b * K + k]) ++nr; else ++ne;
        }
        offs[b + 1] = ne;
        reu[b] = nr;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        long r = 0;
        for (int b = 0; b < p.B; ++b) { const int c = offs[b + 1]; offs[b] = acc; acc += c; r += reu[b]; }
        offs[p.B] = acc;
        *p.nfaces = acc;
        p.totals[0] += acc;
        p.totals[1] += r;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < p.B; b += blockDim.x) {
        int o = offs[b];
        for (int k = 0; k < K; ++k) {
            const long slot = (long)b * K + k;
            const bool emb = p.src[slot] != FRP_TRACK_DEAD && !p.reused[slot];
            p.pos[slot] = emb ? o : -1;
            if (emb) p.face_slot[o++] = (int)slot;
        }
    }
}

// the 512 floats + idx + cos a source descriptor of stream s stands for; 128 threads, one float4 each
__device__ __forceinline__ void tk_fetch(const TrackParams& p, int s, int src, float4& v, int32_t& idx, float& cs) {
    v = make_float4(0.f, 0.f, 0.f, 0.f);
    idx = -1;
    cs = 0.f;
    if (src >= 0) {
        const int f = src < p.B * p.K ? p.pos[src] : -1;
        if (f < 0) return;
        v = ((const float4*)(p.emb + (long)f * FRP_EMB_DIM))[threadIdx.x];
        if (p.best_idx) { idx = p.best_idx[f]; cs = p.best_cos[f]; }
    } else if (s >= 0) {
        const int e = -1 - src;
        if (e >= TK_T) return;
        const long row = ((long)s * 2 + (p.plan[s].old_half & 1)) * TK_T + e;
        v = ((const float4*)(p.tab_emb + row * FRP_EMB_DIM))[threadIdx.x];
        idx = p.meta[row].match_idx;
        cs = p.meta[row].match_cos;
    }
}

__global__ __launch_bounds__(128) void track_resolve_kernel(TrackParams p) {
    const long slot = blockIdx.x;
    const int src = p.src[slot];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    int32_t idx = -1;
    float cs = -1.f;
    if (src != FRP_TRACK_DEAD) tk_fetch(p, p.streams[slot / p.K], src, v, idx, cs);
    ((float4*)(p.slot_emb + slot * FRP_EMB_DIM))[threadIdx.x] = v;
    if (threadIdx.x == 0) { p.slot_idx[slot] = idx; p.slot_cos[slot] = cs; }
}

__global__ __launch_bounds__(128) void track_store_kernel(TrackParams p) {
    const int s = p.present[blockIdx.y];
    const int e = blockIdx.x;
    const TrackPlan pl = p.plan[s];
    if (e >= pl.n_new) return;
    const long row = ((long)s * 2 + ((pl.old_half & 1) ^ 1)) * TK_T + e;
    float4 v;
    int32_t idx;
    float cs;
    tk_fetch(p, s, p.meta[row].src, v, idx, cs);
    ((float4*)(p.tab_emb + row * FRP_EMB_DIM))[threadIdx.x] = v;
    if (threadIdx.x == 0) { p.meta[row].match_idx = idx; p.meta[row].match_cos = cs; }
}

static bool track_params_ok(const TrackParams& p) {
    return p.B > 0 && p.B <= 1024 && p.K > 0 && p.K <= FRP_MAX_FACES_CAP && p.max_streams > 0 && p.n_present >= 0 &&
           p.n_present <= p.max_streams && p.hdr && p.meta && p.tab_emb && p.plan && p.totals && p.streams && (p.present || !p.n_present) &&
           p.track_id && p.reused && p.age && p.src && p.pos;
}

hipError_t launch_track_associate(const TrackParams& p, hipStream_t stream) {
    if (!track_params_ok(p) || !p.boxes || !p.counts || !p.face_slot || !p.nfaces) return hipErrorInvalidValue;
    hipLaunchKernelGGL(track_associate_kernel, dim3(p.n_present + 1), dim3(64), 0, stream, p);
    hipLaunchKernelGGL(track_compact_kernel, dim3(1), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_track_resolve(const TrackParams& p, hipStream_t stream) {
    if (!track_params_ok(p) || !p.emb || !p.slot_emb || !p.slot_idx || !p.slot_cos || (p.best_idx && !p.best_cos)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(track_resolve_kernel, dim3(p.B * p.K), dim3(128), 0, stream, p);
    if (p.n_present > 0) hipLaunchKernelGGL(track_store_kernel, dim3(TK_T, p.n_present), dim3(128), 0, stream, p);
    return hipGetLastError();
}

}  // namespace frp
