// The box arithmetic of the detection tail, in one place: the +1-pixel-area IoU, the descending key sort and the greedy NMS that
// decode_nms.hip (decode_nms_kernel), pyramid_kernels.hip (pyramid_merge_kernel) and track_kernels.hip (tk_key) share.
//
// The arithmetic is a contract: fp32, ONE rounding per operation, operands in the order written here, so the kernels reproduce their
// host models (oracle/network.py: decode_nms, pyramid.merge_scales, tracks.iou - independent restatements on purpose) bit for bit.
// box_area1 / box_iou1 switch contraction off in their own bodies; every other box expression of the including file (the decode of an
// anchor, the pyramid's rx / ry products) needs the same rule, so a file that includes this header must be named in the Makefile's
// -ffp-contract=off rule.  Included by those three files only.
#pragma once
#include <hip/hip_runtime.h>
#include "frp_internal.h"

namespace frp {

__host__ __device__ __forceinline__ float box_area1(float x1, float y1, float x2, float y2) {
#pragma clang fp contract(off)
    return (x2 - x1 + 1.0f) * (y2 - y1 + 1.0f);
}

// IoU of box a and box b with their box_area1 areas.  Not symmetric in the bits of a NaN / inf case: callers pass the operands in the
// order of their host model (NMS: a = the kept box, b = the candidate; tracker: a = the detection, b = the table entry).
__host__ __device__ __forceinline__ float box_iou1(float ax1, float ay1, float ax2, float ay2, float a_area, float bx1, float by1, float bx2,
                                                   float by2, float b_area) {
#pragma clang fp contract(off)
    const float xx1 = fmaxf(ax1, bx1), yy1 = fmaxf(ay1, by1);
    const float xx2 = fminf(ax2, bx2), yy2 = fminf(ay2, by2);
    const float w = fmaxf(0.0f, xx2 - xx1 + 1.0f), h = fmaxf(0.0f, yy2 - yy1 + 1.0f);
    const float inter = w * h;
    return inter / ((a_area + b_area) - inter);
}

// Bitonic sort of keys[0..N) in LDS, descending, by the N threads of the workgroup (tid = threadIdx.x; blockDim.x == N is the caller's
// to guarantee, here and in greedy_nms: both launch sites say so).  The caller's writes of
// `keys` must be behind a barrier; the sorted keys are behind one on return.
template <int N>
__device__ __forceinline__ void sort_keys_desc(unsigned long long* keys, int tid) {
    for (int k2 = 2; k2 <= N; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const int i = tid;
            const int ixj = i ^ j;
            if (ixj > i) {
                const unsigned long long a = keys[i], c = keys[ixj];
                const bool desc = (i & k2) == 0;
                if (desc ? (a < c) : (a > c)) { keys[i] = c; keys[ixj] = a; }
            }
            __syncthreads();
        }
    }
}

// The LDS state of one greedy NMS over at most N candidates, in sort order.
template <int N>
struct NmsBoxes {
    float x1[N], y1[N], x2[N], y2[N], area[N];
    unsigned char supp[N];
    int keep[FRP_MAX_FACES_CAP];     // out: the kept candidates' positions
    int keepn;

    // slot i empty: every slot of the n to come by some thread, slot 0 by one, ahead of the barrier in front of greedy_nms
    __device__ __forceinline__ void reset(int i) {
        supp[i] = 0;
        if (i == 0) keepn = 0;
    }
    __device__ __forceinline__ void set(int i, float bx1, float by1, float bx2, float by2) {
        x1[i] = bx1; y1[i] = by1; x2[i] = bx2; y2[i] = by2;
        area[i] = box_area1(bx1, by1, bx2, by2);
    }
};

// Greedy NMS of candidates 0..n) in that order by the N threads of the workgroup (as sort_keys_desc; n <= N, so every candidate
// behind a kept box has a thread): a candidate that no kept box overlaps by more than `iou` is kept, until K are.  Returns the
// kept count (uniform); their positions are in s.keep.  On entry, behind a barrier: slots 0..n) reset, then set.
// A barrier pair only when a box is kept (<= K of them), none for a suppressed candidate: every thread reads s.keepn while thread 0
// writes s.keep; s.keepn is updated between the two barriers, after every thread has read it and before any reads it again.
template <int N>
__device__ __forceinline__ int greedy_nms(NmsBoxes<N>& s, int n, int K, float iou, int tid) {
    for (int i = 0; i < n; ++i) {
        if (s.supp[i]) continue;          // uniform: written before the last barrier
        const int kept = s.keepn + 1;     // uniform read (updated after the barrier below), ONE read: ahead of the write to s.keep,
        if (tid == 0) s.keep[kept - 1] = i;      // which the compiler takes for one that may change s.keepn (the same object)
        if (kept >= K) { __syncthreads(); if (tid == 0) s.keepn = kept; __syncthreads(); break; }
        const float ix1 = s.x1[i], iy1 = s.y1[i], ix2 = s.x2[i], iy2 = s.y2[i], ia = s.area[i];
        const int j = i + 1 + tid;
        if (j < n) {
            const float ovr = box_iou1(ix1, iy1, ix2, iy2, ia, s.x1[j], s.y1[j], s.x2[j], s.y2[j], s.area[j]);
            if (ovr > iou) s.supp[j] = 1;
        }
        __syncthreads();
        if (tid == 0) s.keepn = kept;
        __syncthreads();
    }
    __syncthreads();
    return s.keepn;
}

// An output slot from the count on: 4 + 10 + 1 zeros (the slot's anchor index is the caller's)
__device__ __forceinline__ void write_empty_face(float* box, float* kps, float* score) {
    box[0] = box[1] = box[2] = box[3] = 0.f;
    for (int t = 0; t < 10; ++t) kps[t] = 0.f;
    *score = 0.f;
}

}  // namespace frp
