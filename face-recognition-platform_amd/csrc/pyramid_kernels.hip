// K3b: cross-scale merge + greedy NMS of the detection pyramid (BASELINE config 4), one workgroup per frame.
//
// The device form of pyramid.merge_scales: every scale's detections (decode_nms_kernel's output, already NMS-ed within the
// scale, coordinates of the resized image) are mapped back to frame pixels with ONE fp32 multiply per coordinate (x by
// rx = W / Ws, y by ry = H / Hs, the ratios computed on the host as launch_resize_u8 computes them; no clipping), taken in
// scale order, then detector order, sorted by score descending and put through the greedy +1-pixel-area NMS of decode_nms_kernel.
//
// Ordering is total: candidate slot c = s * P + j (scale s, detector row j < counts[s][b]) gets the unique key
//   (1 << 41) | (score bits << 9) | (511 - c)
// - scores are finite and >= 0, so their fp32 bits order as unsigned integers; ties go to the lower slot, which is numpy's
// stable argsort of -score; bit 41 marks a real entry, so a score of +0.0 still sorts above the padding (key 0).  The keys are
// bitonic-sorted in LDS.  All box arithmetic is fp32 with one rounding per operation (the file is built with
// -ffp-contract=off), so the result equals pyramid.merge_scales bit for bit.
//
// A few KB per frame: latency-bound, nothing here is tuned.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "frp_internal.h"

namespace frp {

#define PM_NT FRP_PYRAMID_MAX_CAND

// scalar members + select chains (a runtime-indexed kernel-argument array would live in scratch)
__device__ __forceinline__ float pick4(const float (&v)[FRP_PYRAMID_MAX_SCALES], int s) {
    return s == 0 ? v[0] : (s == 1 ? v[1] : (s == 2 ? v[2] : v[3]));
}

__global__ __launch_bounds__(PM_NT) void pyramid_merge_kernel(PyramidMergeParams p) {
    __shared__ unsigned long long keys[PM_NT];
    __shared__ float bx1[PM_NT], by1[PM_NT], bx2[PM_NT], by2[PM_NT], barea[PM_NT];
    __shared__ unsigned char supp[PM_NT];
    __shared__ int s_keepn;
    __shared__ int s_keep[FRP_MAX_FACES_CAP];

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int P = p.P, K = p.max_faces;

    // ---- candidates: slot tid = scale s, detector row j; live while j < counts[s][b] (clamped to the slots there are)
    int n = 0;
    for (int s = 0; s < p.S; ++s) n += min(max(p.counts[s * p.B + b], 0), P);     // uniform
    const int s_of = tid / P, j_of = tid - s_of * P;
    unsigned long long key = 0ull;
    if (s_of < p.S && j_of < min(max(p.counts[s_of * p.B + b], 0), P)) {
        const unsigned bits = __float_as_uint(p.scores[((long)s_of * p.B + b) * P + j_of]);
        key = (1ull << 41) | ((unsigned long long)bits << 9) | (unsigned long long)(PM_NT - 1 - tid);
    }
    keys[tid] = key;
    supp[tid] = 0;
    if (tid == 0) s_keepn = 0;
    __syncthreads();

    // ---- bitonic sort, descending
    for (int k2 = 2; k2 <= PM_NT; k2 <<= 1) {
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

    // ---- the sorted candidates' boxes in frame pixels
    if (tid < n) {
        const int c = PM_NT - 1 - (int)(keys[tid] & (PM_NT - 1));
        const int s = c / P;
        const float rx = pick4(p.rx, s), ry = pick4(p.ry, s);
        const float* q = p.boxes + (((long)s * p.B + b) * P + (c - s * P)) * 4;
        const float x1 = q[0] * rx, y1 = q[1] * ry, x2 = q[2] * rx, y2 = q[3] * ry;
        bx1[tid] = x1; by1[tid] = y1; bx2[tid] = x2; by2[tid] = y2;
        barea[tid] = (x2 - x1 + 1.0f) * (y2 - y1 + 1.0f);
    }
    __syncthreads();

    // ---- greedy NMS in key order; barrier only when a box is kept (decode_nms_kernel's loop)
    for (int i = 0; i < n; ++i) {
        if (supp[i]) continue;            // uniform: written before the last barrier
        if (tid == 0) s_keep[s_keepn] = i;
        const int kept = s_keepn + 1;     // uniform read (updated after the barrier below)
        if (kept >= K) { __syncthreads(); if (tid == 0) s_keepn = kept; __syncthreads(); break; }
        const float ix1 = bx1[i], iy1 = by1[i], ix2 = bx2[i], iy2 = by2[i], ia = barea[i];
        for (int j = i + 1 + tid; j < n; j += PM_NT) {
            const float xx1 = fmaxf(ix1, bx1[j]), yy1 = fmaxf(iy1, by1[j]);
            const float xx2 = fminf(ix2, bx2[j]), yy2 = fminf(iy2, by2[j]);
            const float w = fmaxf(0.0f, xx2 - xx1 + 1.0f), h = fmaxf(0.0f, yy2 - yy1 + 1.0f);
            const float inter = w * h;
            const float ovr = inter / ((ia + barea[j]) - inter);
            if (ovr > p.nms_iou) supp[j] = 1;
        }
        __syncthreads();
        if (tid == 0) s_keepn = kept;
        __syncthreads();
    }
    __syncthreads();
    const int kept = s_keepn;

    // ---- outputs: K slots per frame, zero from the count on, anchor -1 everywhere (a merged face has no anchor of one scale)
    if (tid < K) {
        float* ob = p.out_boxes + ((long)b * K + tid) * 4;
        float* ok = p.out_kps + ((long)b * K + tid) * 10;
        if (tid < kept) {
            const int i = s_keep[tid];
            const unsigned long long k = keys[i];
            const int c = PM_NT - 1 - (int)(k & (PM_NT - 1));
            const int s = c / P;
            const float rx = pick4(p.rx, s), ry = pick4(p.ry, s);
            const float* q = p.kps + (((long)s * p.B + b) * P + (c - s * P)) * 10;
            ob[0] = bx1[i]; ob[1] = by1[i]; ob[2] = bx2[i]; ob[3] = by2[i];
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                ok[2 * t] = q[2 * t] * rx;
                ok[2 * t + 1] = q[2 * t + 1] * ry;
            }
            p.out_scores[(long)b * K + tid] = __uint_as_float((unsigned)(k >> 9));
        } else {
            ob[0] = ob[1] = ob[2] = ob[3] = 0.f;
            for (int t = 0; t < 10; ++t) ok[t] = 0.f;
            p.out_scores[(long)b * K + tid] = 0.f;
        }
        if (p.out_anchor) p.out_anchor[(long)b * K + tid] = -1;
    }
    if (tid == 0) p.out_counts[b] = kept;
}

hipError_t launch_pyramid_merge(PyramidMergeParams p, hipStream_t stream) {
    if (p.S < 1 || p.S > FRP_PYRAMID_MAX_SCALES || p.P < 1 || p.P > FRP_MAX_FACES_CAP || p.S * p.P > FRP_PYRAMID_MAX_CAND ||
        p.max_faces < 1 || p.max_faces > FRP_MAX_FACES_CAP || p.B <= 0 || p.frame_h <= 0 || p.frame_w <= 0)
        return hipErrorInvalidValue;
    if (!p.boxes || !p.kps || !p.scores || !p.counts || !p.out_boxes || !p.out_kps || !p.out_scores || !p.out_counts)
        return hipErrorInvalidValue;
    for (int s = 0; s < FRP_PYRAMID_MAX_SCALES; ++s) {
        p.rx[s] = p.ry[s] = 1.0f;
        if (s >= p.S) continue;
        if (p.det_h[s] <= 0 || p.det_w[s] <= 0) return hipErrorInvalidValue;
        p.ry[s] = (float)p.frame_h / (float)p.det_h[s];          // as launch_resize_u8 and pyramid.merge_scales compute them
        p.rx[s] = (float)p.frame_w / (float)p.det_w[s];
    }
    hipLaunchKernelGGL(pyramid_merge_kernel, dim3(p.B), dim3(PM_NT), 0, stream, p);
    return hipGetLastError();
}

}  // namespace frp
