// The detection pyramid's own kernels (BASELINE config 4): the u8 bilinear resize that makes the scales (resize_u8_kernel, at the
// end of the file) and K3b, the cross-scale merge + greedy NMS of their detections, one workgroup per frame.
//
// K3b is the device form of pyramid.merge_scales: every scale's detections (decode_nms_kernel's output, already NMS-ed within the
// scale, coordinates of the resized image) are mapped back to frame pixels with ONE fp32 multiply per coordinate (x by
// rx = W / Ws, y by ry = H / Hs, the ratios computed on the host as launch_resize_u8 computes them; no clipping), taken in
// scale order, then detector order, sorted by score descending and put through the greedy +1-pixel-area NMS that
// decode_nms_kernel runs (box_nms.h: sort_keys_desc, greedy_nms; this file keeps the candidate keys, the rx / ry mapping and
// the outputs).
//
// Ordering is total: candidate slot c = s * P + j (scale s, detector row j < counts[s][b]) gets the unique key
//   (1 << 41) | (score bits << 9) | (511 - c)
// - scores are finite and >= 0, so their fp32 bits order as unsigned integers; ties go to the lower slot, which is numpy's
// stable argsort of -score; bit 41 marks a real entry, so a score of +0.0 still sorts above the padding (key 0).  All box
// arithmetic is fp32 with one rounding per operation (the file is built with -ffp-contract=off, as every file that includes
// box_nms.h), so the result equals pyramid.merge_scales bit for bit.
//
// A few KB per frame: latency-bound, nothing here is tuned.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "box_nms.h"
#include "frp_internal.h"

namespace frp {

#define PM_NT FRP_PYRAMID_MAX_CAND

// scalar members + select chains (a runtime-indexed kernel-argument array would live in scratch)
__device__ __forceinline__ float pick4(const float (&v)[FRP_PYRAMID_MAX_SCALES], int s) {
    return s == 0 ? v[0] : (s == 1 ? v[1] : (s == 2 ? v[2] : v[3]));
}

__global__ __launch_bounds__(PM_NT) void pyramid_merge_kernel(PyramidMergeParams p) {
    // (the alignment puts `keys` in front of `nms`; behind it this compiler pads `nms`: 15376 B of LDS instead of 15368.  Nothing
    // depends on the order but that figure, which tests/test_box_nms_host.py holds)
    __shared__ alignas(32) unsigned long long keys[PM_NT];
    __shared__ NmsBoxes<PM_NT> nms;

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
    nms.reset(tid);
    __syncthreads();

    sort_keys_desc<PM_NT>(keys, tid);

    // ---- the sorted candidates' boxes in frame pixels, greedy NMS in key order
    if (tid < n) {
        const int c = PM_NT - 1 - (int)(keys[tid] & (PM_NT - 1));
        const int s = c / P;
        const float rx = pick4(p.rx, s), ry = pick4(p.ry, s);
        const float* q = p.boxes + (((long)s * p.B + b) * P + (c - s * P)) * 4;
        nms.set(tid, q[0] * rx, q[1] * ry, q[2] * rx, q[3] * ry);
    }
    __syncthreads();
    const int kept = greedy_nms<PM_NT>(nms, n, K, p.nms_iou, tid);

    // ---- outputs: K slots per frame, zero from the count on, anchor -1 everywhere (a merged face has no anchor of one scale)
    if (tid < K) {
        float* ob = p.out_boxes + ((long)b * K + tid) * 4;
        float* ok = p.out_kps + ((long)b * K + tid) * 10;
        if (tid < kept) {
            const int i = nms.keep[tid];
            const unsigned long long k = keys[i];
            const int c = PM_NT - 1 - (int)(k & (PM_NT - 1));
            const int s = c / P;
            const float rx = pick4(p.rx, s), ry = pick4(p.ry, s);
            const float* q = p.kps + (((long)s * p.B + b) * P + (c - s * P)) * 10;
            ob[0] = nms.x1[i]; ob[1] = nms.y1[i]; ob[2] = nms.x2[i]; ob[3] = nms.y2[i];
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                ok[2 * t] = q[2 * t] * rx;
                ok[2 * t + 1] = q[2 * t + 1] * ry;
            }
            p.out_scores[(long)b * K + tid] = __uint_as_float((unsigned)(k >> 9));
        } else {
            write_empty_face(ob, ok, p.out_scores + (long)b * K + tid);
        }
        if (p.out_anchor) p.out_anchor[(long)b * K + tid] = -1;
    }
    if (tid == 0) p.out_counts[b] = kept;
}

// Bilinear down/up-scale of u8 frames for the multi-scale pyramid (BASELINE config 4).  Pixel centres:
// src = (dst + 0.5) * (S / D) - 0.5, clamped to the image; fp32 lerp in x then y with one rounding per
// operation (this file is built with -ffp-contract=off), result floor(v + 0.5) -> u8.
__global__ __launch_bounds__(256) void resize_u8_kernel(const uint8_t* __restrict__ src, int B, int H, int W,
                                                        uint8_t* __restrict__ dst, int Hs, int Ws, float ry, float rx) {
    const long total = (long)B * Hs * Ws;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Ws);
        const long r = i / Ws;
        const int y = (int)(r % Hs);
        const int b = (int)(r / Hs);
        float sy = ((float)y + 0.5f) * ry - 0.5f, sx = ((float)x + 0.5f) * rx - 0.5f;
        sy = fminf(fmaxf(sy, 0.0f), (float)(H - 1));
        sx = fminf(fmaxf(sx, 0.0f), (float)(W - 1));
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + 1 < H ? y0 + 1 : H - 1, x1 = x0 + 1 < W ? x0 + 1 : W - 1;
        const float fy = sy - (float)y0, fx = sx - (float)x0;
        const uint8_t* p00 = src + (((long)b * H + y0) * W + x0) * 3;
        const uint8_t* p01 = src + (((long)b * H + y0) * W + x1) * 3;
        const uint8_t* p10 = src + (((long)b * H + y1) * W + x0) * 3;
        const uint8_t* p11 = src + (((long)b * H + y1) * W + x1) * 3;
        uint8_t* o = dst + i * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = (float)p00[c] * (1.0f - fx) + (float)p01[c] * fx;
            const float bot = (float)p10[c] * (1.0f - fx) + (float)p11[c] * fx;
            const float v = top * (1.0f - fy) + bot * fy;
            o[c] = (uint8_t)fminf(fmaxf(floorf(v + 0.5f), 0.0f), 255.0f);
        }
    }
}

hipError_t launch_resize_u8(const uint8_t* src, int B, int H, int W, uint8_t* dst, int Hs, int Ws, hipStream_t stream) {
    if (!src || !dst || B <= 0 || H <= 0 || W <= 0 || Hs <= 0 || Ws <= 0) return hipErrorInvalidValue;
    const long total = (long)B * Hs * Ws;
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(resize_u8_kernel, dim3(grid), dim3(256), 0, stream, src, B, H, W, dst, Hs, Ws,
                       (float)H / (float)Hs, (float)W / (float)Ws);
    return hipGetLastError();
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
    static_assert(PM_NT == FRP_PYRAMID_MAX_CAND && (PM_NT & (PM_NT - 1)) == 0, "one thread per candidate slot, a power of two of them");
    hipLaunchKernelGGL(pyramid_merge_kernel, dim3(p.B), dim3(PM_NT), 0, stream, p);      // PM_NT threads: sort_keys_desc / greedy_nms<PM_NT>
    return hipGetLastError();
}

}  // namespace frp
