// The stand-alone kernel entry points of libfrp.so: one conv launch on host tensors (frp_conv2d_nhwc, frp_conv2d_f8: the parity
// tests' way to a single kernel; frp_debug_pyramid_merge: the cross-scale merge on host detections; frp_debug_fc_l2norm: the embedder's tail on host operands) and, in libfrp_lab.so only, the tuning hooks of include/frp_lab.h.
#include <hip/hip_runtime.h>

#include <cmath>

#include "frp.h"
#ifdef FRP_LAB
#include "frp_lab.h"
#endif
#include "frp_handle.h"

using namespace frp;

#ifdef FRP_LAB
namespace {
// the lab hooks' clock: `warm` launches, then `iters` of them between the handle's first two events; *ms = the time between the events
template <typename Launch>
hipError_t time_launches(frp_handle* h, int warm, int iters, Launch launch, float* ms) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < warm && e == hipSuccess; ++i) e = launch();
    if (e == hipSuccess) e = hipEventRecord(h->ev[0], h->stream);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch();
    if (e == hipSuccess) e = hipEventRecord(h->ev[1], h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, h->ev[0], h->ev[1]);
    return e;
}
}  // namespace
#endif

extern "C" {

namespace {   // (inside extern "C", where it always stood: its C name stays in the library's dynamic symbol table)
// frp_conv2d_nhwc / frp_conv_bench `flags` (include/frp.h) -> the kernel A/B bits and the tile class of one conv launch
void conv_route_from_abi_flags(int32_t flags, ConvParams& p) {
    p.dbg = ((flags >> 8) & 0xff) | ((flags & (1 << 19)) ? CONV_DBG_WINO_2D : 0) | ((flags & (1 << 20)) ? CONV_DBG_NO_C64 : 0) |
            ((flags & (1 << 21)) ? CONV_DBG_S2 : 0) | ((flags & (1 << 22)) ? CONV_DBG_C64_SAME_ORDER : 0) |
            (process_switches().c64_all ? CONV_DBG_C64_ALL : 0);
    p.small_m = (flags & (1 << 17)) ? 1 : (flags & ((1 << 18) | (1 << 16))) ? -1 : 0;     // (the Winograd kernel: never quarter tiles)
}
}  // namespace

int frp_conv2d_nhwc(frp_handle* h, const void* x, int32_t N, int32_t H, int32_t W, int32_t Cin, const void* w, int32_t Cout,
                    int32_t ksize, int32_t stride, const float* bias, const float* slope, const void* res, int32_t res_h,
                    int32_t res_w, int32_t act, int32_t flags, void* out) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!x || !w || !bias || !out || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !(ksize == 1 || ksize == 3) ||
        !(stride == 1 || stride == 2))
        return fail(h, FRP_ERR_INVALID, "bad conv arguments");
    const int pad = ksize / 2;
    const int Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    const bool up2 = flags & FRP_FLAG_RES_UP2;
    const size_t xb = (size_t)N * H * W * Cin * 2, wb = (size_t)Cout * ksize * ksize * Cin * 2;
    const size_t bb = (size_t)Cout * 4 * ((flags & FRP_FLAG_BORDER_BIAS) ? 9 : 1);
    const size_t ob = (size_t)N * Ho * Wo * Cout * ((flags & FRP_FLAG_OUT_F32) ? 4 : 2);
    const size_t rb = res ? (size_t)N * (up2 ? res_h : Ho) * (up2 ? res_w : Wo) * Cout * 2 : 0;
    ScopedBuf dx, dw, db, ds, dr, dout, dwino;
    FRPCHK(ensure(h, dx, xb));
    FRPCHK(ensure(h, dw, wb));
    FRPCHK(ensure(h, db, bb));
    FRPCHK(ensure(h, dout, ob));
    if (slope) FRPCHK(ensure(h, ds, (size_t)Cout * 4));
    if (res) FRPCHK(ensure(h, dr, rb));
    ConvParams p{};
    conv_route_from_abi_flags(flags, p);
    // flags bit 16: through the Winograd kernel (parity tests); an ineligible shape is an error, not a silent fallback
    const bool want_wino = (flags & (1 << 16)) != 0;
    std::vector<uint16_t> wimg;
    if (want_wino) {
        const bool shape_ok = conv3x3_wino_call_ok(N, H, W, Cin, Cout, ksize, stride, h->n_cu, res != nullptr, p.dbg);
        if (!shape_ok || (flags & (FRP_FLAG_OUT_F32 | FRP_FLAG_RES_UP2)))
            return fail(h, FRP_ERR_INVALID, "shape not covered by the Winograd kernel");
        wimg.resize(conv3x3_wino_image_bytes(Cin, Cout) / 2);
        build_wino_image((const uint16_t*)w, Cin, Cout, wimg.data());
        FRPCHK(ensure(h, dwino, wimg.size() * 2));
    }
    hipError_t e = hipMemcpyAsync(dx->p, x, xb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && want_wino) e = hipMemcpyAsync(dwino->p, wimg.data(), wimg.size() * 2, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dw->p, w, wb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db->p, bias, bb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && slope) e = hipMemcpyAsync(ds->p, slope, (size_t)Cout * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && res) e = hipMemcpyAsync(dr->p, res, rb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        p.x = (const _Float16*)dx->p; p.w = (const _Float16*)dw->p; p.bias = (const float*)db->p;
        p.slope = slope ? (const float*)ds->p : nullptr;
        p.res = res ? (const _Float16*)dr->p : nullptr;
        p.out = dout->p;
        p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.KS = ksize; p.stride = stride; p.act = act;
        p.flags = flags & (FRP_FLAG_BORDER_BIAS | FRP_FLAG_OUT_F32 | FRP_FLAG_RES_UP2);
        p.Hr = res_h; p.Wr = res_w;
        if (want_wino) p.wino_w = (const _Float16*)dwino->p;
        e = launch_conv(p, h->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout->p, ob, hipMemcpyDeviceToHost, h->stream);
    hipError_t e2 = hipStreamSynchronize(h->stream);      // (before the buffers go)
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? FRP_ERR_INVALID : FRP_ERR_HIP, std::string("conv2d: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("conv2d sync: ") + hipGetErrorString(e2));
    return FRP_OK;
}

int frp_conv2d_f8(frp_handle* h, const void* x8, int32_t N, int32_t H, int32_t W, int32_t Cin, const void* w8, int32_t Cout,
                  const float* wscale, const float* bias, const float* slope, const void* res16, int32_t act, int32_t flags,
                  float in_scale, float out_scale, void* out, void* out2_f8) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!x8 || !w8 || !wscale || !bias || !out || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0)
        return fail(h, FRP_ERR_INVALID, "bad conv arguments");
    const bool out8 = (flags & FRP_FLAG_OUT_FP8) != 0;
    const size_t xb = (size_t)N * H * W * Cin, wb = (size_t)Cout * 9 * Cin, on = (size_t)N * H * W * Cout;
    const size_t bb = (size_t)Cout * 4 * ((flags & FRP_FLAG_BORDER_BIAS) ? 9 : 1);
    ScopedBuf dx, dw, dws, db, ds, dr, dout, dout2;
    FRPCHK(ensure(h, dx, xb));
    FRPCHK(ensure(h, dw, wb));
    FRPCHK(ensure(h, dws, (size_t)Cout * 4));
    FRPCHK(ensure(h, db, bb));
    FRPCHK(ensure(h, dout, on * (out8 ? 1 : 2)));
    if (out2_f8) FRPCHK(ensure(h, dout2, on));
    if (slope) FRPCHK(ensure(h, ds, (size_t)Cout * 4));
    if (res16) FRPCHK(ensure(h, dr, on * 2));
    hipError_t e = hipMemcpyAsync(dx->p, x8, xb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dw->p, w8, wb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dws->p, wscale, (size_t)Cout * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db->p, bias, bb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && slope) e = hipMemcpyAsync(ds->p, slope, (size_t)Cout * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && res16) e = hipMemcpyAsync(dr->p, res16, on * 2, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        ConvParams p{};
        p.x = (const _Float16*)dx->p; p.w = (const _Float16*)dw->p; p.bias = (const float*)db->p;
        p.slope = slope ? (const float*)ds->p : nullptr;
        p.res = res16 ? (const _Float16*)dr->p : nullptr;
        p.out = dout->p;
        p.out2 = out2_f8 ? dout2->p : nullptr;
        p.wscale = (const float*)dws->p;
        p.in_scale = in_scale; p.out_scale = out_scale;
        p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.KS = 3; p.stride = 1; p.act = act;
        p.flags = (flags & (FRP_FLAG_BORDER_BIAS | FRP_FLAG_OUT_FP8)) | FRP_FLAG_F8;
        e = launch_conv(p, h->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout->p, on * (out8 ? 1 : 2), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && out2_f8) e = hipMemcpyAsync(out2_f8, dout2->p, on, hipMemcpyDeviceToHost, h->stream);
    hipError_t e2 = hipStreamSynchronize(h->stream);      // (before the buffers go)
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? FRP_ERR_INVALID : FRP_ERR_HIP, std::string("conv2d_f8: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("conv2d_f8 sync: ") + hipGetErrorString(e2));
    return FRP_OK;
}

int frp_conv_block64(frp_handle* h, const void* x, int32_t N, int32_t H, int32_t W, const void* w1, const float* bias1, const float* slope1,
                     int32_t act1, int32_t flags1, const void* w2, const float* bias2, const float* slope2, int32_t act2, void* out) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!x || !w1 || !bias1 || !w2 || !bias2 || !out || N <= 0 || H <= 0 || W <= 0) return fail(h, FRP_ERR_INVALID, "bad block arguments");
    if (!conv3x3_block64_variant(act1, flags1, slope1 != nullptr, act2, 0)) return fail(h, FRP_ERR_INVALID, "block epilogues not covered by the fused kernel");
    Block64Plan plan;
    if (!conv3x3_block64_plan(N, H, W, h->n_cu, &plan) || ((flags1 & FRP_FLAG_BORDER_BIAS) && (H < 2 || W < 2)))
        return fail(h, FRP_ERR_INVALID, "block shape out of the fused kernel's reach");
    const size_t tb = (size_t)N * H * W * 128, wb = (size_t)64 * 576 * 2, guard = 4096;
    const size_t b1 = (size_t)64 * 4 * ((flags1 & FRP_FLAG_BORDER_BIAS) ? 9 : 1);
    ScopedBuf dx, dw1, dw2, db1, db2, ds1, ds2, dout;
    FRPCHK(ensure(h, dx, tb + 2 * guard));
    FRPCHK(ensure(h, dout, tb + 2 * guard));
    FRPCHK(ensure(h, dw1, wb));
    FRPCHK(ensure(h, dw2, wb));
    FRPCHK(ensure(h, db1, b1));
    FRPCHK(ensure(h, db2, 256));
    if (slope1) FRPCHK(ensure(h, ds1, 256));
    if (slope2) FRPCHK(ensure(h, ds2, 256));
    std::vector<uint16_t> nan(guard, 0x7e00u), back(guard);          // (guard bytes front + guard bytes back)
    char *gx = (char*)dx->p, *go = (char*)dout->p;
    hipError_t e = hipMemcpyAsync(gx, nan.data(), guard, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(gx + guard + tb, nan.data(), guard, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(go, nan.data(), guard, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(go + guard + tb, nan.data(), guard, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(go + guard, 0x7e, tb, h->stream);          // (a pixel the launch does not write stays a NaN)
    if (e == hipSuccess) e = hipMemcpyAsync(gx + guard, x, tb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dw1->p, w1, wb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dw2->p, w2, wb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db1->p, bias1, b1, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db2->p, bias2, 256, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && slope1) e = hipMemcpyAsync(ds1->p, slope1, 256, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && slope2) e = hipMemcpyAsync(ds2->p, slope2, 256, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        Block64Params p{};
        p.x = (const _Float16*)(gx + guard); p.out = go + guard;
        p.w1 = (const _Float16*)dw1->p; p.bias1 = (const float*)db1->p; p.slope1 = slope1 ? (const float*)ds1->p : nullptr;
        p.w2 = (const _Float16*)dw2->p; p.bias2 = (const float*)db2->p; p.slope2 = slope2 ? (const float*)ds2->p : nullptr;
        p.N = N; p.H = H; p.W = W; p.act1 = act1; p.flags1 = flags1; p.act2 = act2;
        p.n_cu = h->n_cu;
        e = launch_conv3x3_block64(p, h->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, go + guard, tb, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(back.data(), go, guard, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync((char*)back.data() + guard, go + guard + tb, guard, hipMemcpyDeviceToHost, h->stream);
    hipError_t e2 = hipStreamSynchronize(h->stream);      // (before the buffers go)
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? FRP_ERR_INVALID : FRP_ERR_HIP, std::string("conv_block64: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("conv_block64 sync: ") + hipGetErrorString(e2));
    if (back != nan) return fail(h, FRP_ERR_HIP, "conv_block64: the launch wrote outside its output tensor");
    return FRP_OK;
}

int frp_debug_pyramid_merge(frp_handle* h, int32_t n_scales, const int32_t* det_hw, int32_t B, int32_t per_scale, int32_t frame_h,
                            int32_t frame_w, const float* boxes, const float* kps, const float* scores, const int32_t* counts,
                            int32_t max_faces, float nms_iou, float* out_boxes, float* out_kps, float* out_scores, int32_t* out_counts) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!det_hw || !boxes || !kps || !scores || !counts || !out_boxes || !out_kps || !out_scores || !out_counts)
        return fail(h, FRP_ERR_INVALID, "pyramid_merge: null argument");
    if (n_scales < 1 || n_scales > FRP_PYRAMID_MAX_SCALES || per_scale < 1 || per_scale > FRP_MAX_FACES_CAP ||
        n_scales * per_scale > FRP_PYRAMID_MAX_CAND || max_faces < 1 || max_faces > FRP_MAX_FACES_CAP || B < 1 || B > 1024 || frame_h < 1 ||
        frame_w < 1)
        return fail(h, FRP_ERR_INVALID, "pyramid_merge: 1..4 scales, per_scale and max_faces in 1..128, at most 512 candidates per frame");
    const int S = n_scales, P = per_scale, K = max_faces;
    PyramidMergeParams mp{};
    for (int s = 0; s < S; ++s) {
        mp.det_h[s] = det_hw[2 * s]; mp.det_w[s] = det_hw[2 * s + 1];
        if (mp.det_h[s] < 1 || mp.det_w[s] < 1) return fail(h, FRP_ERR_INVALID, "pyramid_merge: bad detector size");
        for (int b = 0; b < B; ++b) {
            const int32_t n = counts[s * B + b];
            if (n < 0 || n > P) return fail(h, FRP_ERR_INVALID, "pyramid_merge: count outside [0, per_scale]");
            for (int j = 0; j < n; ++j) {
                const float v = scores[((size_t)s * B + b) * P + j];
                if (!std::isfinite(v) || v < 0.f) return fail(h, FRP_ERR_INVALID, "pyramid_merge: score of a live row not finite or below 0");
            }
        }
    }
    const size_t in = (size_t)S * B * P, on = (size_t)B * K;
    ScopedBuf db, dk, ds, dc, ob, ok, os, oc;
    FRPCHK(ensure(h, db, in * 16));
    FRPCHK(ensure(h, dk, in * 40));
    FRPCHK(ensure(h, ds, in * 4));
    FRPCHK(ensure(h, dc, (size_t)S * B * 4));
    FRPCHK(ensure(h, ob, on * 16));
    FRPCHK(ensure(h, ok, on * 40));
    FRPCHK(ensure(h, os, on * 4));
    FRPCHK(ensure(h, oc, (size_t)B * 4));
    hipError_t e = hipMemcpyAsync(db->p, boxes, in * 16, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dk->p, kps, in * 40, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ds->p, scores, in * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dc->p, counts, (size_t)S * B * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        mp.boxes = (const float*)db->p; mp.kps = (const float*)dk->p; mp.scores = (const float*)ds->p; mp.counts = (const int32_t*)dc->p;
        mp.S = S; mp.B = B; mp.P = P; mp.max_faces = K;
        mp.frame_h = frame_h; mp.frame_w = frame_w;
        mp.nms_iou = nms_iou;
        mp.out_boxes = (float*)ob->p; mp.out_kps = (float*)ok->p; mp.out_scores = (float*)os->p; mp.out_counts = (int32_t*)oc->p;
        e = launch_pyramid_merge(mp, h->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out_boxes, ob->p, on * 16, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_kps, ok->p, on * 40, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_scores, os->p, on * 4, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_counts, oc->p, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream);
    hipError_t e2 = hipStreamSynchronize(h->stream);      // (before the buffers go)
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? FRP_ERR_INVALID : FRP_ERR_HIP, std::string("pyramid_merge: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("pyramid_merge sync: ") + hipGetErrorString(e2));
    return FRP_OK;
}

int frp_debug_fc_l2norm(frp_handle* h, const void* x_f16, const void* w_f16, const float* bias, int32_t cap, int32_t n, int32_t K, int32_t D,
                        int32_t mode, int32_t flags, float* emb, void* emb_f16, int32_t* n_cu, int32_t* host_factor) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!x_f16 || !w_f16 || !bias || !emb || !emb_f16) return fail(h, FRP_ERR_INVALID, "fc_l2norm: null argument");
    if (cap < 1 || n < 0 || n > cap || K < 8 || D < 8 || D > 1024 || mode < FRP_FC_DEVICE_COUNT || (flags & ~((1 << 17) | (1 << 18))))
        return fail(h, FRP_ERR_INVALID, "fc_l2norm: 0 <= n <= cap, cap >= 1, K >= 8, 8 <= D <= 1024, mode >= -1, flags bits 17 / 18 only");
    const bool dev_count = mode == FRP_FC_DEVICE_COUNT;
    const int N = dev_count ? cap : n;                      // the images the launches are made for
    const int fc_flags = FRP_FLAG_OUT_F32;
    // the launch decisions of a pass (net_program.cpp: pick_fc_splitk): host count -> the factor of n, device count -> -1 and slabs for the
    // capacity; a forced factor s stands where the host's would (s == 1: no split, the conv's own fp32 epilogue)
    FcSplitChoice c = fc_splitk_choice(N > 0 ? N : 1, 1, dev_count, D, K, fc_flags, false, h->n_cu);
    if (mode >= 2) c = {mode, (size_t)mode * (N > 0 ? N : 1) * D * 4};
    if (mode == 1) c = {0, 0};
    if (n_cu) *n_cu = h->n_cu;
    if (host_factor) *host_factor = conv_pick_ksplit(n, D, K, fc_flags, false, h->n_cu);
    const size_t xb = (size_t)cap * K * 2, wb = (size_t)D * K * 2, eb = (size_t)cap * D * 4;
    ScopedBuf dx, dw, db, dn, dws, de, de16;
    FRPCHK(ensure(h, dx, xb));
    FRPCHK(ensure(h, dw, wb));
    FRPCHK(ensure(h, db, (size_t)D * 4));
    FRPCHK(ensure(h, dn, 4));
    FRPCHK(ensure(h, de, eb));
    FRPCHK(ensure(h, de16, eb / 2));
    if (c.ws_bytes) FRPCHK(ensure(h, dws, c.ws_bytes));
    ConvParams p{};
    conv_route_from_abi_flags(flags, p);
    p.x = (const _Float16*)dx->p; p.w = (const _Float16*)dw->p; p.bias = (const float*)db->p;
    p.out = c.ksplit ? dws->p : de->p;
    p.N = N; p.H = 1; p.W = 1; p.Cin = K; p.Cout = D; p.KS = 1; p.stride = 1; p.act = FRP_ACT_NONE;
    p.flags = fc_flags;
    p.ksplit = c.ksplit;
    p.n_dev = dev_count ? (const int32_t*)dn->p : nullptr;
    p.n_cu = h->n_cu;
    p.in_scale = p.out_scale = 1.0f;
    if (N > 0) {                                            // what launch_conv would refuse is refused before anything is queued
        ConvParams probe = p;
        int ncu = 0;
        if (conv_derive(probe, &ncu) != hipSuccess) return fail(h, FRP_ERR_INVALID, "fc_l2norm: shape or split factor the conv launch refuses");
    }
    // 0xFF bytes (NaN patterns) where the launches write: a slab read without having been written, a row at or beyond n written, shows
    hipError_t e = hipMemsetAsync(de->p, 0xFF, eb, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(de16->p, 0xFF, eb / 2, h->stream);
    if (e == hipSuccess && c.ws_bytes) e = hipMemsetAsync(dws->p, 0xFF, c.ws_bytes, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dx->p, x_f16, xb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dw->p, w_f16, wb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db->p, bias, (size_t)D * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dn->p, &n, 4, hipMemcpyHostToDevice, h->stream);
    if (N > 0) {                                            // (run_embed: a call without faces launches nothing)
        if (e == hipSuccess) e = launch_conv(p, h->stream);
        if (e == hipSuccess)
            e = launch_l2norm((float*)de->p, (_Float16*)de16->p, N, D, h->stream, c.ksplit != 0 && c.ksplit != 1 ? (const float*)dws->p : nullptr,
                              c.ksplit, p.bias, p.n_dev, K, h->n_cu);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(emb, de->p, eb, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(emb_f16, de16->p, eb / 2, hipMemcpyDeviceToHost, h->stream);
    hipError_t e2 = hipStreamSynchronize(h->stream);      // (before the buffers go, and `n` on this frame)
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? FRP_ERR_INVALID : FRP_ERR_HIP, std::string("fc_l2norm: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("fc_l2norm sync: ") + hipGetErrorString(e2));
    return FRP_OK;
}

#ifdef FRP_LAB   // tuning hooks (include/frp_lab.h): only in libfrp_lab.so
int frp_conv_bench(frp_handle* h, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride,
                   int32_t act, int32_t flags, int32_t with_res, int32_t iters, float* ms_avg, uint64_t* stamps_out) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!ms_avg || iters <= 0 || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !(ksize == 1 || ksize == 3) ||
        !(stride == 1 || stride == 2))
        return fail(h, FRP_ERR_INVALID, "bad bench arguments");
    const int pad = ksize / 2;
    const int Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    const size_t xn = (size_t)N * H * W * Cin, wn = (size_t)Cout * ksize * ksize * Cin, on = (size_t)N * Ho * Wo * Cout;
    const bool f8 = (flags & FRP_FLAG_F8) != 0;          // fp8 operands: random fp16 bit patterns read as E4M3 bytes (timing only)
    ScopedBuf dx, dw, db, ds, dr, dout, dwino, dst;
    FRPCHK(ensure(h, dx, xn * 2));
    FRPCHK(ensure(h, dw, wn * 2));
    FRPCHK(ensure(h, db, (size_t)Cout * 4 * 9));
    FRPCHK(ensure(h, ds, (size_t)Cout * 4));
    FRPCHK(ensure(h, dr, on * 2));
    FRPCHK(ensure(h, dout, on * 4));
    float ms = 0.f;
    hipError_t e = launch_fill_random_f16((_Float16*)dx->p, (long)xn, 1u, 1.0f, h->stream);
    if (e == hipSuccess) e = launch_fill_random_f16((_Float16*)dw->p, (long)wn, 2u, 1.0f / sqrtf((float)(ksize * ksize * Cin)), h->stream);
    if (e == hipSuccess) e = launch_fill_random_f16((_Float16*)dr->p, (long)on, 3u, 1.0f, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(db->p, 0, (size_t)Cout * 36, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ds->p, 0, (size_t)Cout * 4, h->stream);
    ConvParams p{};
    p.x = (const _Float16*)dx->p; p.w = (const _Float16*)dw->p; p.bias = (const float*)db->p; p.slope = (const float*)ds->p;
    p.res = with_res ? (const _Float16*)dr->p : nullptr; p.out = dout->p;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.KS = ksize; p.stride = stride; p.act = act;
    p.flags = flags & (FRP_FLAG_BORDER_BIAS | FRP_FLAG_OUT_F32 | FRP_FLAG_F8 | FRP_FLAG_OUT_FP8);
    if (f8) {                                         // unit scales in the slope buffer's neighbour: reuse the bias buffer (zeros) + 1
        p.wscale = (const float*)ds->p;                // zeros: products vanish, timing is unaffected
        p.in_scale = p.out_scale = 1.0f;
        if (!(flags & FRP_FLAG_OUT_FP8)) p.out2 = dr->p;   // conv2-style: fp16 out + fp8 copy (residual buffer doubles as the copy target when unused)
        if (with_res) p.out2 = nullptr;
    }
    conv_route_from_abi_flags(flags, p);
    const bool wino_shape = conv3x3_wino_call_ok(N, H, W, Cin, Cout, ksize, stride, h->n_cu, with_res != 0, p.dbg);
    if ((flags & (1 << 16)) && wino_shape) {     // Winograd kernel: a random weight image (timing only)
        const size_t ib = conv3x3_wino_image_bytes(Cin, Cout);
        if (ensure(h, dwino, ib) == FRP_OK) {
            e = launch_fill_random_f16((_Float16*)dwino->p, (long)(ib / 2), 5u, 1.0f / sqrtf((float)(9 * Cin)), h->stream);
            p.wino_w = (const _Float16*)dwino->p;
        }
    }
    if (stamps_out && ensure(h, dst, 256 * 8 * 8) == FRP_OK) {
        (void)hipMemsetAsync(dst->p, 0, 256 * 8 * 8, h->stream);
        p.stamps = (unsigned long long*)dst->p;
    }
    if (flags & (1 << 23)) {                    // the fused residual block (conv3x3_block64.hip) this conv1 opens: conv1 (act, border bias), conv2 + x
        Block64Params bp{};                     // (+ ReLU behind a ReLU conv1: the detector's block; none behind PReLU: the embedder's)
        bp.x = p.x; bp.out = p.out; bp.w1 = bp.w2 = p.w; bp.bias1 = bp.bias2 = p.bias; bp.slope1 = p.slope;
        bp.N = N; bp.H = H; bp.W = W; bp.act1 = act; bp.flags1 = flags & FRP_FLAG_BORDER_BIAS; bp.act2 = act == FRP_ACT_RELU ? FRP_ACT_RELU : FRP_ACT_NONE;
        bp.n_cu = h->n_cu;
        if (Cin != 64 || Cout != 64 || ksize != 3 || stride != 1) e = hipErrorInvalidValue;
        if (e == hipSuccess) e = time_launches(h, 2, iters, [&] { return launch_conv3x3_block64(bp, h->stream); }, &ms);
    } else
    if (e == hipSuccess) e = time_launches(h, 2, iters, [&] { return launch_conv(p, h->stream); }, &ms);
    if (e == hipSuccess && stamps_out && p.stamps) e = hipMemcpy(stamps_out, p.stamps, 256 * 8 * 8, hipMemcpyDeviceToHost);
    (void)hipStreamSynchronize(h->stream);      // (before the buffers go)
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("conv_bench: ") + hipGetErrorString(e));
    *ms_avg = ms / iters;
    return FRP_OK;
}

int frp_mfma_peak(frp_handle* h, int32_t waves_per_simd, int32_t iters, float* tflops) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    // waves_per_simd 1..8: register-operand loop.  16*r + 2 (r = 4, 3, 2): the conv k-step mix - 8 waves per CU,
    // r ds_read_b128 per 4 MFMAs - one 512-thread block per CU
    const int lds_reads = waves_per_simd >> 4;
    if (lds_reads) waves_per_simd &= 15;
    if (!tflops || iters <= 0 || waves_per_simd < 1 || waves_per_simd > 8 || (lds_reads && (waves_per_simd != 2 || lds_reads < 2 || lds_reads > 4)))
        return fail(h, FRP_ERR_INVALID, "bad arguments");
    const int blocks = lds_reads ? h->n_cu : 256 * waves_per_simd;   // 256 CUs x (4 waves per block = one per SIMD)
    ScopedBuf src, dst;
    FRPCHK(ensure(h, src, 3 * 384 * 128));
    FRPCHK(ensure(h, dst, (size_t)blocks * 512 * 4));
    float ms = 0.f;
    hipError_t e = launch_fill_random_f16((_Float16*)src->p, 3 * 384 * 64, 7u, 1.0f, h->stream);
    if (e == hipSuccess)
        e = time_launches(h, 1, 1, [&] {
            return lds_reads ? launch_mfma_lds((const _Float16*)src->p, (float*)dst->p, blocks, lds_reads, iters, h->stream)
                             : launch_mfma_peak((const _Float16*)src->p, (float*)dst->p, blocks, iters, h->stream);
        }, &ms);
    (void)hipStreamSynchronize(h->stream);      // (before the buffers go)
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("mfma_peak: ") + hipGetErrorString(e));
    *tflops = (float)((double)blocks * (lds_reads ? 8.0 * 16 : 4.0 * 4) * iters * 32768.0 / (ms * 1e-3) / 1e12);
    return FRP_OK;
}

int frp_kstep_lab(frp_handle* h, int32_t variant, int32_t iters, float* tflops) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!tflops || iters <= 0) return fail(h, FRP_ERR_INVALID, "bad arguments");
    const int blocks = h->n_cu;
    ScopedBuf src, dst;
    FRPCHK(ensure(h, src, 4u << 20));        // LDS image + the 4 MiB window the lab's LDS-DMA variants read
    FRPCHK(ensure(h, dst, (size_t)blocks * 512 * 4));
    float ms = 0.f;
    hipError_t e = launch_fill_random_f16((_Float16*)src->p, 2L << 20, 7u, 1.0f, h->stream);
    if (e == hipSuccess)
        e = time_launches(h, 1, 1, [&] { return launch_kstep_lab((const _Float16*)src->p, (float*)dst->p, blocks, variant, iters, h->stream); }, &ms);
    (void)hipStreamSynchronize(h->stream);      // (before the buffers go)
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? FRP_ERR_INVALID : FRP_ERR_HIP, std::string("kstep_lab: ") + hipGetErrorString(e));
    // fp8 variants (bit 10): 8 MFMAs of 32x32x64 per wave and step = twice the FLOPs of the fp16 step
    *tflops = (float)((double)blocks * kstep_lab_waves(variant) * 16 * kstep_lab_steps_per_iter(variant) * iters * 32768.0 * ((variant & 1024) ? 2.0 : 1.0) /
                      (ms * 1e-3) / 1e12);
    return FRP_OK;
}
#endif  // FRP_LAB

}  // extern "C"
