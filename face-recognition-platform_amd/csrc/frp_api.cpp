// C-ABI host runtime of libfrp.so: handle, weight/program blob, gallery snapshots, the
// detect -> align -> embed -> match pipeline on one HIP stream, per-stage HIP-event timing.
// Interface and the reference call sites each entry point replaces: include/frp.h.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: the library opens librccl at first use (frp_dist_*)
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#include <thread>
#include <atomic>

#include "frp.h"
#ifdef FRP_LAB
#include "frp_lab.h"
#endif
#include "frp_blob.h"
#include "frp_internal.h"
#include "frp_handle.h"
#include "jpeg_host.h"

using namespace frp;

// The only readers of the environment (besides the JPEG size limit, jpeg_host.cpp: jpeg_max_pixels); the switches: frp_internal.h
#define FRP_WINO_MIN_FACES 128   // default of Switches::wino_min_faces (run_embed)
Switches frp::read_switches() {
    auto set = [](const char* n) { return getenv(n) ? 1 : 0; };
    const char *sm = getenv("FRP_SMALL_M"), *wm = getenv("FRP_WINO_MIN_FACES");
    Switches s{};
    s.small_m = !sm ? 0 : (sm[0] == '0' ? -1 : 1);
    s.wino_min_faces = wm ? atoi(wm) : FRP_WINO_MIN_FACES;
    s.s2 = set("FRP_S2"); s.host_count = set("FRP_HOST_COUNT"); s.match_v1 = set("FRP_MATCH_V1");
    s.no_fused_stem12 = set("FRP_NO_FUSED_STEM12"); s.no_fused_stem = set("FRP_NO_FUSED_STEM");
    s.no_emb_stem = set("FRP_NO_EMB_STEM"); s.no_stem_fuse = set("FRP_NO_STEM_FUSE");
    s.no_wino = set("FRP_NO_WINO"); s.no_kconcat = set("FRP_NO_KCONCAT");
    return s;
}

const ProcessSwitches& frp::process_switches() {
    static const ProcessSwitches s = [] {
        const char* jh = getenv("FRP_JPEG_DEVICE_HUFFMAN");
        return ProcessSwitches{getenv("FRP_NO_GRAPH") != nullptr, getenv("FRP_C64_ALL") != nullptr, !jh ? 0 : (jh[0] == '0' ? -1 : 1)};
    }();
    return s;
}

namespace {

// librccl, opened at first use (frp_dist_*: the gallery all-gather; a process that never goes multi-GPU does not load it)
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
};
Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.lib) break;
        }
        if (!r.lib) { r.err = std::string("librccl not found: ") + (dlerror() ? dlerror() : "?"); return; }
        r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.lib, "ncclGetUniqueId");
        r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.lib, "ncclCommInitRank");
        r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
        r.AllGather = (decltype(r.AllGather))dlsym(r.lib, "ncclAllGather");
        r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.lib, "ncclGetErrorString");
        if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.GetErrorString) r.err = "librccl lacks an expected symbol";
    });
    return r;
}

float logit_threshold(float t) {
    if (!(t > 0.f)) return -INFINITY;
    if (t >= 1.f) return INFINITY;
    return (float)std::log((double)t / (1.0 - (double)t));
}

void rec(frp_handle* h, int which) {
    if (h->cfg.profile) (void)hipEventRecord(h->ev[which], h->stream);
}

int upload_frames(frp_handle* h, const uint8_t* bgr, int B, int H, int W, int64_t row_stride) {
    if (!bgr || B <= 0 || H <= 0 || W <= 0 || row_stride < (int64_t)W * 3) return fail(h, FRP_ERR_INVALID, "bad frame arguments");
    if (B > 1024) return fail(h, FRP_ERR_INVALID, "batch too large (max 1024 frames per call)");
    FRPCHK(ensure(h, h->frames, (size_t)B * H * W * 3));
    rec(h, EV_START);
    HIPCHK(h, hipMemcpy2DAsync(h->frames.p, (size_t)W * 3, bgr, (size_t)row_stride, (size_t)W * 3, (size_t)B * H,
                               hipMemcpyHostToDevice, h->stream));
    rec(h, EV_H2D);
    h->rB = B; h->rH = H; h->rW = W;
    h->dH = H; h->dW = W; h->det_scaled = false;
    h->canvas_h = round_up(H, 32);
    h->canvas_w = round_up(W, 32);
    return FRP_OK;
}

// choose the detector source: the resident frames (Hs,Ws == frame size) or a bilinear resize of them
int select_det_source(frp_handle* h, int Hs, int Ws) {
    if (h->rB <= 0) return fail(h, FRP_ERR_INVALID, "no resident frames (call frp_upload_frames)");
    if (Hs <= 0 || Ws <= 0 || Hs > 16384 || Ws > 16384) return fail(h, FRP_ERR_INVALID, "bad detector size");
    if (Hs == h->rH && Ws == h->rW) {
        h->det_scaled = false;
    } else {
        FRPCHK(ensure(h, h->scaled, (size_t)h->rB * Hs * Ws * 3));
        hipError_t e = launch_resize_u8((const uint8_t*)h->frames.p, h->rB, h->rH, h->rW, (uint8_t*)h->scaled.p, Hs, Ws, h->stream);
        if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("resize: ") + hipGetErrorString(e));
        h->det_scaled = true;
    }
    h->dH = Hs; h->dW = Ws;
    h->canvas_h = round_up(Hs, 32);
    h->canvas_w = round_up(Ws, 32);
    return FRP_OK;
}

int ensure_results(frp_handle* h, int B, int K) {
    const size_t s = (size_t)B * K;
    FRPCHK(ensure(h, h->boxes, s * 4 * 4));
    FRPCHK(ensure(h, h->kps, s * 10 * 4));
    FRPCHK(ensure(h, h->scores, s * 4));
    FRPCHK(ensure(h, h->anchor, s * 4));
    FRPCHK(ensure(h, h->counts, (size_t)B * 4));
    FRPCHK(ensure(h, h->face_slot, s * 4));
    FRPCHK(ensure(h, h->nfaces, 16));
    return FRP_OK;
}

int run_detect(frp_handle* h, const Switches& sw, int K, float det_thresh, float nms_iou, uint32_t flags) {
    if (!h->have_weights) return fail(h, FRP_ERR_NO_WEIGHTS, "no weights loaded");
    if (h->rB <= 0) return fail(h, FRP_ERR_INVALID, "no resident frames (call frp_upload_frames)");
    if (K <= 0 || K > FRP_MAX_FACES_CAP) return fail(h, FRP_ERR_INVALID, "max_faces out of range");
    const int B = h->rB, Hc = h->canvas_h, Wc = h->canvas_w;
    // The detector's first layer reads the u8 frames directly (fused normalise + conv) whenever
    // the program starts with the standard 3x3 s2 3->32 stem; FRP_NO_FUSED_STEM keeps the
    // two-kernel path (preprocess to an NHWC8 blob, then the generic conv) for A/B runs.
    const bool fused = h->det.det_stem && !sw.no_fused_stem;
    FRPCHK(plan_net(h, h->det, B, Hc, Wc, fused));
    FRPCHK(ensure_results(h, B, K));
    hipError_t e = hipSuccess;
    StemParams sp{};
    const uint8_t* dsrc = h->det_scaled ? (const uint8_t*)h->scaled.p : (const uint8_t*)h->frames.p;
    if (fused) {
        sp.frames = dsrc;
        sp.B = B; sp.H = h->dH; sp.W = h->dW;
        sp.row_stride = (long)h->dW * 3; sp.frame_stride = (long)h->dH * h->dW * 3;
        sp.Hc = Hc; sp.Wc = Wc; sp.Ho = Hc / 2; sp.Wo = Wc / 2;
        sp.rgb_in = (flags & FRP_FLAG_RGB) ? 1 : 0;
    } else {
        e = launch_preprocess(dsrc, B, h->dH, h->dW, (long)h->dW * 3, (long)h->dH * h->dW * 3,
                              (_Float16*)h->det.bufs[h->det.in_buf].p, Hc, Wc, (flags & FRP_FLAG_RGB) ? 1 : 0, h->stream);
        if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("preprocess: ") + hipGetErrorString(e));
    }
    rec(h, EV_PRE);
    // Winograd family for the detector's wide 128 / 256-channel layers: from two rounds of 8 x 30 tiles on its stride-8 maps on
    // (1080p: four frames; below that the direct family with its quarter tiles and weight prefetch: single-image latency)
    const bool det_wino = (long)B * (Hc / 8) * (Wc / 8) >= 2L * 240 * (h->n_cu > 0 ? h->n_cu : 256);
    FRPCHK(run_net(h, sw, h->det, B, Hc, Wc, &h->ctr.det_conv_flops, &h->ctr.det_conv_launches, fused ? &sp : nullptr, nullptr, det_wino));
    rec(h, EV_DET);
    DecodeParams dp{};
    for (int l = 0; l < 3; ++l) {
        const int bi = (int)h->hdr.det_head_buf[l];
        dp.head[l] = (const _Float16*)h->det.bufs[bi].p;
        dp.hl[l] = h->det.dims[bi].h;
        dp.wl[l] = h->det.dims[bi].w;
        if (h->det.dims[bi].c != 32) return fail(h, FRP_ERR_BLOB, "detector head must have 32 channels");
    }
    dp.B = B;
    dp.max_faces = K;
    const bool forced = flags & FRP_FLAG_FORCED_K;
    dp.logit_thresh = forced ? -INFINITY : logit_threshold(det_thresh);
    dp.nms_iou = forced ? 2.0f : nms_iou;
    dp.boxes = (float*)h->boxes.p; dp.kps = (float*)h->kps.p; dp.scores = (float*)h->scores.p;
    dp.anchor = (int32_t*)h->anchor.p; dp.counts = (int32_t*)h->counts.p;
    {
        size_t anchors = 0;
        for (int l = 0; l < 3; ++l) anchors += (size_t)dp.hl[l] * dp.wl[l] * 2;
        FRPCHK(ensure(h, h->dense_logits, (size_t)B * anchors * 2));
        dp.logits = (_Float16*)h->dense_logits.p;
    }
    e = launch_decode_nms(dp, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("decode_nms: ") + hipGetErrorString(e));
    e = launch_compact_faces((const int32_t*)h->counts.p, B, K, (int32_t*)h->face_slot.p, (int32_t*)h->nfaces.p, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("compact_faces: ") + hipGetErrorString(e));
    rec(h, EV_DEC);
    h->last_B = B;
    h->last_K = K;
    return FRP_OK;
}

// chips for n faces are in emb.bufs[in]; run embedder + l2norm (+ fp16 copy for the matcher)
// Kernel family of an embedder pass.  The Winograd kernel (256 x 128 tiles only) pays from about 128 faces up (end to end,
// tools/family_crossover.py: 80 slots 5.06 vs 4.62 ms, 100 / 128 slots equal, 160 slots 7.58 vs 7.78); below, the direct kernels in
// quarter tiles are up to 2.6 x faster per layer (tools/small_m_probe.py).  The two families differ in the last
// bits (1 - cos 1.6e-6), so the choice is made ONCE per call, from a count that does not depend on what the detector
// found: `family_count` = the slots of the call (B x K of a process call, whether the face count stays on the device or
// not; the faces handed to the embed / finish calls).  Within a family every tile size gives the same bits, so a face's
// embedding depends on the call's slot count being above or below FRP_WINO_MIN_FACES and on nothing else in the batch.
int run_embed(frp_handle* h, const Switches& sw, int n, const int32_t* n_dev = nullptr, int family_count = -1) {
    if (n <= 0) return FRP_OK;
    if (family_count < 0) family_count = n;
    FcSplitK fc;                          // the FC wrote split-K slabs: l2norm reduces them
    FRPCHK(run_net(h, sw, h->emb, n, FRP_CHIP, FRP_CHIP, &h->ctr.emb_conv_flops, &h->ctr.emb_conv_launches, nullptr, n_dev,
                   family_count >= sw.wino_min_faces, &fc));
    rec(h, EV_EMB);
    const int mpad = round_up(n, 32);
    FRPCHK(ensure(h, h->q16, (size_t)mpad * FRP_EMB_DIM * 2));
    HIPCHK(h, hipMemsetAsync(h->q16.p, 0, (size_t)mpad * FRP_EMB_DIM * 2, h->stream));
    hipError_t e = launch_l2norm((float*)h->emb.bufs[h->hdr.emb_out_buf].p, (_Float16*)h->q16.p, n, FRP_EMB_DIM, h->stream,
                                 fc.ksplit != 0 && fc.ksplit != 1 ? (const float*)h->splitk_ws.p : nullptr, fc.ksplit, fc.bias, n_dev, fc.ktot,
                                 h->n_cu);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("l2norm: ") + hipGetErrorString(e));
    rec(h, EV_L2);
    return FRP_OK;
}

// q16 [mpad,512] holds n unit queries -> best_idx/best_cos [n]
int run_match(frp_handle* h, const Switches& sw, int n, float* all_scores_dev, const int32_t* n_dev = nullptr) {
    if (n <= 0) return FRP_OK;
    if (h->g_rows <= 0) return fail(h, FRP_ERR_NO_GALLERY, "gallery is empty");
    const int mpad = round_up(n, 32);
    MatchParams mp{};
    mp.gallery = (const _Float16*)h->gallery.p;
    mp.N = h->g_rows;
    mp.q = (const _Float16*)h->q16.p;
    mp.M = n;
    mp.Mpad = mpad;
    mp.n_wg = match_num_workgroups(h->g_rows);
    FRPCHK(ensure(h, h->part_cos, (size_t)mp.n_wg * mpad * 4));
    FRPCHK(ensure(h, h->part_idx, (size_t)mp.n_wg * mpad * 4));
    FRPCHK(ensure(h, h->best_cos, (size_t)mpad * 4));
    FRPCHK(ensure(h, h->best_idx, (size_t)mpad * 4));
    mp.part_cos = (float*)h->part_cos.p; mp.part_idx = (int32_t*)h->part_idx.p;
    mp.best_cos = (float*)h->best_cos.p; mp.best_idx = (int32_t*)h->best_idx.p;
    mp.all_scores = all_scores_dev;
    mp.n_dev = n_dev;
    hipError_t e = launch_match(mp, sw.match_v1 != 0, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("match: ") + hipGetErrorString(e));
    h->ctr.match_bytes += (double)h->g_rows * FRP_EMB_DIM * 2;
    h->ctr.match_launches += 1;
    return FRP_OK;
}

// align + embed + match for the faces listed in h->kps / h->counts / h->face_slot (device), always from
// the full-resolution resident frames.  n_known >= 0: face count known on the host.
int resolve_count(frp_handle* h);
int run_faces(frp_handle* h, const Switches& sw, int K, int n_known, uint32_t flags) {
    const int B = h->rB;
    int n;
    // a device-count pass that nobody fetched or synchronised yet (two process calls queued back to back): its count and its
    // counter corrections live in single slots (h_nfaces, pend_*) this pass is about to reuse - settle it first
    if (h->last_nfaces < 0) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        FRPCHK(resolve_count(h));
    }
    // Threshold mode (the reference's loop, routes/camera.py:232-259): how many faces the detector kept is known on the
    // device only.  It STAYS there: align, the embedder's kernels, the l2norm and the matcher are launched for the capacity
    // B x K and read the count from device memory (grids sized for the capacity; workgroups beyond the real tiles leave at
    // once), so the pipeline has no host round trip.  The host learns the count with the results (frp_fetch_results).
    // FRP_HOST_COUNT keeps the former path (copy the count, wait, launch for exactly n) for A/B runs - both give the
    // same bits.  More than FRP_MATCH_TOP1_MAX slots: the per-tile matcher has no device-count form, former path.
    // (FRP_MATCH_V1 pins the per-tile matcher for A/B runs: it has no device-count form either)
    const bool dev_count = n_known < 0 && round_up(B * K, 32) <= FRP_MATCH_TOP1_MAX && !sw.host_count && !sw.match_v1;
    const int32_t* n_dev = nullptr;
    if (n_known >= 0) {
        n = n_known;
    } else if (dev_count) {
        n = B * K;
        n_dev = (const int32_t*)h->nfaces.p;
        HIPCHK(h, hipMemcpyAsync(h->h_nfaces, h->nfaces.p, 4, hipMemcpyDeviceToHost, h->stream));   // read after the next wait
    } else {
        HIPCHK(h, hipMemcpyAsync(h->h_nfaces, h->nfaces.p, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        n = *h->h_nfaces;
        if (n < 0 || n > B * K) return fail(h, FRP_ERR_HIP, "corrupt face count");
    }
    h->last_nfaces = n_dev ? -1 : n;          // -1: pending, resolved by the next call that waits for the stream
    h->last_cap = n;
    h->last_matched = false;
    const double flops0 = h->ctr.emb_conv_flops, f8flops0 = h->ctr.f8_conv_flops;
    if (n > 0) {
        FRPCHK(plan_net(h, h->emb, n, FRP_CHIP, FRP_CHIP));
        AlignParams ap{};
        ap.frames = (const uint8_t*)h->frames.p;
        ap.B = B; ap.H = h->rH; ap.W = h->rW;
        ap.row_stride = (long)h->rW * 3;
        ap.frame_stride = (long)h->rH * h->rW * 3;
        ap.kps = (const float*)h->kps.p;
        ap.counts = (const int32_t*)h->counts.p;
        ap.max_faces = K;
        ap.face_slot = (const int32_t*)h->face_slot.p;
        ap.n_faces = n;
        ap.n_dev = n_dev;
        ap.rgb_in = (flags & FRP_FLAG_RGB) ? 1 : 0;
        ap.chips = (_Float16*)h->emb.bufs[h->emb.in_buf].p;
        hipError_t e = launch_align(ap, h->stream);
        if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("align: ") + hipGetErrorString(e));
        rec(h, EV_ALIGN);
        FRPCHK(run_embed(h, sw, n, n_dev, n_known >= 0 ? n_known : B * K));
        if (!(flags & FRP_FLAG_NO_MATCH) && h->g_rows > 0) {
            FRPCHK(run_match(h, sw, n, nullptr, n_dev));
            h->last_matched = true;
        }
        rec(h, EV_MATCH);
    } else {
        rec(h, EV_ALIGN); rec(h, EV_EMB); rec(h, EV_L2); rec(h, EV_MATCH);
    }
    h->ctr.frames += B;
    if (n_dev) {
        h->pend_flops = h->ctr.emb_conv_flops - flops0;      // charged for the capacity: corrected once the count is known
        h->pend_f8flops = h->ctr.f8_conv_flops - f8flops0;
        h->pend_cap = n;
    } else {
        h->ctr.faces += n;
    }
    return FRP_OK;
}

// the face count of a device-count pass, once the stream has been waited for (h_nfaces was copied behind the pass)
int resolve_count(frp_handle* h) {
    if (h->last_nfaces >= 0) return FRP_OK;
    int n = *h->h_nfaces;
    const bool corrupt = n < 0 || n > h->last_cap;     // (the host-count path fails the same way: "corrupt face count")
    if (corrupt) n = 0;
    h->last_nfaces = n;
    h->ctr.faces += n;
    if (h->pend_cap > 0) {
        h->ctr.emb_conv_flops += h->pend_flops * n / h->pend_cap - h->pend_flops;
        h->ctr.f8_conv_flops += h->pend_f8flops * n / h->pend_cap - h->pend_f8flops;
    }
    h->pend_cap = 0;
    h->pend_flops = h->pend_f8flops = 0.0;
    return corrupt ? fail(h, FRP_ERR_HIP, "corrupt face count") : FRP_OK;
}

int run_pipeline(frp_handle* h, int K, float det_thresh, float nms_iou, uint32_t flags) {
    const Switches sw = read_switches();
    if (h->det_scaled) FRPCHK(select_det_source(h, h->rH, h->rW));     // the fused path always detects at full size
    FRPCHK(run_detect(h, sw, K, det_thresh, nms_iou, flags));
    const long A = (long)h->det.dims[h->hdr.det_head_buf[0]].h * h->det.dims[h->hdr.det_head_buf[0]].w * 2;
    return run_faces(h, sw, K, ((flags & FRP_FLAG_FORCED_K) && A >= K) ? h->rB * K : -1, flags);   // forced-K: count known
}

void accumulate_events(frp_handle* h, bool with_h2d) {
    if (!h->cfg.profile) return;
    auto el = [&](int a, int b) { float ms = 0.f; return hipEventElapsedTime(&ms, h->ev[a], h->ev[b]) == hipSuccess ? (double)ms : 0.0; };
    frp_counters& c = h->ctr;
    if (with_h2d) c.ms_h2d += el(EV_START, EV_H2D);
    c.ms_preprocess += el(EV_H2D, EV_PRE);
    c.ms_det_conv += el(EV_PRE, EV_DET);
    c.ms_decode += el(EV_DET, EV_DEC);
    c.ms_align += el(EV_DEC, EV_ALIGN);
    c.ms_emb_conv += el(EV_ALIGN, EV_EMB);
    c.ms_l2norm += el(EV_EMB, EV_L2);
    c.ms_match += el(EV_L2, EV_MATCH);
    c.ms_total += el(with_h2d ? EV_START : EV_H2D, EV_MATCH);
}

// the split entry points (pyramid: frp_detect_resident, frp_finish_faces) account their half of the stage times
void accumulate_detect_events(frp_handle* h) {
    if (!h->cfg.profile) return;
    auto el = [&](int a, int b) { float ms = 0.f; return hipEventElapsedTime(&ms, h->ev[a], h->ev[b]) == hipSuccess ? (double)ms : 0.0; };
    h->ctr.ms_preprocess += el(EV_H2D, EV_PRE);          // incl. the pyramid resize
    h->ctr.ms_det_conv += el(EV_PRE, EV_DET);
    h->ctr.ms_decode += el(EV_DET, EV_DEC);
    h->ctr.ms_total += el(EV_H2D, EV_DEC);
}
void accumulate_face_events(frp_handle* h) {
    if (!h->cfg.profile) return;
    auto el = [&](int a, int b) { float ms = 0.f; return hipEventElapsedTime(&ms, h->ev[a], h->ev[b]) == hipSuccess ? (double)ms : 0.0; };
    h->ctr.ms_align += el(EV_DEC, EV_ALIGN);
    h->ctr.ms_emb_conv += el(EV_ALIGN, EV_EMB);
    h->ctr.ms_l2norm += el(EV_EMB, EV_L2);
    h->ctr.ms_match += el(EV_L2, EV_MATCH);
    h->ctr.ms_total += el(EV_DEC, EV_MATCH);
}

// frp_process_resident returns without waiting for the device also when the stage timers are on: its events are read
// by whichever entry point next waits for the stream anyway (frp_fetch_results, frp_synchronize), or - with a wait of
// their own - by the first other call on the handle, before it could re-record them.  (Reading them inside
// frp_process_resident cost a full stream drain per step: 0.8 ms of a 15 ms step in bench.py's fetch-every-step loop.)
void settle_events(frp_handle* h, bool stream_is_idle) {
    if (!h->ev_pending) return;
    h->ev_pending = false;
    if (!stream_is_idle && hipStreamSynchronize(h->stream) != hipSuccess) return;
    accumulate_events(h, false);
}

// page-locked staging for the result fetch, grown on demand.  Device -> PAGEABLE host copies go through the runtime's own
// bounce buffers with whole-device synchronisation semantics: next to torch / RCCL in the process they serialised the
// copy stream's upload of the next batch behind the fetch (the overlapped loop lost its overlap: 20 vs 14.7 ms per
// step); device -> pinned copies are plain stream-ordered DMA on the handle's own stream.
int ensure_pinned(frp_handle* h, size_t bytes) {
    if (bytes <= h->pin_cap && h->pin_stage) return FRP_OK;
    if (h->pin_stage) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        (void)hipHostFree(h->pin_stage);
        h->pin_stage = nullptr;
        h->pin_cap = 0;
    }
    const size_t want = std::max<size_t>(bytes, 1 << 20);
    void* p = nullptr;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return fail(h, FRP_ERR_OOM, "hipHostMalloc (result staging) failed");
    h->pin_stage = (unsigned char*)p;
    h->pin_cap = want;
    return FRP_OK;
}

int fetch_results(frp_handle* h, float* boxes, float* kps, float* scores, int32_t* counts, float* emb,
                  int32_t* match_idx, float* match_cos) {
    const int B = h->last_B, K = h->last_K;
    if (B <= 0) return fail(h, FRP_ERR_INVALID, "nothing to fetch");
    if (h->last_nfaces < 0) {                  // device-count pass: one short wait for the count, then copy exactly n rows
        HIPCHK(h, hipStreamSynchronize(h->stream));
        FRPCHK(resolve_count(h));
    }
    const int n = h->last_nfaces;
    const size_t s = (size_t)B * K;
    const bool want_emb = n > 0 && emb, want_match = n > 0 && h->last_matched && (match_idx || match_cos);
    // staging layout: counts | boxes | kps | scores | emb (compact, n rows) | idx | cos
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_cnt = take((size_t)B * 4), o_box = take(boxes ? s * 16 : 0), o_kps = take(kps ? s * 40 : 0),
                 o_sc = take(scores ? s * 4 : 0), o_emb = take(want_emb ? (size_t)n * FRP_EMB_DIM * 4 : 0),
                 o_idx = take(want_match ? (size_t)n * 4 : 0), o_cos = take(want_match ? (size_t)n * 4 : 0);
    FRPCHK(ensure_pinned(h, off));
    unsigned char* st = h->pin_stage;
    HIPCHK(h, hipMemcpyAsync(st + o_cnt, h->counts.p, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (boxes) HIPCHK(h, hipMemcpyAsync(st + o_box, h->boxes.p, s * 16, hipMemcpyDeviceToHost, h->stream));
    if (kps) HIPCHK(h, hipMemcpyAsync(st + o_kps, h->kps.p, s * 40, hipMemcpyDeviceToHost, h->stream));
    if (scores) HIPCHK(h, hipMemcpyAsync(st + o_sc, h->scores.p, s * 4, hipMemcpyDeviceToHost, h->stream));
    if (want_emb)
        HIPCHK(h, hipMemcpyAsync(st + o_emb, h->emb.bufs[h->hdr.emb_out_buf].p, (size_t)n * FRP_EMB_DIM * 4, hipMemcpyDeviceToHost, h->stream));
    if (want_match) {
        HIPCHK(h, hipMemcpyAsync(st + o_idx, h->best_idx.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(st + o_cos, h->best_cos.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    settle_events(h, true);
    const int32_t* cnt = (const int32_t*)(st + o_cnt);
    if (counts) memcpy(counts, cnt, (size_t)B * 4);
    if (boxes) memcpy(boxes, st + o_box, s * 16);
    if (kps) memcpy(kps, st + o_kps, s * 40);
    if (scores) memcpy(scores, st + o_sc, s * 4);
    const float* cemb = (const float*)(st + o_emb);
    const int32_t* cidx = (const int32_t*)(st + o_idx);
    const float* ccos = (const float*)(st + o_cos);
    // compact face list -> [B][K] slots; slots beyond counts[b] are zero / -1
    int f = 0;
    for (int b = 0; b < B; ++b) {
        const int nb = std::max(0, std::min(cnt[b], K));
        for (int k = 0; k < K; ++k) {
            const size_t slot = (size_t)b * K + k;
            const bool live = k < nb && f < n;
            if (emb) {
                if (live && want_emb) memcpy(emb + slot * FRP_EMB_DIM, cemb + (size_t)f * FRP_EMB_DIM, FRP_EMB_DIM * 4);
                else memset(emb + slot * FRP_EMB_DIM, 0, FRP_EMB_DIM * 4);
            }
            if (match_idx) match_idx[slot] = (live && want_match) ? cidx[f] : -1;
            if (match_cos) match_cos[slot] = (live && want_match) ? ccos[f] : -1.f;
            if (live) ++f;
        }
    }
    return FRP_OK;
}

int to_f32(frp_handle* h, const void* src, size_t count, int dtype, std::vector<float>& out) {
    out.resize(count);
    if (dtype == FRP_F32) {
        memcpy(out.data(), src, count * 4);
    } else if (dtype == FRP_F64) {
        const double* d = (const double*)src;
        for (size_t i = 0; i < count; ++i) out[i] = (float)d[i];
    } else if (dtype == FRP_F16) {
        const _Float16* d = (const _Float16*)src;
        for (size_t i = 0; i < count; ++i) out[i] = (float)d[i];
    } else {
        return fail(h, FRP_ERR_INVALID, "unknown dtype");
    }
    return FRP_OK;
}

// host fp32 rows -> unit fp16 rows at dst (device), via the scratch buffer
int upload_rows_normalized(frp_handle* h, const float* rows, int64_t n, _Float16* dst) {
    if (n <= 0) return FRP_OK;
    const int64_t chunk = 1 << 16;
    FRPCHK(ensure(h, h->scratch, (size_t)std::min(n, chunk) * FRP_EMB_DIM * 4));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        HIPCHK(h, hipMemcpyAsync(h->scratch.p, rows + r0 * FRP_EMB_DIM, (size_t)m * FRP_EMB_DIM * 4, hipMemcpyHostToDevice, h->stream));
        hipError_t e = launch_gallery_normalize((const float*)h->scratch.p, dst + r0 * FRP_EMB_DIM, m, FRP_EMB_DIM, h->stream);
        if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("gallery_normalize: ") + hipGetErrorString(e));
        HIPCHK(h, hipStreamSynchronize(h->stream));   // scratch is reused by the next chunk
    }
    return FRP_OK;
}

// exact compat rows: `n` host rows of `d` = 512 values of `dtype` -> float64 at dst (device row pointer)
int upload_rows_exact(frp_handle* h, const void* emb, int64_t n, int dtype, double* dst) {
    if (n <= 0) return FRP_OK;
    const size_t cnt = (size_t)n * FRP_EMB_DIM;
    std::vector<double> tmp;
    const double* src = (const double*)emb;
    if (dtype != FRP_F64) {
        tmp.resize(cnt);
        if (dtype == FRP_F32) { const float* f = (const float*)emb; for (size_t i = 0; i < cnt; ++i) tmp[i] = (double)f[i]; }
        else if (dtype == FRP_F16) { const uint16_t* u = (const uint16_t*)emb; for (size_t i = 0; i < cnt; ++i) tmp[i] = (double)f16_bits_to_f32(u[i]); }
        else return fail(h, FRP_ERR_INVALID, "bad dtype");
        src = tmp.data();
    }
    HIPCHK(h, hipMemcpyAsync(dst, src, cnt * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (tmp / the caller's rows go away)
    return FRP_OK;
}

// a fresh exact matrix of `n` rows widened from unit fp16 device rows (rows installed from device data, or that existed before)
int exact_from_f16(frp_handle* h, const void* dev_f16, int64_t n, DevBuf& fresh) {
    if (n <= 0) return FRP_OK;
    FRPCHK(ensure(h, fresh, (size_t)n * FRP_EMB_DIM * 8));
    hipError_t e = launch_gallery_widen((const _Float16*)dev_f16, (double*)fresh.p, n, FRP_EMB_DIM, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { release(fresh); return fail(h, FRP_ERR_HIP, std::string("gallery_widen: ") + hipGetErrorString(e)); }
    return FRP_OK;
}

struct Guard {
    std::lock_guard<std::mutex> lk;
    explicit Guard(frp_handle* h, bool settle = true) : lk(h->mu) {
        (void)hipSetDevice(h->device);
        if (settle) settle_events(h, false);
    }
};

}  // namespace

extern "C" {

const char* frp_version(void) { return "frp 0.1 (gfx950)"; }

int frp_create(int device, const frp_config* cfg, frp_handle** out) {
    if (!out) return FRP_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FRP_ERR_HIP;   // fail loudly: no CPU fallback
    if (device < 0 || device >= ndev) return FRP_ERR_INVALID;
    frp_handle* h = new (std::nothrow) frp_handle();
    if (!h) return FRP_ERR_OOM;
    h->device = device;
    h->cfg.struct_size = sizeof(frp_config);
    h->cfg.max_batch = 32; h->cfg.max_faces = 10; h->cfg.max_h = 1080; h->cfg.max_w = 1920; h->cfg.profile = 0;
    if (cfg) {
        if (cfg->struct_size != (int32_t)sizeof(frp_config)) { delete h; return FRP_ERR_INVALID; }
        if (cfg->max_batch > 0) h->cfg.max_batch = cfg->max_batch;
        if (cfg->max_faces > 0) h->cfg.max_faces = std::min<int>(cfg->max_faces, FRP_MAX_FACES_CAP);
        if (cfg->max_h > 0) h->cfg.max_h = cfg->max_h;
        if (cfg->max_w > 0) h->cfg.max_w = cfg->max_w;
        h->cfg.profile = cfg->profile ? 1 : 0;
    }
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i < EV_COUNT; ++i) ok = hipEventCreate(&h->ev[i]) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&h->h_nfaces, 64, hipHostMallocDefault) == hipSuccess;
    if (ok) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->n_cu = prop.multiProcessorCount;
    }
    // The copy stream gets its own PRIORITY class: the runtime multiplexes the streams of one class onto a few hardware
    // queues (4 by default), and next to torch's and RCCL's streams in the process the staged upload shared a queue with
    // the compute stream and serialised behind the step's kernels (overlapped loop 18.7-20.6 instead of 14.7 ms per
    // step; GPU_MAX_HW_QUEUES=8 restored it).  A stream of another priority class is not pooled with them.
    if (ok) {
        int lo = 0, hi = 0;
        hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (e == hipSuccess && hi != lo) ok = hipStreamCreateWithPriority(&h->copy_stream, hipStreamNonBlocking, hi) == hipSuccess;
        else ok = hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking) == hipSuccess;
    }
    ok = ok && hipEventCreateWithFlags(&h->ev_next_ready, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&h->ev_next_free, hipEventDisableTiming) == hipSuccess;
    if (!ok) { frp_destroy(h); return FRP_ERR_HIP; }
    h->ctr.struct_size = sizeof(frp_counters);
    *out = h;
    return FRP_OK;
}

void frp_destroy(frp_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
    if (h->comm) { (void)rccl().CommDestroy((ncclComm_t)h->comm); h->comm = nullptr; }
    drop_graphs(h);
    for (DevBuf& b : h->det.bufs) release(b);
    for (DevBuf& b : h->emb.bufs) release(b);
    DevBuf* all[] = {&h->wdata, &h->frames, &h->frames_next, &h->boxes, &h->kps, &h->scores, &h->counts, &h->anchor, &h->face_slot, &h->nfaces,
                     &h->q16, &h->part_cos, &h->part_idx, &h->best_cos, &h->best_idx, &h->scratch, &h->splitk_ws, &h->dense_logits, &h->scaled, &h->gallery,
                     &h->g_reserved, &h->gx, &h->gx_q, &h->gx_out, &h->jpeg_coef, &h->jpeg_planes, &h->jpeg_scan, &h->jpeg_err, &h->det_hashes};
    for (DevBuf* b : all) release(*b);
    for (int i = 0; i < EV_COUNT; ++i) if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    for (int i = 0; i < 2; ++i) {
        if (h->jpeg_pin[i]) (void)hipHostFree(h->jpeg_pin[i]);
        if (h->ev_jpeg_h2d[i]) (void)hipEventDestroy(h->ev_jpeg_h2d[i]);
    }
    if (h->h_nfaces) (void)hipHostFree(h->h_nfaces);
    if (h->pin_stage) (void)hipHostFree(h->pin_stage);
    for (void* p : h->pinned) (void)hipHostFree(p);
    if (h->ev_next_ready) (void)hipEventDestroy(h->ev_next_ready);
    if (h->ev_next_free) (void)hipEventDestroy(h->ev_next_free);
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

const char* frp_last_error(const frp_handle* h) { return h ? h->err.c_str() : "null handle"; }

int frp_load_weights(frp_handle* h, const void* blob, size_t bytes) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    h->have_weights = false;          // a failed load never leaves a half-replaced program runnable
    ++h->alloc_epoch;                 // (captured passes of the old program are stale even where the new one lands in the same allocation)
    if (!blob || bytes < sizeof(frp_blob_header)) return fail(h, FRP_ERR_BLOB, "blob too small");
    frp_blob_header hd;
    memcpy(&hd, blob, sizeof(hd));
    if (memcmp(hd.magic, FRP_BLOB_MAGIC, 8) != 0 || hd.version != FRP_BLOB_VERSION || hd.header_bytes != sizeof(frp_blob_header))
        return fail(h, FRP_ERR_BLOB, "bad magic/version");
    if (hd.data_offset > bytes || hd.data_bytes > bytes - hd.data_offset) return fail(h, FRP_ERR_BLOB, "data section out of range");
    if (hd.emb_dim != FRP_EMB_DIM || hd.emb_size != FRP_CHIP || hd.det_in_ch != 8 || hd.emb_in_ch != 8 || hd.det_num_anchors != 2)
        return fail(h, FRP_ERR_BLOB, "unsupported network geometry");
    std::vector<unsigned char> image;     // the device weight image: the data section + the load-time rewrites (net_program.cpp)
    FRPCHK(load_program(h, hd, (const unsigned char*)blob, bytes, read_switches(), image));
    FRPCHK(ensure(h, h->wdata, image.size()));
    HIPCHK(h, hipMemcpyAsync(h->wdata.p, image.data(), image.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->hdr = hd;
    h->have_weights = true;
    return FRP_OK;
}

// ---------------------------------------------------------------- gallery
int frp_gallery_set(frp_handle* h, const void* emb, int64_t n, int32_t d, int32_t dtype) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (h->g_reserved.p) return fail(h, FRP_ERR_INVALID, "a gallery reservation is pending: commit or cancel it first (frp_gallery_commit / frp_gallery_cancel)");
    if (n < 0 || (n > 0 && !emb) || d != FRP_EMB_DIM) return fail(h, FRP_ERR_INVALID, "gallery must be [n x 512]");
    DevBuf fresh, fresh_x;   // new snapshot(s), swapped in when complete
    if (n > 0) {
        std::vector<float> f;
        const float* rows = (const float*)emb;
        if (dtype != FRP_F32) { FRPCHK(to_f32(h, emb, (size_t)n * d, dtype, f)); rows = f.data(); }
        FRPCHK(ensure(h, fresh, (size_t)n * d * 2));
        int r = upload_rows_normalized(h, rows, n, (_Float16*)fresh.p);
        if (r == FRP_OK && h->g_exact) {
            r = ensure(h, fresh_x, (size_t)n * d * 8);
            if (r == FRP_OK) r = upload_rows_exact(h, emb, n, dtype, (double*)fresh_x.p);
        }
        if (r != FRP_OK) { release(fresh); release(fresh_x); return r; }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    release(h->gallery);
    h->gallery = fresh;
    release(h->gx);
    h->gx = fresh_x;
    h->g_rows = n;
    return FRP_OK;
}

int frp_gallery_set_device(frp_handle* h, const void* dev_f16, int64_t n, int32_t d) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (h->g_reserved.p) return fail(h, FRP_ERR_INVALID, "a gallery reservation is pending: commit or cancel it first (frp_gallery_commit / frp_gallery_cancel)");
    if (n <= 0 || !dev_f16 || d != FRP_EMB_DIM) return fail(h, FRP_ERR_INVALID, "gallery must be [n x 512] fp16 on the device");
    DevBuf fresh;
    FRPCHK(ensure(h, fresh, (size_t)n * d * 2));
    hipError_t e = hipMemcpyAsync(fresh.p, dev_f16, (size_t)n * d * 2, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { release(fresh); return fail(h, FRP_ERR_HIP, std::string("gallery copy: ") + hipGetErrorString(e)); }
    DevBuf fresh_x;
    if (h->g_exact) { int r = exact_from_f16(h, fresh.p, n, fresh_x); if (r != FRP_OK) { release(fresh); return r; } }
    release(h->gallery);
    h->gallery = fresh;
    release(h->gx);
    h->gx = fresh_x;
    h->g_rows = n;
    return FRP_OK;
}

int frp_gallery_reserve(frp_handle* h, int64_t capacity_rows, void** dev_f16) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!dev_f16 || capacity_rows <= 0 || capacity_rows > 0x7fffff00L) return fail(h, FRP_ERR_INVALID, "bad gallery reservation");
    release(h->g_reserved);
    FRPCHK(ensure(h, h->g_reserved, (size_t)capacity_rows * FRP_EMB_DIM * 2));
    *dev_f16 = h->g_reserved.p;
    return FRP_OK;
}

int frp_gallery_cancel(frp_handle* h) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (h->g_reserved.p) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        release(h->g_reserved);
    }
    return FRP_OK;
}

int frp_gallery_commit(frp_handle* h, int64_t n_rows) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!h->g_reserved.p || n_rows < 0 || (size_t)n_rows * FRP_EMB_DIM * 2 > h->g_reserved.cap)
        return fail(h, FRP_ERR_INVALID, "gallery commit without a matching reservation");
    HIPCHK(h, hipStreamSynchronize(h->stream));      // nothing of this handle still reads the old snapshot
    DevBuf fresh_x;
    if (h->g_exact) FRPCHK(exact_from_f16(h, h->g_reserved.p, n_rows, fresh_x));
    release(h->gallery);
    h->gallery = h->g_reserved;
    h->g_reserved = DevBuf();
    release(h->gx);
    h->gx = fresh_x;
    h->g_rows = n_rows;
    return FRP_OK;
}

// ---------------------------------------------------------------- multi-GPU: the one collective of the path, on RCCL
// frames are sharded one stream per GPU and need no exchange; the watch list is the exception - every rank decrypts /
// builds N / R rows and the full unit fp16 matrix is all-gathered over xGMI at load and on updates (the reference holds ENCODINGS
// once, in its one process: backend/app/state.py:78).  The library owns that collective: librccl is opened at first use (dlopen - a
// process that never goes multi-GPU does not load it), the communicator lives in the handle, and the gather lands STRAIGHT in a
// reserved snapshot (shard r at row offset r * ceil(N / R): no compaction copy) that is then committed like any other gallery.
// The caller's launcher (torch.distributed.run, MPI, a shell loop) only has to carry the 128-byte unique id from rank 0 to the others.
static_assert(sizeof(ncclUniqueId) == FRP_DIST_ID_BYTES, "include/frp.h: FRP_DIST_ID_BYTES");

int frp_dist_unique_id(void* id128) {
    if (!id128) return FRP_ERR_INVALID;
    Rccl& r = rccl();
    if (!r.err.empty()) return FRP_ERR_HIP;
    ncclUniqueId id;
    if (r.GetUniqueId(&id) != ncclSuccess) return FRP_ERR_HIP;
    memcpy(id128, &id, sizeof(id));
    return FRP_OK;
}

int frp_dist_init(frp_handle* h, const void* id128, int32_t rank, int32_t world) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!id128 || world <= 0 || rank < 0 || rank >= world) return fail(h, FRP_ERR_INVALID, "bad rank / world size");
    if (h->comm) return fail(h, FRP_ERR_INVALID, "this handle already has a communicator (frp_dist_destroy first)");
    Rccl& r = rccl();
    if (!r.err.empty()) return fail(h, FRP_ERR_HIP, r.err);
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t c = nullptr;
    const ncclResult_t e = r.CommInitRank(&c, world, id, rank);          // collective over the ranks (the guard has set this handle's device)
    if (e != ncclSuccess) return fail(h, FRP_ERR_HIP, std::string("ncclCommInitRank: ") + r.GetErrorString(e));
    h->comm = c;
    h->dist_rank = rank;
    h->dist_world = world;
    return FRP_OK;
}

int frp_dist_destroy(frp_handle* h) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (h->comm) {
        (void)hipStreamSynchronize(h->stream);
        (void)rccl().CommDestroy((ncclComm_t)h->comm);
        h->comm = nullptr;
        h->dist_world = 0;
    }
    return FRP_OK;
}

int frp_gallery_allgather(frp_handle* h, const void* shard, int64_t shard_rows, int32_t dtype, int64_t n_total) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!h->comm) return fail(h, FRP_ERR_INVALID, "no communicator (frp_dist_init)");
    if (h->g_reserved.p) return fail(h, FRP_ERR_INVALID, "a gallery reservation is pending: commit or cancel it first");
    const int world = h->dist_world, rank = h->dist_rank;
    if (n_total <= 0 || n_total > 0x7fffff00L || shard_rows < 0 || (shard_rows > 0 && !shard)) return fail(h, FRP_ERR_INVALID, "bad shard");
    const int64_t block = (n_total + world - 1) / world;
    const int64_t first = std::min<int64_t>((int64_t)rank * block, n_total), mine = std::min<int64_t>(block, n_total - first);
    if (shard_rows != mine) return fail(h, FRP_ERR_INVALID, "this rank owns rows [rank * ceil(N / R), ...): shard has another row count");
    Rccl& r = rccl();
    // this rank's rows, unit fp16, padded with zero rows to the block size (the last ranks' shards may be short or empty)
    DevBuf send;
    FRPCHK(ensure(h, send, (size_t)block * FRP_EMB_DIM * 2));
    int rc = FRP_OK;
    hipError_t he = hipMemsetAsync(send.p, 0, (size_t)block * FRP_EMB_DIM * 2, h->stream);
    if (he != hipSuccess) rc = fail(h, FRP_ERR_HIP, std::string("memset: ") + hipGetErrorString(he));
    if (rc == FRP_OK && mine > 0) {
        std::vector<float> f;
        const float* rows = (const float*)shard;
        if (dtype != FRP_F32) { rc = to_f32(h, shard, (size_t)mine * FRP_EMB_DIM, dtype, f); rows = f.data(); }
        if (rc == FRP_OK) rc = upload_rows_normalized(h, rows, mine, (_Float16*)send.p);
    }
    if (rc == FRP_OK) rc = ensure(h, h->g_reserved, (size_t)world * block * FRP_EMB_DIM * 2);
    if (rc == FRP_OK) {
        const ncclResult_t e = r.AllGather(send.p, h->g_reserved.p, (size_t)block * FRP_EMB_DIM, ncclFloat16, (ncclComm_t)h->comm, h->stream);
        if (e != ncclSuccess) rc = fail(h, FRP_ERR_HIP, std::string("ncclAllGather: ") + r.GetErrorString(e));
    }
    if (rc == FRP_OK) {
        he = hipStreamSynchronize(h->stream);
        if (he != hipSuccess) rc = fail(h, FRP_ERR_HIP, std::string("all-gather: ") + hipGetErrorString(he));
    }
    release(send);
    if (rc != FRP_OK) { release(h->g_reserved); return rc; }
    // commit (as frp_gallery_commit): rows [0, n_total) of the gathered blocks ARE the gallery
    DevBuf fresh_x;
    if (h->g_exact) {
        rc = exact_from_f16(h, h->g_reserved.p, n_total, fresh_x);
        if (rc != FRP_OK) { release(h->g_reserved); return rc; }
    }
    release(h->gallery);
    h->gallery = h->g_reserved;
    h->g_reserved = DevBuf();
    release(h->gx);
    h->gx = fresh_x;
    h->g_rows = n_total;
    return FRP_OK;
}

const void* frp_gallery_device_ptr(frp_handle* h) {
    if (!h) return nullptr;
    Guard g(h);
    return h->g_rows > 0 ? h->gallery.p : nullptr;
}

int frp_gallery_update_row(frp_handle* h, int64_t row, const void* emb, int32_t d, int32_t dtype) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (h->g_reserved.p) return fail(h, FRP_ERR_INVALID, "a gallery reservation is pending: commit or cancel it first (frp_gallery_commit / frp_gallery_cancel)");
    if (!emb || d != FRP_EMB_DIM || row < 0 || row > h->g_rows) return fail(h, FRP_ERR_INVALID, "bad gallery row");
    std::vector<float> f;
    FRPCHK(to_f32(h, emb, (size_t)d, dtype, f));
    if (row == h->g_rows && (size_t)(h->g_rows + 1) * d * 2 > h->gallery.cap) {
        // grow: new snapshot with doubled capacity
        DevBuf fresh;
        const size_t cap_rows = std::max<int64_t>(1024, h->g_rows * 2);
        FRPCHK(ensure(h, fresh, cap_rows * d * 2));
        if (h->g_rows > 0) {
            hipError_t e = hipMemcpyAsync(fresh.p, h->gallery.p, (size_t)h->g_rows * d * 2, hipMemcpyDeviceToDevice, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) { release(fresh); return fail(h, FRP_ERR_HIP, std::string("gallery grow: ") + hipGetErrorString(e)); }
        }
        release(h->gallery);
        h->gallery = fresh;
    }
    if (h->g_exact && (size_t)(row + 1) * d * 8 > h->gx.cap) {        // the exact copy grows with the snapshot's row capacity
        DevBuf fresh;
        const size_t cap_rows = std::max<size_t>(h->gallery.cap / ((size_t)d * 2), (size_t)row + 1);
        FRPCHK(ensure(h, fresh, cap_rows * d * 8));
        if (h->g_rows > 0) {
            hipError_t e = hipMemcpyAsync(fresh.p, h->gx.p, (size_t)h->g_rows * d * 8, hipMemcpyDeviceToDevice, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) { release(fresh); return fail(h, FRP_ERR_HIP, std::string("exact gallery grow: ") + hipGetErrorString(e)); }
        }
        release(h->gx);
        h->gx = fresh;
    }
    FRPCHK(upload_rows_normalized(h, f.data(), 1, (_Float16*)h->gallery.p + row * d));
    if (h->g_exact) FRPCHK(upload_rows_exact(h, emb, 1, dtype, (double*)h->gx.p + row * d));
    if (row == h->g_rows) h->g_rows += 1;
    return FRP_OK;
}

int frp_gallery_remove_row(frp_handle* h, int64_t row) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (h->g_reserved.p) return fail(h, FRP_ERR_INVALID, "a gallery reservation is pending: commit or cancel it first (frp_gallery_commit / frp_gallery_cancel)");
    if (row < 0 || row >= h->g_rows) return fail(h, FRP_ERR_INVALID, "bad gallery row");
    const int64_t last = h->g_rows - 1;
    if (row != last) {
        HIPCHK(h, hipMemcpyAsync((_Float16*)h->gallery.p + row * FRP_EMB_DIM, (_Float16*)h->gallery.p + last * FRP_EMB_DIM,
                                 FRP_EMB_DIM * 2, hipMemcpyDeviceToDevice, h->stream));
        if (h->g_exact)
            HIPCHK(h, hipMemcpyAsync((double*)h->gx.p + row * FRP_EMB_DIM, (double*)h->gx.p + last * FRP_EMB_DIM, FRP_EMB_DIM * 8,
                                     hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->g_rows = last;
    return FRP_OK;
}

int64_t frp_gallery_size(const frp_handle* h) { return h ? h->g_rows : -1; }

int frp_gallery_get(frp_handle* h, void* out_f16, int64_t first_row, int64_t n_rows) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!out_f16 || first_row < 0 || n_rows < 0 || first_row + n_rows > h->g_rows) return fail(h, FRP_ERR_INVALID, "bad gallery range");
    if (n_rows == 0) return FRP_OK;
    HIPCHK(h, hipMemcpyAsync(out_f16, (_Float16*)h->gallery.p + first_row * FRP_EMB_DIM, (size_t)n_rows * FRP_EMB_DIM * 2,
                             hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

int frp_gallery_exact(frp_handle* h, int32_t on) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!on) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        release(h->gx); release(h->gx_q); release(h->gx_out);
        h->g_exact = false;
        return FRP_OK;
    }
    if (h->g_exact) return FRP_OK;
    DevBuf fresh;
    if (h->g_rows > 0) {          // rows that exist already: the unit fp16 rows widened (their exact values are gone)
        const size_t cap_rows = std::max<size_t>(h->gallery.cap / ((size_t)FRP_EMB_DIM * 2), (size_t)h->g_rows);
        FRPCHK(ensure(h, fresh, cap_rows * FRP_EMB_DIM * 8));
        hipError_t e = launch_gallery_widen((const _Float16*)h->gallery.p, (double*)fresh.p, h->g_rows, FRP_EMB_DIM, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) { release(fresh); return fail(h, FRP_ERR_HIP, std::string("gallery_widen: ") + hipGetErrorString(e)); }
    }
    release(h->gx);
    h->gx = fresh;
    h->g_exact = true;
    return FRP_OK;
}

int frp_gallery_distances(frp_handle* h, const double* q, int32_t M, double* dist, int64_t n_cols) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!h->g_exact) return fail(h, FRP_ERR_INVALID, "exact rows are not enabled (frp_gallery_exact)");
    if (!q || !dist || M <= 0 || M > 65536) return fail(h, FRP_ERR_INVALID, "bad distance arguments");
    if (n_cols != h->g_rows) return fail(h, FRP_ERR_INVALID, "gallery_distances: output sized for another gallery size");
    if (h->g_rows == 0) return FRP_OK;
    FRPCHK(ensure(h, h->gx_q, (size_t)M * FRP_EMB_DIM * 8));
    FRPCHK(ensure(h, h->gx_out, (size_t)M * h->g_rows * 8));
    HIPCHK(h, hipMemcpyAsync(h->gx_q.p, q, (size_t)M * FRP_EMB_DIM * 8, hipMemcpyHostToDevice, h->stream));
    hipError_t e = launch_gallery_distances((const double*)h->gx.p, h->g_rows, (const double*)h->gx_q.p, M, (double*)h->gx_out.p, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("gallery_distances: ") + hipGetErrorString(e));
    HIPCHK(h, hipMemcpyAsync(dist, h->gx_out.p, (size_t)M * h->g_rows * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

int frp_gallery_get_exact(frp_handle* h, double* out, int64_t first_row, int64_t n_rows) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!h->g_exact) return fail(h, FRP_ERR_INVALID, "exact rows are not enabled (frp_gallery_exact)");
    if (!out || first_row < 0 || n_rows < 0 || first_row + n_rows > h->g_rows) return fail(h, FRP_ERR_INVALID, "bad gallery range");
    if (n_rows == 0) return FRP_OK;
    HIPCHK(h, hipMemcpyAsync(out, (double*)h->gx.p + first_row * FRP_EMB_DIM, (size_t)n_rows * FRP_EMB_DIM * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

// ---------------------------------------------------------------- hot path
int frp_upload_frames(frp_handle* h, const uint8_t* bgr, int32_t B, int32_t H, int32_t W, int64_t row_stride) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    FRPCHK(upload_frames(h, bgr, B, H, W, row_stride));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

void* frp_host_alloc(frp_handle* h, size_t bytes) {
    if (!h || bytes == 0) return nullptr;
    Guard g(h);
    void* p = nullptr;
    if (hipSetDevice(h->device) != hipSuccess || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        fail(h, FRP_ERR_OOM, "hipHostMalloc failed");
        return nullptr;
    }
    h->pinned.push_back(p);
    return p;
}

void frp_host_free(frp_handle* h, void* p) {
    if (!h || !p) return;
    Guard g(h);
    for (size_t i = 0; i < h->pinned.size(); ++i)
        if (h->pinned[i] == p) {
            (void)hipStreamSynchronize(h->copy_stream);
            (void)hipHostFree(p);
            h->pinned.erase(h->pinned.begin() + (long)i);
            return;
        }
}

int frp_upload_frames_async(frp_handle* h, const uint8_t* bgr, int32_t B, int32_t H, int32_t W, int64_t row_stride) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);      // copy stream only: does not re-record the stage events, so a pending pass is not drained
                            // (with the timers on, settling here made the upload of batch t+1 wait for batch t)
    if (!bgr || B <= 0 || H <= 0 || W <= 0 || row_stride < (int64_t)W * 3) return fail(h, FRP_ERR_INVALID, "bad frame arguments");
    if (B > 1024) return fail(h, FRP_ERR_INVALID, "batch too large (max 1024 frames per call)");
    const size_t need = (size_t)B * H * W * 3;
    if (need > h->frames_next.cap || !h->frames_next.p) {
        // growing the staging buffer: nothing may still be copying into / computing from it
        HIPCHK(h, hipStreamSynchronize(h->copy_stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        FRPCHK(ensure(h, h->frames_next, need));
    }
    // the staging buffer was the resident one until the last swap: wait for the work enqueued before it
    HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->ev_next_free, 0));
    HIPCHK(h, hipMemcpy2DAsync(h->frames_next.p, (size_t)W * 3, bgr, (size_t)row_stride, (size_t)W * 3, (size_t)B * H,
                               hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(h, hipEventRecord(h->ev_next_ready, h->copy_stream));
    h->nB = B; h->nH = H; h->nW = W;
    h->next_valid = true;
    return FRP_OK;
}

int frp_jpeg_info_get(const uint8_t* data, size_t size, frp_jpeg_info* info) {
    if (!data || !info) return FRP_ERR_INVALID;
    return jpeg_info(data, size, info, nullptr);
}

int frp_jpeg_coefficients(const uint8_t* data, size_t size, int16_t* coef, size_t coef_elems, uint16_t* qtab, frp_jpeg_info* info) {
    if (!data || !coef || !qtab) return FRP_ERR_INVALID;
    return jpeg_decode_coefficients(data, size, coef, coef_elems, qtab, info, nullptr);
}

// Device entropy decode of a batch whose frames all carry restart intervals (round 5; jpeg_kernels.hip: jpeg_huffman_kernel): the host
// parses headers and finds the RSTn markers (one memchr pass), the COMPRESSED scans go to the device (~0.5 MB per 1080p frame instead of
// 6.3 MB of coefficients), one thread per interval decodes, and the host waits only for the per-image error flags (a corrupt stream
// must be reported by this call, as on the host path) before the pixel kernels are queued.  -> FRP_OK, an error, or 1 = "not this
// batch" (not switched on, no restart intervals, too few of them to fill a wave): the caller takes the host decoder.
namespace {
int upload_jpeg_device(frp_handle* h, const uint8_t* const* jpegs, const size_t* sizes, int32_t B, const frp_jpeg_info& I, int turn,
                       JpegParams& p, size_t total_host_layout, size_t q_off) {
    // When: one thread per interval decodes 32 x 1080p frames in 17.8 ms at one interval per MCU row (120 MCUs), 4.5 ms at 30 MCUs,
    // 1.25 ms at 8 (profiles/r5/jpeg_device_entropy.txt) - the time goes with the LENGTH of an interval, and 16 host threads take
    // 9-12 ms: by default the device decodes streams whose intervals are at most 32 MCUs and the host the others.
    // FRP_JPEG_DEVICE_HUFFMAN=1 (read once): the device whatever the interval (takes the entropy decode off the host's cores; at
    // one interval per row it is slower than the pipeline consumes frames), =0: never.
    const int mode = process_switches().jpeg_device_huffman;
    if (mode < 0 || I.restart_interval <= 0 || (mode == 0 && I.restart_interval > 32)) return 1;
    const long mcus = (long)I.mcus_x * I.mcus_y;
    const long n_int = (mcus + I.restart_interval - 1) / I.restart_interval;
    if ((long)B * n_int < 64 || n_int > 0x7fffff) return 1;
    std::vector<JpegDevicePlan> plans((size_t)B);
    std::vector<JpegHuffTableDev> tabs((size_t)B * 6);
    for (int i = 0; i < B; ++i) {
        std::string e;
        if (!jpegs[i]) return fail(h, FRP_ERR_INVALID, "JPEG " + std::to_string(i) + ": null image");
        const int rc = jpeg_plan_device_decode(jpegs[i], sizes[i], plans[i], tabs.data() + (size_t)i * 6, &e);
        if (rc != FRP_OK) {
            if (plans[i].info.restart_interval <= 0 && plans[i].info.width > 0) return 1;          // a frame without intervals: host path for the batch
            return fail(h, rc, "JPEG " + std::to_string(i) + ": " + e);
        }
        const frp_jpeg_info& Ii = plans[i].info;
        if (Ii.width != I.width || Ii.height != I.height || Ii.components != I.components || Ii.h_samp[0] != I.h_samp[0] || Ii.v_samp[0] != I.v_samp[0])
            return fail(h, FRP_ERR_INVALID, "JPEG " + std::to_string(i) + ": geometry differs from image 0 (one batch = one frame size and sampling)");
        if (Ii.restart_interval != I.restart_interval) return 1;
    }
    // staging layout: scans | interval offsets | tables | quantisation tables | error flags (read back)
    std::vector<size_t> soff((size_t)B + 1, 0);
    for (int i = 0; i < B; ++i) soff[i + 1] = (soff[i] + plans[i].scan_bytes + 15) & ~(size_t)15;
    if (soff[B] >= 0xfffffff0u) return 1;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_int = up(soff[B]), o_tab = up(o_int + (size_t)B * (n_int + 1) * 4), o_q = up(o_tab + (size_t)B * 6 * sizeof(JpegHuffTableDev)),
                 o_err = up(o_q + (size_t)B * 192 * 2), stage_total = o_err + (size_t)B * 4;
    if (h->jpeg_h2d_pending[turn]) {
        HIPCHK(h, hipEventSynchronize(h->ev_jpeg_h2d[turn]));
        h->jpeg_h2d_pending[turn] = false;
    }
    if (stage_total > h->jpeg_pin_cap[turn]) {
        if (h->jpeg_pin[turn]) { (void)hipHostFree(h->jpeg_pin[turn]); h->jpeg_pin[turn] = nullptr; h->jpeg_pin_cap[turn] = 0; }
        if (hipHostMalloc(&h->jpeg_pin[turn], stage_total, hipHostMallocDefault) != hipSuccess) return fail(h, FRP_ERR_OOM, "hipHostMalloc (JPEG staging) failed");
        h->jpeg_pin_cap[turn] = stage_total;
    }
    if (!h->ev_jpeg_h2d[turn]) HIPCHK(h, hipEventCreateWithFlags(&h->ev_jpeg_h2d[turn], hipEventDisableTiming));
    char* st = (char*)h->jpeg_pin[turn];
    uint32_t* io = (uint32_t*)(st + o_int);
    for (int i = 0; i < B; ++i) {
        memcpy(st + soff[i], plans[i].scan, plans[i].scan_bytes);
        for (long k = 0; k <= n_int; ++k) io[(size_t)i * (n_int + 1) + k] = (uint32_t)(soff[i] + plans[i].int_off[(size_t)k]);
        memcpy(st + o_q + (size_t)i * 384, plans[i].qtab, 384);
    }
    memcpy(st + o_tab, tabs.data(), tabs.size() * sizeof(JpegHuffTableDev));
    const size_t need = (size_t)B * I.height * I.width * 3;
    if (need > h->frames_next.cap || !h->frames_next.p || total_host_layout > h->jpeg_coef.cap || (size_t)B * p.plane_img > h->jpeg_planes.cap ||
        o_err > h->jpeg_scan.cap || (size_t)B * 4 > h->jpeg_err.cap) {
        HIPCHK(h, hipStreamSynchronize(h->copy_stream));     // growing buffers: nothing may still be copying into / computing from them
        HIPCHK(h, hipStreamSynchronize(h->stream));
        FRPCHK(ensure(h, h->frames_next, need));
        FRPCHK(ensure(h, h->jpeg_coef, total_host_layout));
        FRPCHK(ensure(h, h->jpeg_planes, (size_t)B * p.plane_img));
        FRPCHK(ensure(h, h->jpeg_scan, o_err));
        FRPCHK(ensure(h, h->jpeg_err, (size_t)B * 4));
    }
    HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->ev_next_free, 0));
    HIPCHK(h, hipMemcpyAsync(h->jpeg_scan.p, st, o_err, hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(h, hipMemsetAsync(h->jpeg_coef.p, 0, q_off, h->copy_stream));
    HIPCHK(h, hipMemcpyAsync((char*)h->jpeg_coef.p + q_off, (char*)h->jpeg_scan.p + o_q, (size_t)B * 384, hipMemcpyDeviceToDevice, h->copy_stream));
    HIPCHK(h, hipMemsetAsync(h->jpeg_err.p, 0, (size_t)B * 4, h->copy_stream));
    JpegHuffParams hp{};
    hp.scan = (const uint8_t*)h->jpeg_scan.p;
    hp.int_off = (const uint32_t*)((const char*)h->jpeg_scan.p + o_int);
    hp.tables = (const JpegHuffTableDev*)((const char*)h->jpeg_scan.p + o_tab);
    hp.coef = (int16_t*)h->jpeg_coef.p;
    hp.err = (int32_t*)h->jpeg_err.p;
    hp.coef_per_image = (long)jpeg_coef_elems(I);
    hp.B = B; hp.n_int = (int)n_int; hp.ri = I.restart_interval;
    hp.mcus_x = I.mcus_x; hp.mcus_y = I.mcus_y; hp.components = I.components;
    for (int c = 0; c < 3; ++c) { hp.hs[c] = I.h_samp[c]; hp.vs[c] = I.v_samp[c]; hp.bx[c] = p.bx[c]; hp.comp_off[c] = p.plane_off[c]; }
    hipError_t e = launch_jpeg_huffman(hp, h->copy_stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("jpeg huffman: ") + hipGetErrorString(e));
    HIPCHK(h, hipMemcpyAsync(st + o_err, h->jpeg_err.p, (size_t)B * 4, hipMemcpyDeviceToHost, h->copy_stream));
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));          // the flags decide this call's return value (and the staging buffer is free again)
    const int32_t* flags = (const int32_t*)(st + o_err);
    for (int i = 0; i < B; ++i)
        if (flags[i]) return fail(h, FRP_ERR_INVALID, "JPEG " + std::to_string(i) + ": corrupt or truncated entropy-coded data");
    p.coef = (const int16_t*)h->jpeg_coef.p;
    p.qtab = (const uint16_t*)((const char*)h->jpeg_coef.p + q_off);
    p.planes = (uint8_t*)h->jpeg_planes.p;
    p.frames = (uint8_t*)h->frames_next.p;
    e = launch_jpeg_decode(p, h->copy_stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("jpeg decode: ") + hipGetErrorString(e));
    HIPCHK(h, hipEventRecord(h->ev_next_ready, h->copy_stream));
    h->nB = B; h->nH = I.height; h->nW = I.width;
    h->next_valid = true;
    h->ctr_jpeg_device_batches += 1;
    return FRP_OK;
}
}  // namespace

int frp_upload_jpeg_async(frp_handle* h, const uint8_t* const* jpegs, const size_t* sizes, int32_t B) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);      // copy stream only (as frp_upload_frames_async)
    if (!jpegs || !sizes || B <= 0 || B > 1024) return fail(h, FRP_ERR_INVALID, "bad JPEG batch arguments");
    frp_jpeg_info I{};
    std::string err;
    if (!jpegs[0] || jpeg_info(jpegs[0], sizes[0], &I, &err) != FRP_OK) return fail(h, FRP_ERR_INVALID, "JPEG 0: " + err);
    const size_t ce = jpeg_coef_elems(I);
    // staging: [B] coefficients (int16) then [B][3][64] tables (uint16), 16-byte aligned parts
    const size_t coef_bytes = (size_t)B * ce * 2, q_off = (coef_bytes + 255) & ~(size_t)255, total = q_off + (size_t)B * 3 * 64 * 2;
    const int turn = h->jpeg_turn;
    h->jpeg_turn ^= 1;
    JpegParams p{};
    p.B = B; p.W = I.width; p.H = I.height; p.components = I.components;
    p.hs = I.h_samp[0]; p.vs = I.v_samp[0];
    p.cw = (I.width + p.hs - 1) / p.hs;
    p.ch = (I.height + p.vs - 1) / p.vs;
    long off = 0;
    for (int c = 0; c < I.components; ++c) {
        p.bx[c] = I.mcus_x * I.h_samp[c];
        p.by[c] = I.mcus_y * I.v_samp[c];
        p.blocks_per_image += p.bx[c] * p.by[c];
        p.plane_off[c] = off;
        off += (long)p.bx[c] * p.by[c] * 64;
    }
    p.plane_img = off;
    {   // restart-interval streams: entropy decode on the device
        const int dr = upload_jpeg_device(h, jpegs, sizes, B, I, turn, p, total, q_off);
        if (dr != 1) return dr;
    }
    if (h->jpeg_h2d_pending[turn]) {                 // the copy of the batch before the previous one read this staging buffer
        HIPCHK(h, hipEventSynchronize(h->ev_jpeg_h2d[turn]));
        h->jpeg_h2d_pending[turn] = false;
    }
    if (total > h->jpeg_pin_cap[turn]) {
        if (h->jpeg_pin[turn]) { (void)hipHostFree(h->jpeg_pin[turn]); h->jpeg_pin[turn] = nullptr; h->jpeg_pin_cap[turn] = 0; }
        if (hipHostMalloc(&h->jpeg_pin[turn], total, hipHostMallocDefault) != hipSuccess) return fail(h, FRP_ERR_OOM, "hipHostMalloc (JPEG staging) failed");
        h->jpeg_pin_cap[turn] = total;
    }
    if (!h->ev_jpeg_h2d[turn]) HIPCHK(h, hipEventCreateWithFlags(&h->ev_jpeg_h2d[turn], hipEventDisableTiming));
    int16_t* coef = (int16_t*)h->jpeg_pin[turn];
    uint16_t* qtab = (uint16_t*)((char*)h->jpeg_pin[turn] + q_off);
    // entropy decoding: one image per task on host threads (the images are independent; within one the bit stream is serial)
    std::vector<int> rcs((size_t)B, FRP_OK);
    std::vector<std::string> errs((size_t)B);
    {
        const int nth = std::max(1, std::min<int>(B, (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()))));
        std::atomic<int> next{0};
        auto work = [&]() {
            for (int i = next.fetch_add(1); i < B; i = next.fetch_add(1)) {
                frp_jpeg_info Ii{};
                if (!jpegs[i]) { rcs[i] = FRP_ERR_INVALID; errs[i] = "null image"; continue; }
                rcs[i] = jpeg_decode_coefficients(jpegs[i], sizes[i], coef + (size_t)i * ce, ce, qtab + (size_t)i * 192, &Ii, &errs[i]);
                if (rcs[i] == FRP_OK && (Ii.width != I.width || Ii.height != I.height || Ii.components != I.components ||
                                         Ii.h_samp[0] != I.h_samp[0] || Ii.v_samp[0] != I.v_samp[0])) {
                    rcs[i] = FRP_ERR_INVALID;
                    errs[i] = "geometry differs from image 0 (one batch = one frame size and sampling)";
                }
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < nth; ++t) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
    }
    for (int i = 0; i < B; ++i)
        if (rcs[i] != FRP_OK) return fail(h, rcs[i], "JPEG " + std::to_string(i) + ": " + errs[i]);
    const size_t need = (size_t)B * I.height * I.width * 3;
    if (need > h->frames_next.cap || !h->frames_next.p || total > h->jpeg_coef.cap || (size_t)B * off > h->jpeg_planes.cap) {
        HIPCHK(h, hipStreamSynchronize(h->copy_stream));     // growing buffers: nothing may still be copying into / computing from them
        HIPCHK(h, hipStreamSynchronize(h->stream));
        FRPCHK(ensure(h, h->frames_next, need));
        FRPCHK(ensure(h, h->jpeg_coef, total));
        FRPCHK(ensure(h, h->jpeg_planes, (size_t)B * off));
    }
    HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->ev_next_free, 0));     // the staging frame buffer was the resident one until the last swap
    HIPCHK(h, hipMemcpyAsync(h->jpeg_coef.p, h->jpeg_pin[turn], total, hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(h, hipEventRecord(h->ev_jpeg_h2d[turn], h->copy_stream));
    h->jpeg_h2d_pending[turn] = true;
    p.coef = (const int16_t*)h->jpeg_coef.p;
    p.qtab = (const uint16_t*)((const char*)h->jpeg_coef.p + q_off);
    p.planes = (uint8_t*)h->jpeg_planes.p;
    p.frames = (uint8_t*)h->frames_next.p;
    hipError_t e = launch_jpeg_decode(p, h->copy_stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("jpeg decode: ") + hipGetErrorString(e));
    HIPCHK(h, hipEventRecord(h->ev_next_ready, h->copy_stream));
    h->nB = B; h->nH = I.height; h->nW = I.width;
    h->next_valid = true;
    return FRP_OK;
}

// diagnostic: network passes replayed from a captured hipGraph (run_net)
int64_t frp_debug_graph_replays(frp_handle* h) {
    if (!h) return -1;
    Guard g(h);
    return h->graph_replays;
}

// diagnostic: how many frp_upload_jpeg_async batches had their entropy decode on the device (restart-interval streams)
int64_t frp_debug_jpeg_device_batches(frp_handle* h) {
    if (!h) return -1;
    Guard g(h, false);
    return h->ctr_jpeg_device_batches;
}

int frp_swap_frames(frp_handle* h) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);      // enqueues a wait + an event on the compute stream; the stage events stay as recorded
    if (!h->next_valid) return fail(h, FRP_ERR_INVALID, "no staged frames (call frp_upload_frames_async)");
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_next_ready, 0));     // compute waits for the staged copy
    std::swap(h->frames, h->frames_next);
    HIPCHK(h, hipEventRecord(h->ev_next_free, h->stream));            // ... and the old resident buffer is free after
    h->rB = h->nB; h->rH = h->nH; h->rW = h->nW;                       // everything enqueued so far
    h->dH = h->rH; h->dW = h->rW; h->det_scaled = false;
    h->canvas_h = round_up(h->rH, 32);
    h->canvas_w = round_up(h->rW, 32);
    h->next_valid = false;
    return FRP_OK;
}

int frp_process_resident(frp_handle* h, int32_t max_faces, float det_thresh, float nms_iou, uint32_t flags) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    rec(h, EV_H2D);
    FRPCHK(run_pipeline(h, max_faces, det_thresh, nms_iou, flags));
    h->ev_pending = h->cfg.profile != 0;
    h->ctr.calls += 1;
    return FRP_OK;
}

int frp_synchronize(frp_handle* h) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    FRPCHK(resolve_count(h));
    settle_events(h, true);
    return FRP_OK;
}

int frp_fetch_results(frp_handle* h, int32_t B, int32_t max_faces, float* boxes, float* kps, float* scores, int32_t* counts,
                      float* emb, int32_t* match_idx, float* match_cos) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    // the caller sized its buffers for B x max_faces: refuse when another thread's call on this handle changed
    // the shape of the results in between (checked under the handle mutex)
    if (B != h->last_B || max_faces != h->last_K)
        return fail(h, FRP_ERR_INVALID, "fetch_results: buffers sized for another batch (results were replaced by a later call)");
    return fetch_results(h, boxes, kps, scores, counts, emb, match_idx, match_cos);
}

int frp_process_frames(frp_handle* h, const uint8_t* bgr, int32_t B, int32_t H, int32_t W, int64_t row_stride,
                       int32_t max_faces, float det_thresh, float nms_iou, uint32_t flags, float* boxes, float* kps,
                       float* scores, int32_t* counts, float* emb, int32_t* match_idx, float* match_cos) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    FRPCHK(upload_frames(h, bgr, B, H, W, row_stride));
    FRPCHK(run_pipeline(h, max_faces, det_thresh, nms_iou, flags));
    FRPCHK(fetch_results(h, boxes, kps, scores, counts, emb, match_idx, match_cos));
    accumulate_events(h, true);
    h->ctr.calls += 1;
    return FRP_OK;
}

int frp_detect(frp_handle* h, const uint8_t* bgr, int32_t B, int32_t H, int32_t W, int64_t row_stride, int32_t max_faces,
               float det_thresh, float nms_iou, uint32_t flags, float* boxes, float* kps, float* scores, int32_t* counts,
               int32_t* anchor_idx) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    FRPCHK(upload_frames(h, bgr, B, H, W, row_stride));
    FRPCHK(run_detect(h, read_switches(), max_faces, det_thresh, nms_iou, flags));
    const size_t s = (size_t)B * max_faces;
    if (boxes) HIPCHK(h, hipMemcpyAsync(boxes, h->boxes.p, s * 16, hipMemcpyDeviceToHost, h->stream));
    if (kps) HIPCHK(h, hipMemcpyAsync(kps, h->kps.p, s * 40, hipMemcpyDeviceToHost, h->stream));
    if (scores) HIPCHK(h, hipMemcpyAsync(scores, h->scores.p, s * 4, hipMemcpyDeviceToHost, h->stream));
    if (counts) HIPCHK(h, hipMemcpyAsync(counts, h->counts.p, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (anchor_idx) HIPCHK(h, hipMemcpyAsync(anchor_idx, h->anchor.p, s * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->last_nfaces = 0;
    return FRP_OK;
}

int frp_detect_resident(frp_handle* h, int32_t B, int32_t det_h, int32_t det_w, int32_t max_faces, float det_thresh, float nms_iou,
                        uint32_t flags, float* boxes, float* kps, float* scores, int32_t* counts, int32_t* anchor_idx) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (B != h->rB) return fail(h, FRP_ERR_INVALID, "detect_resident: buffers sized for another resident batch");
    rec(h, EV_H2D);
    FRPCHK(select_det_source(h, det_h, det_w));
    FRPCHK(run_detect(h, read_switches(), max_faces, det_thresh, nms_iou, flags));
    const size_t s = (size_t)B * max_faces;
    if (boxes) HIPCHK(h, hipMemcpyAsync(boxes, h->boxes.p, s * 16, hipMemcpyDeviceToHost, h->stream));
    if (kps) HIPCHK(h, hipMemcpyAsync(kps, h->kps.p, s * 40, hipMemcpyDeviceToHost, h->stream));
    if (scores) HIPCHK(h, hipMemcpyAsync(scores, h->scores.p, s * 4, hipMemcpyDeviceToHost, h->stream));
    if (counts) HIPCHK(h, hipMemcpyAsync(counts, h->counts.p, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (anchor_idx) HIPCHK(h, hipMemcpyAsync(anchor_idx, h->anchor.p, s * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    accumulate_detect_events(h);
    h->last_nfaces = 0;
    return FRP_OK;
}

int frp_get_det_source(frp_handle* h, uint8_t* out, int64_t out_bytes, int32_t* hs, int32_t* ws) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (h->rB <= 0) return fail(h, FRP_ERR_INVALID, "no resident frames");
    if (hs) *hs = h->dH;
    if (ws) *ws = h->dW;
    const int64_t need = (int64_t)h->rB * h->dH * h->dW * 3;
    if (!out) return FRP_OK;
    if (out_bytes < need) return fail(h, FRP_ERR_INVALID, "buffer too small");
    HIPCHK(h, hipMemcpyAsync(out, h->det_scaled ? h->scaled.p : h->frames.p, (size_t)need, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

int frp_finish_faces(frp_handle* h, int32_t B_in, const float* boxes, const float* kps, const float* scores, const int32_t* counts,
                     int32_t max_faces, uint32_t flags, float* emb, int32_t* match_idx, float* match_cos) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!h->have_weights) return fail(h, FRP_ERR_NO_WEIGHTS, "no weights loaded");
    if (h->rB <= 0) return fail(h, FRP_ERR_INVALID, "no resident frames (call frp_upload_frames)");
    if (B_in != h->rB) return fail(h, FRP_ERR_INVALID, "finish_faces: face list sized for another resident batch");
    if (!kps || !counts || max_faces <= 0 || max_faces > FRP_MAX_FACES_CAP) return fail(h, FRP_ERR_INVALID, "bad face list");
    const int B = h->rB, K = max_faces;
    int n = 0;
    for (int b = 0; b < B; ++b) {
        if (counts[b] < 0 || counts[b] > K) return fail(h, FRP_ERR_INVALID, "face count out of range");
        n += counts[b];
    }
    FRPCHK(ensure_results(h, B, K));
    const size_t s = (size_t)B * K;
    HIPCHK(h, hipMemcpyAsync(h->kps.p, kps, s * 40, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->counts.p, counts, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
    if (boxes) HIPCHK(h, hipMemcpyAsync(h->boxes.p, boxes, s * 16, hipMemcpyHostToDevice, h->stream));
    if (scores) HIPCHK(h, hipMemcpyAsync(h->scores.p, scores, s * 4, hipMemcpyHostToDevice, h->stream));
    hipError_t e = launch_compact_faces((const int32_t*)h->counts.p, B, K, (int32_t*)h->face_slot.p, (int32_t*)h->nfaces.p, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("compact_faces: ") + hipGetErrorString(e));
    h->last_B = B;
    h->last_K = K;
    rec(h, EV_DEC);
    FRPCHK(run_faces(h, read_switches(), K, n, flags));
    FRPCHK(fetch_results(h, nullptr, nullptr, nullptr, nullptr, emb, match_idx, match_cos));
    accumulate_face_events(h);
    h->ctr.calls += 1;
    return FRP_OK;
}

int frp_get_head_map(frp_handle* h, int32_t level, void* out_f16, int64_t out_bytes, int32_t* hl, int32_t* wl) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!h->have_weights || level < 0 || level > 2 || h->last_B <= 0) return fail(h, FRP_ERR_INVALID, "no head map available");
    const int bi = (int)h->hdr.det_head_buf[level];
    const TensorDims d = h->det.dims[bi];
    if (hl) *hl = d.h;
    if (wl) *wl = d.w;
    const int64_t need = (int64_t)h->last_B * d.h * d.w * d.c * 2;
    if (!out_f16) return FRP_OK;
    if (out_bytes < need) return fail(h, FRP_ERR_INVALID, "head map buffer too small");
    HIPCHK(h, hipMemcpyAsync(out_f16, h->det.bufs[bi].p, (size_t)need, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

// Diagnostic (tools/det_hash_bisect.py): enable != 0 - every later detector pass takes a 64-bit hash of each op's output right behind
// the op (stream order: the tensor as the NEXT op reads it); out64 (64 slots, op order) receives the hashes of the last pass.
int frp_debug_det_hashes(frp_handle* h, int32_t enable, uint64_t* out64) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (enable) {
        FRPCHK(ensure(h, h->det_hashes, 64 * 8));
        h->det_hash_on = true;
    } else h->det_hash_on = false;
    if (out64) {
        if (!h->det_hashes.p) return fail(h, FRP_ERR_INVALID, "hashes were never enabled");
        HIPCHK(h, hipMemcpyAsync(out64, h->det_hashes.p, 64 * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return FRP_OK;
}

// Diagnostic (tools/det_bisect.py): the detector program on the resident frames up to and including op `n_ops - 1`, then that op's
// output tensor [B, th, tw, tc] fp16.  Physical buffers are shared between tensors by liveness, so a tensor can only be read
// while nothing behind it has run: hence a prefix run rather than a read after a full pass.
int frp_debug_det_prefix(frp_handle* h, int32_t n_ops, void* out_f16, int64_t out_bytes, int32_t* th, int32_t* tw, int32_t* tc) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!h->have_weights) return fail(h, FRP_ERR_NO_WEIGHTS, "no weights loaded");
    if (h->rB <= 0) return fail(h, FRP_ERR_INVALID, "no resident frames (call frp_upload_frames)");
    if (n_ops <= 0 || n_ops > (int)h->det.ops.size()) return fail(h, FRP_ERR_INVALID, "op count out of range");
    const int B = h->rB, Hc = h->canvas_h, Wc = h->canvas_w;
    const Switches sw = read_switches();
    const bool fused = h->det.det_stem && !sw.no_fused_stem;
    if (!fused) return fail(h, FRP_ERR_INVALID, "prefix runs need the fused stem");
    FRPCHK(plan_net(h, h->det, B, Hc, Wc, fused));
    StemParams sp{};
    sp.frames = h->det_scaled ? (const uint8_t*)h->scaled.p : (const uint8_t*)h->frames.p;
    sp.B = B; sp.H = h->dH; sp.W = h->dW;
    sp.row_stride = (long)h->dW * 3; sp.frame_stride = (long)h->dH * h->dW * 3;
    sp.Hc = Hc; sp.Wc = Wc; sp.Ho = Hc / 2; sp.Wo = Wc / 2;
    sp.rgb_in = 0;
    const bool det_wino = (long)B * (Hc / 8) * (Wc / 8) >= 2L * 240 * (h->n_cu > 0 ? h->n_cu : 256);
    double fl = 0.0;
    int64_t ln = 0;
    h->det_op_limit = n_ops;
    const int rc = run_net(h, sw, h->det, B, Hc, Wc, &fl, &ln, &sp, nullptr, det_wino);
    h->det_op_limit = -1;
    if (rc != FRP_OK) return rc;
    const frp_conv_op& op = h->det.ops[n_ops - 1];
    const TensorDims d = h->det.dims[op.out_buf];
    if (th) *th = d.h;
    if (tw) *tw = d.w;
    if (tc) *tc = d.c;
    const int64_t need = (int64_t)B * d.h * d.w * d.c * 2;
    if (!out_f16) { HIPCHK(h, hipStreamSynchronize(h->stream)); return FRP_OK; }
    if (out_bytes < need) return fail(h, FRP_ERR_INVALID, "tensor buffer too small");
    HIPCHK(h, hipMemcpyAsync(out_f16, h->det.bufs[op.out_buf].p, (size_t)need, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

int frp_decode_heads(frp_handle* h, const void* head8, const void* head16, const void* head32, int32_t B, int32_t canvas_h,
                     int32_t canvas_w, int32_t max_faces, float det_thresh, float nms_iou, uint32_t flags, float* boxes,
                     float* kps, float* scores, int32_t* counts, int32_t* anchor_idx) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!head8 || !head16 || !head32 || B <= 0 || B > 1024 || canvas_h <= 0 || canvas_w <= 0 || (canvas_h & 31) || (canvas_w & 31) ||
        max_faces <= 0 || max_faces > FRP_MAX_FACES_CAP)
        return fail(h, FRP_ERR_INVALID, "bad decode arguments");
    const void* src[3] = {head8, head16, head32};
    DevBuf tmp[3];
    DecodeParams dp{};
    int rc = FRP_OK;
    for (int l = 0; l < 3 && rc == FRP_OK; ++l) {
        dp.hl[l] = canvas_h / (8 << l);
        dp.wl[l] = canvas_w / (8 << l);
        const size_t bytes = (size_t)B * dp.hl[l] * dp.wl[l] * 32 * 2;
        rc = ensure(h, tmp[l], bytes);
        if (rc == FRP_OK && hipMemcpyAsync(tmp[l].p, src[l], bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess)
            rc = fail(h, FRP_ERR_HIP, "head upload failed");
        dp.head[l] = (const _Float16*)tmp[l].p;
    }
    if (rc == FRP_OK) rc = ensure_results(h, B, max_faces);
    if (rc == FRP_OK) {
        dp.B = B; dp.max_faces = max_faces;
        const bool forced = flags & FRP_FLAG_FORCED_K;
        dp.logit_thresh = forced ? -INFINITY : logit_threshold(det_thresh);
        dp.nms_iou = forced ? 2.0f : nms_iou;
        dp.boxes = (float*)h->boxes.p; dp.kps = (float*)h->kps.p; dp.scores = (float*)h->scores.p;
        dp.anchor = (int32_t*)h->anchor.p; dp.counts = (int32_t*)h->counts.p;
        size_t anchors = 0;
        for (int l = 0; l < 3; ++l) anchors += (size_t)dp.hl[l] * dp.wl[l] * 2;
        rc = ensure(h, h->dense_logits, (size_t)B * anchors * 2);
        dp.logits = (_Float16*)h->dense_logits.p;
        hipError_t e = rc == FRP_OK ? launch_decode_nms(dp, h->stream) : hipSuccess;
        if (e != hipSuccess) rc = fail(h, FRP_ERR_HIP, std::string("decode_nms: ") + hipGetErrorString(e));
    }
    const size_t s = (size_t)B * max_faces;
    hipError_t e = hipSuccess;
    if (rc == FRP_OK) {
        if (boxes) e = hipMemcpyAsync(boxes, h->boxes.p, s * 16, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && kps) e = hipMemcpyAsync(kps, h->kps.p, s * 40, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && scores) e = hipMemcpyAsync(scores, h->scores.p, s * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && counts) e = hipMemcpyAsync(counts, h->counts.p, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && anchor_idx) e = hipMemcpyAsync(anchor_idx, h->anchor.p, s * 4, hipMemcpyDeviceToHost, h->stream);
    }
    hipError_t e2 = hipStreamSynchronize(h->stream);
    for (int l = 0; l < 3; ++l) release(tmp[l]);
    if (rc != FRP_OK) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return fail(h, FRP_ERR_HIP, "decode result copy failed");
    return FRP_OK;
}

// to_embedder: chips go to the embedder's input buffer (needs weights); else to h->scratch
static int align_common(frp_handle* h, const uint8_t* bgr, int H, int W, int64_t row_stride, const float* kps, int M, uint32_t flags,
                        bool to_embedder) {
    if (to_embedder && !h->have_weights) return fail(h, FRP_ERR_NO_WEIGHTS, "no weights loaded");
    if (!kps || M <= 0 || M > 65536) return fail(h, FRP_ERR_INVALID, "bad landmark arguments");
    FRPCHK(upload_frames(h, bgr, 1, H, W, row_stride));
    if (to_embedder) FRPCHK(plan_net(h, h->emb, M, FRP_CHIP, FRP_CHIP));
    else FRPCHK(ensure(h, h->scratch, (size_t)M * FRP_CHIP_PIX * 16));
    FRPCHK(ensure(h, h->kps, (size_t)M * 40));
    HIPCHK(h, hipMemcpyAsync(h->kps.p, kps, (size_t)M * 40, hipMemcpyHostToDevice, h->stream));
    AlignParams ap{};
    ap.frames = (const uint8_t*)h->frames.p;
    ap.B = 1; ap.H = H; ap.W = W;
    ap.row_stride = (long)W * 3; ap.frame_stride = (long)H * W * 3;
    ap.kps = (const float*)h->kps.p;
    ap.max_faces = M;
    ap.face_slot = nullptr;
    ap.n_faces = M;
    ap.rgb_in = (flags & FRP_FLAG_RGB) ? 1 : 0;
    ap.chips = to_embedder ? (_Float16*)h->emb.bufs[h->emb.in_buf].p : (_Float16*)h->scratch.p;
    hipError_t e = launch_align(ap, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("align: ") + hipGetErrorString(e));
    return FRP_OK;
}

int frp_align(frp_handle* h, const uint8_t* bgr, int32_t H, int32_t W, int64_t row_stride, const float* kps, int32_t M,
              uint32_t flags, void* chips_f16) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!chips_f16) return fail(h, FRP_ERR_INVALID, "null output");
    FRPCHK(align_common(h, bgr, H, W, row_stride, kps, M, flags, false));
    HIPCHK(h, hipMemcpyAsync(chips_f16, h->scratch.p, (size_t)M * FRP_CHIP_PIX * 8 * 2, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

int frp_embed_faces(frp_handle* h, const uint8_t* bgr, int32_t H, int32_t W, int64_t row_stride, const float* kps, int32_t M,
                    uint32_t flags, float* emb) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!emb) return fail(h, FRP_ERR_INVALID, "null output");
    FRPCHK(align_common(h, bgr, H, W, row_stride, kps, M, flags, true));
    FRPCHK(run_embed(h, read_switches(), M));
    HIPCHK(h, hipMemcpyAsync(emb, h->emb.bufs[h->hdr.emb_out_buf].p, (size_t)M * FRP_EMB_DIM * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

int frp_embed_aligned(frp_handle* h, const uint8_t* chips, int32_t M, float* emb) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!h->have_weights) return fail(h, FRP_ERR_NO_WEIGHTS, "no weights loaded");
    if (!chips || !emb || M <= 0 || M > 65536) return fail(h, FRP_ERR_INVALID, "bad chip arguments");
    FRPCHK(plan_net(h, h->emb, M, FRP_CHIP, FRP_CHIP));
    FRPCHK(ensure(h, h->scratch, (size_t)M * FRP_CHIP_PIX * 3));
    HIPCHK(h, hipMemcpyAsync(h->scratch.p, chips, (size_t)M * FRP_CHIP_PIX * 3, hipMemcpyHostToDevice, h->stream));
    hipError_t e = launch_chips_to_blob((const uint8_t*)h->scratch.p, M, (_Float16*)h->emb.bufs[h->emb.in_buf].p, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("chips_to_blob: ") + hipGetErrorString(e));
    FRPCHK(run_embed(h, read_switches(), M));
    HIPCHK(h, hipMemcpyAsync(emb, h->emb.bufs[h->hdr.emb_out_buf].p, (size_t)M * FRP_EMB_DIM * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

static int match_common(frp_handle* h, const float* q, int M, float* all_scores_host, int32_t* idx, float* cos) {
    const Switches sw = read_switches();
    if (!q || M <= 0 || M > (1 << 20)) return fail(h, FRP_ERR_INVALID, "bad query arguments");
    if (h->g_rows <= 0) return fail(h, FRP_ERR_NO_GALLERY, "gallery is empty");
    const int mpad = round_up(M, 32);
    FRPCHK(ensure(h, h->q16, (size_t)mpad * FRP_EMB_DIM * 2));
    HIPCHK(h, hipMemsetAsync(h->q16.p, 0, (size_t)mpad * FRP_EMB_DIM * 2, h->stream));
    FRPCHK(upload_rows_normalized(h, q, M, (_Float16*)h->q16.p));
    DevBuf all;
    if (all_scores_host) FRPCHK(ensure(h, all, (size_t)M * h->g_rows * 4));
    int rc = run_match(h, sw, M, (float*)all.p);
    hipError_t e = hipSuccess;
    if (rc == FRP_OK) {
        if (idx) e = hipMemcpyAsync(idx, h->best_idx.p, (size_t)M * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && cos) e = hipMemcpyAsync(cos, h->best_cos.p, (size_t)M * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && all_scores_host)
            e = hipMemcpyAsync(all_scores_host, all.p, (size_t)M * h->g_rows * 4, hipMemcpyDeviceToHost, h->stream);
    }
    hipError_t e2 = hipStreamSynchronize(h->stream);
    release(all);
    if (rc != FRP_OK) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return fail(h, FRP_ERR_HIP, "match result copy failed");
    return FRP_OK;
}

int frp_match(frp_handle* h, const float* q, int32_t M, int32_t topk, int32_t* idx, float* cos) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (topk < 1 || topk > FRP_MAX_TOPK) return fail(h, FRP_ERR_INVALID, "topk must be in 1..FRP_MAX_TOPK");
    if (topk == 1) return match_common(h, q, M, nullptr, idx, cos);
    // k > 1: score matrix on the device (query chunks of <= 1 GiB of scores), then k selection passes per row
    if (!q || !idx || !cos || M <= 0 || M > (1 << 20)) return fail(h, FRP_ERR_INVALID, "bad query arguments");
    if (h->g_rows <= 0) return fail(h, FRP_ERR_NO_GALLERY, "gallery is empty");
    const long N = h->g_rows;
    const Switches sw = read_switches();
    int chunk = (int)std::max<long>(1, std::min<long>(M, (1L << 28) / N));
    DevBuf all, didx, dcos;
    int rc = ensure(h, all, (size_t)chunk * N * 4);
    if (rc == FRP_OK) rc = ensure(h, didx, (size_t)chunk * topk * 4);
    if (rc == FRP_OK) rc = ensure(h, dcos, (size_t)chunk * topk * 4);
    hipError_t e = hipSuccess;
    for (int m0 = 0; rc == FRP_OK && e == hipSuccess && m0 < M; m0 += chunk) {
        const int m = std::min(chunk, M - m0);
        const int mpad = round_up(m, 32);
        rc = ensure(h, h->q16, (size_t)mpad * FRP_EMB_DIM * 2);
        if (rc != FRP_OK) break;
        e = hipMemsetAsync(h->q16.p, 0, (size_t)mpad * FRP_EMB_DIM * 2, h->stream);
        if (e != hipSuccess) break;
        rc = upload_rows_normalized(h, q + (size_t)m0 * FRP_EMB_DIM, m, (_Float16*)h->q16.p);
        if (rc == FRP_OK) rc = run_match(h, sw, m, (float*)all.p);
        if (rc != FRP_OK) break;
        e = launch_topk_rows((const float*)all.p, m, N, topk, (int32_t*)didx.p, (float*)dcos.p, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(idx + (size_t)m0 * topk, didx.p, (size_t)m * topk * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cos + (size_t)m0 * topk, dcos.p, (size_t)m * topk * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    (void)hipStreamSynchronize(h->stream);
    release(all); release(didx); release(dcos);
    if (rc != FRP_OK) return rc;
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("match top-k: ") + hipGetErrorString(e));
    return FRP_OK;
}

int frp_match_scores(frp_handle* h, const float* q, int32_t M, float* cos_all, int64_t n_cols) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!cos_all) return fail(h, FRP_ERR_INVALID, "null output");
    // cos_all holds M x n_cols floats: the gallery may have grown since the caller read its size
    if (n_cols != h->g_rows) return fail(h, FRP_ERR_INVALID, "match_scores: output sized for another gallery size");
    return match_common(h, q, M, cos_all, nullptr, nullptr);
}

namespace {
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
    DevBuf dx, dw, db, ds, dr, dout, dwino;
    int rc = ensure(h, dx, xb);
    if (rc == FRP_OK) rc = ensure(h, dw, wb);
    if (rc == FRP_OK) rc = ensure(h, db, bb);
    if (rc == FRP_OK) rc = ensure(h, dout, ob);
    if (rc == FRP_OK && slope) rc = ensure(h, ds, (size_t)Cout * 4);
    if (rc == FRP_OK && res) rc = ensure(h, dr, rb);
    ConvParams p{};
    conv_route_from_abi_flags(flags, p);
    // flags bit 16: through the Winograd kernel (parity tests); an ineligible shape is an error, not a silent fallback
    const bool want_wino = (flags & (1 << 16)) != 0;
    std::vector<uint16_t> wimg;
    if (want_wino) {
        bool shape_ok = conv3x3_wino_shape_ok(W, Cin, ksize, stride) ||
                        (ksize == 3 && stride == 1 && conv3x3_wino_wide_pays(N, H, W, Cin, Cout, h->n_cu, res != nullptr));      // (2-D tiles: wide maps)
#ifdef FRP_LAB
        shape_ok = shape_ok || ((p.dbg & (CONV_DBG_WINO_ROW_PATCH | CONV_DBG_WINO_2D)) && conv3x3_wino_lab_shape_ok(W, Cin, ksize, stride));
#endif
        if (!shape_ok || (flags & (FRP_FLAG_OUT_F32 | FRP_FLAG_RES_UP2)))
            return fail(h, FRP_ERR_INVALID, "shape not covered by the Winograd kernel");
        wimg.resize(conv3x3_wino_image_bytes(Cin, Cout) / 2);
        build_wino_image((const uint16_t*)w, Cin, Cout, wimg.data());
        if (rc == FRP_OK) rc = ensure(h, dwino, wimg.size() * 2);
    }
    hipError_t e = hipSuccess;
    if (rc == FRP_OK) {
        e = hipMemcpyAsync(dx.p, x, xb, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess && want_wino) e = hipMemcpyAsync(dwino.p, wimg.data(), wimg.size() * 2, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dw.p, w, wb, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(db.p, bias, bb, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess && slope) e = hipMemcpyAsync(ds.p, slope, (size_t)Cout * 4, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess && res) e = hipMemcpyAsync(dr.p, res, rb, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) {
            p.x = (const _Float16*)dx.p; p.w = (const _Float16*)dw.p; p.bias = (const float*)db.p;
            p.slope = slope ? (const float*)ds.p : nullptr;
            p.res = res ? (const _Float16*)dr.p : nullptr;
            p.out = dout.p;
            p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.KS = ksize; p.stride = stride; p.act = act;
            p.flags = flags & (FRP_FLAG_BORDER_BIAS | FRP_FLAG_OUT_F32 | FRP_FLAG_RES_UP2);
            p.Hr = res_h; p.Wr = res_w;
            if (want_wino) p.wino_w = (const _Float16*)dwino.p;
            e = launch_conv(p, h->stream);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out, dout.p, ob, hipMemcpyDeviceToHost, h->stream);
    }
    hipError_t e2 = hipStreamSynchronize(h->stream);
    DevBuf* all[] = {&dx, &dw, &db, &ds, &dr, &dout, &dwino};
    for (DevBuf* b : all) release(*b);
    if (rc != FRP_OK) return rc;
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
    DevBuf dx, dw, dws, db, ds, dr, dout, dout2;
    int rc = ensure(h, dx, xb);
    if (rc == FRP_OK) rc = ensure(h, dw, wb);
    if (rc == FRP_OK) rc = ensure(h, dws, (size_t)Cout * 4);
    if (rc == FRP_OK) rc = ensure(h, db, bb);
    if (rc == FRP_OK) rc = ensure(h, dout, on * (out8 ? 1 : 2));
    if (rc == FRP_OK && out2_f8) rc = ensure(h, dout2, on);
    if (rc == FRP_OK && slope) rc = ensure(h, ds, (size_t)Cout * 4);
    if (rc == FRP_OK && res16) rc = ensure(h, dr, on * 2);
    hipError_t e = hipSuccess;
    if (rc == FRP_OK) {
        e = hipMemcpyAsync(dx.p, x8, xb, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dw.p, w8, wb, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dws.p, wscale, (size_t)Cout * 4, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(db.p, bias, bb, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess && slope) e = hipMemcpyAsync(ds.p, slope, (size_t)Cout * 4, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess && res16) e = hipMemcpyAsync(dr.p, res16, on * 2, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) {
            ConvParams p{};
            p.x = (const _Float16*)dx.p; p.w = (const _Float16*)dw.p; p.bias = (const float*)db.p;
            p.slope = slope ? (const float*)ds.p : nullptr;
            p.res = res16 ? (const _Float16*)dr.p : nullptr;
            p.out = dout.p;
            p.out2 = out2_f8 ? dout2.p : nullptr;
            p.wscale = (const float*)dws.p;
            p.in_scale = in_scale; p.out_scale = out_scale;
            p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.KS = 3; p.stride = 1; p.act = act;
            p.flags = (flags & (FRP_FLAG_BORDER_BIAS | FRP_FLAG_OUT_FP8)) | FRP_FLAG_F8;
            e = launch_conv(p, h->stream);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out, dout.p, on * (out8 ? 1 : 2), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && out2_f8) e = hipMemcpyAsync(out2_f8, dout2.p, on, hipMemcpyDeviceToHost, h->stream);
    }
    hipError_t e2 = hipStreamSynchronize(h->stream);
    DevBuf* all[] = {&dx, &dw, &dws, &db, &ds, &dr, &dout, &dout2};
    for (DevBuf* b : all) release(*b);
    if (rc != FRP_OK) return rc;
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? FRP_ERR_INVALID : FRP_ERR_HIP, std::string("conv2d_f8: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("conv2d_f8 sync: ") + hipGetErrorString(e2));
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
    DevBuf dx, dw, db, ds, dr, dout;
    int rc = ensure(h, dx, xn * 2);
    if (rc == FRP_OK) rc = ensure(h, dw, wn * 2);
    if (rc == FRP_OK) rc = ensure(h, db, (size_t)Cout * 4 * 9);
    if (rc == FRP_OK) rc = ensure(h, ds, (size_t)Cout * 4);
    if (rc == FRP_OK) rc = ensure(h, dr, on * 2);
    if (rc == FRP_OK) rc = ensure(h, dout, on * 4);
    hipError_t e = hipSuccess;
    float ms = 0.f;
    if (rc == FRP_OK) {
        e = launch_fill_random_f16((_Float16*)dx.p, (long)xn, 1u, 1.0f, h->stream);
        if (e == hipSuccess) e = launch_fill_random_f16((_Float16*)dw.p, (long)wn, 2u, 1.0f / sqrtf((float)(ksize * ksize * Cin)), h->stream);
        if (e == hipSuccess) e = launch_fill_random_f16((_Float16*)dr.p, (long)on, 3u, 1.0f, h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(db.p, 0, (size_t)Cout * 36, h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(ds.p, 0, (size_t)Cout * 4, h->stream);
        ConvParams p{};
        p.x = (const _Float16*)dx.p; p.w = (const _Float16*)dw.p; p.bias = (const float*)db.p; p.slope = (const float*)ds.p;
        p.res = with_res ? (const _Float16*)dr.p : nullptr; p.out = dout.p;
        p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.KS = ksize; p.stride = stride; p.act = act;
        p.flags = flags & (FRP_FLAG_BORDER_BIAS | FRP_FLAG_OUT_F32 | FRP_FLAG_F8 | FRP_FLAG_OUT_FP8);
        if (f8) {                                         // unit scales in the slope buffer's neighbour: reuse the bias buffer (zeros) + 1
            p.wscale = (const float*)ds.p;                // zeros: products vanish, timing is unaffected
            p.in_scale = p.out_scale = 1.0f;
            if (!(flags & FRP_FLAG_OUT_FP8)) p.out2 = dr.p;   // conv2-style: fp16 out + fp8 copy (residual buffer doubles as the copy target when unused)
            if (with_res) p.out2 = nullptr;
        }
        conv_route_from_abi_flags(flags, p);
        DevBuf dwino;
        bool wino_shape = conv3x3_wino_shape_ok(W, Cin, ksize, stride) || (ksize == 3 && stride == 1 && conv3x3_wino_wide_pays(N, H, W, Cin, Cout, h->n_cu, with_res != 0));
        wino_shape = wino_shape || ((p.dbg & (CONV_DBG_WINO_ROW_PATCH | CONV_DBG_WINO_2D)) && conv3x3_wino_lab_shape_ok(W, Cin, ksize, stride));
        if ((flags & (1 << 16)) && wino_shape) {     // Winograd kernel: a random weight image (timing only)
            const size_t ib = conv3x3_wino_image_bytes(Cin, Cout);
            if (ensure(h, dwino, ib) == FRP_OK) {
                e = launch_fill_random_f16((_Float16*)dwino.p, (long)(ib / 2), 5u, 1.0f / sqrtf((float)(9 * Cin)), h->stream);
                p.wino_w = (const _Float16*)dwino.p;
            }
        }
        DevBuf dst;
        if (stamps_out && ensure(h, dst, 256 * 8 * 8) == FRP_OK) {
            (void)hipMemsetAsync(dst.p, 0, 256 * 8 * 8, h->stream);
            p.stamps = (unsigned long long*)dst.p;
        }
        for (int i = 0; i < 2 && e == hipSuccess; ++i) e = launch_conv(p, h->stream);   // warm-up
        if (e == hipSuccess) e = hipEventRecord(h->ev[0], h->stream);
        for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch_conv(p, h->stream);
        if (e == hipSuccess) e = hipEventRecord(h->ev[1], h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, h->ev[0], h->ev[1]);
        if (e == hipSuccess && stamps_out && p.stamps) e = hipMemcpy(stamps_out, p.stamps, 256 * 8 * 8, hipMemcpyDeviceToHost);
        release(dst);
        (void)hipStreamSynchronize(h->stream);
        release(dwino);
    }
    (void)hipStreamSynchronize(h->stream);
    DevBuf* all[] = {&dx, &dw, &db, &ds, &dr, &dout};
    for (DevBuf* b : all) release(*b);
    if (rc != FRP_OK) return rc;
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
    DevBuf src, dst;
    int rc = ensure(h, src, 3 * 384 * 128);
    if (rc == FRP_OK) rc = ensure(h, dst, (size_t)blocks * 512 * 4);
    hipError_t e = hipSuccess;
    float ms = 0.f;
    if (rc == FRP_OK) {
        e = launch_fill_random_f16((_Float16*)src.p, 3 * 384 * 64, 7u, 1.0f, h->stream);
        auto run = [&]() {
            return lds_reads ? launch_mfma_lds((const _Float16*)src.p, (float*)dst.p, blocks, lds_reads, iters, h->stream)
                             : launch_mfma_peak((const _Float16*)src.p, (float*)dst.p, blocks, iters, h->stream);
        };
        if (e == hipSuccess) e = run();
        if (e == hipSuccess) e = hipEventRecord(h->ev[0], h->stream);
        if (e == hipSuccess) e = run();
        if (e == hipSuccess) e = hipEventRecord(h->ev[1], h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, h->ev[0], h->ev[1]);
    }
    (void)hipStreamSynchronize(h->stream);
    release(src);
    release(dst);
    if (rc != FRP_OK) return rc;
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("mfma_peak: ") + hipGetErrorString(e));
    *tflops = (float)((double)blocks * (lds_reads ? 8.0 * 16 : 4.0 * 4) * iters * 32768.0 / (ms * 1e-3) / 1e12);
    return FRP_OK;
}

int frp_kstep_lab(frp_handle* h, int32_t variant, int32_t iters, float* tflops) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!tflops || iters <= 0) return fail(h, FRP_ERR_INVALID, "bad arguments");
    const int blocks = h->n_cu;
    DevBuf src, dst;
    int rc = ensure(h, src, 4u << 20);        // LDS image + the 4 MiB window the lab's LDS-DMA variants read
    if (rc == FRP_OK) rc = ensure(h, dst, (size_t)blocks * 512 * 4);
    hipError_t e = hipSuccess;
    float ms = 0.f;
    if (rc == FRP_OK) {
        e = launch_fill_random_f16((_Float16*)src.p, 2L << 20, 7u, 1.0f, h->stream);
        if (e == hipSuccess) e = launch_kstep_lab((const _Float16*)src.p, (float*)dst.p, blocks, variant, iters, h->stream);
        if (e == hipSuccess) e = hipEventRecord(h->ev[0], h->stream);
        if (e == hipSuccess) e = launch_kstep_lab((const _Float16*)src.p, (float*)dst.p, blocks, variant, iters, h->stream);
        if (e == hipSuccess) e = hipEventRecord(h->ev[1], h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, h->ev[0], h->ev[1]);
    }
    (void)hipStreamSynchronize(h->stream);
    release(src);
    release(dst);
    if (rc != FRP_OK) return rc;
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? FRP_ERR_INVALID : FRP_ERR_HIP, std::string("kstep_lab: ") + hipGetErrorString(e));
    // fp8 variants (bit 10): 8 MFMAs of 32x32x64 per wave and step = twice the FLOPs of the fp16 step
    *tflops = (float)((double)blocks * kstep_lab_waves(variant) * 16 * kstep_lab_steps_per_iter(variant) * iters * 32768.0 * ((variant & 1024) ? 2.0 : 1.0) /
                      (ms * 1e-3) / 1e12);
    return FRP_OK;
}

#endif  // FRP_LAB

int frp_get_counters(frp_handle* h, frp_counters* out) {
    if (!h || !out) return FRP_ERR_INVALID;
    Guard g(h);
    h->ctr.struct_size = sizeof(frp_counters);
    h->ctr.gallery_rows = h->g_rows;
    *out = h->ctr;
    return FRP_OK;
}

int frp_set_profile(frp_handle* h, int32_t on) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    h->cfg.profile = on ? 1 : 0;
    return FRP_OK;
}

int frp_reset_counters(frp_handle* h) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    h->ctr = frp_counters{};
    h->ctr.struct_size = sizeof(frp_counters);
    return FRP_OK;
}

}  // extern "C"
