// C-ABI host runtime of libfrp.so: handle, weight/program blob, the detect -> align -> embed -> match pipeline on one HIP stream and
// the state of its last pass (Pass, settle_count), the result fetch, the stage entry points, per-stage HIP-event timing.  The matcher's
// host half (queries, launches, hit lists, frp_match*): match_api.cpp; frame ingest: ingest_api.cpp; the gallery snapshots and the
// multi-GPU all-gather: gallery_api.cpp; the network program: net_program.cpp; the stand-alone kernel entry points and the lab hooks:
// kernel_api.cpp.  Interface and the reference call sites each entry point replaces: include/frp.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "frp.h"
#include "frp_blob.h"
#include "frp_internal.h"
#include "frp_handle.h"

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
    s.no_block_fuse = set("FRP_NO_BLOCK_FUSE"); s.block_fuse_all = set("FRP_BLOCK_FUSE_ALL");
    return s;
}

const ProcessSwitches& frp::process_switches() {
    static const ProcessSwitches s = [] {
        const char* jh = getenv("FRP_JPEG_DEVICE_HUFFMAN");
        const char* js = getenv("FRP_JPEG_SELFSYNC");
        return ProcessSwitches{getenv("FRP_NO_GRAPH") != nullptr, getenv("FRP_C64_ALL") != nullptr, !jh ? 0 : (jh[0] == '0' ? -1 : 1), js && js[0] != '0'};
    }();
    return s;
}

namespace {

float logit_threshold(float t) {
    if (!(t > 0.f)) return -INFINITY;
    if (t >= 1.f) return INFINITY;
    return (float)std::log((double)t / (1.0 - (double)t));
}

bool det_size_ok(int Hs, int Ws) { return Hs > 0 && Ws > 0 && Hs <= 16384 && Ws <= 16384; }

// choose the detector source: the resident frames (Hs,Ws == frame size) or a bilinear resize of them
int select_det_source(frp_handle* h, int Hs, int Ws) {
    if (h->rB <= 0) return fail(h, FRP_ERR_INVALID, "no resident frames (call frp_upload_frames)");
    if (!det_size_ok(Hs, Ws)) return fail(h, FRP_ERR_INVALID, "bad detector size");
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

// where a decode writes its K slots per frame instead of the handle's result buffers (frp_process_pyramid: one scale's slice)
struct DetOut {
    float *boxes, *kps, *scores;
    int32_t* counts;
};

// decode + NMS of B frames' head maps (dims[l] = {h, w}) into the result buffers (ensure_results), or into `out`.  Forced-K: no threshold,
// no suppression
int run_decode(frp_handle* h, const void* const head[3], const int dims[3][2], int B, int K, float det_thresh, float nms_iou, uint32_t flags,
               const DetOut* out = nullptr) {
    DecodeParams dp{};
    size_t anchors = 0;
    for (int l = 0; l < 3; ++l) {
        dp.head[l] = (const _Float16*)head[l];
        dp.hl[l] = dims[l][0];
        dp.wl[l] = dims[l][1];
        anchors += (size_t)dp.hl[l] * dp.wl[l] * 2;
    }
    dp.B = B;
    dp.max_faces = K;
    const bool forced = flags & FRP_FLAG_FORCED_K;
    dp.logit_thresh = forced ? -INFINITY : logit_threshold(det_thresh);
    dp.nms_iou = forced ? 2.0f : nms_iou;
    if (out) {
        dp.boxes = out->boxes; dp.kps = out->kps; dp.scores = out->scores; dp.counts = out->counts;     // (no anchor indices)
    } else {
        dp.boxes = (float*)h->boxes.p; dp.kps = (float*)h->kps.p; dp.scores = (float*)h->scores.p;
        dp.anchor = (int32_t*)h->anchor.p; dp.counts = (int32_t*)h->counts.p;
    }
    FRPCHK(ensure(h, h->dense_logits, (size_t)B * anchors * 2));
    dp.logits = (_Float16*)h->dense_logits.p;
    const hipError_t e = launch_decode_nms(dp, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("decode_nms: ") + hipGetErrorString(e));
    return FRP_OK;
}

// counts [B] (device) -> the compact face list (face_slot) and the total (nfaces)
int compact_faces(frp_handle* h, int B, int K) {
    hipError_t e = launch_compact_faces((const int32_t*)h->counts.p, B, K, (int32_t*)h->face_slot.p, (int32_t*)h->nfaces.p, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("compact_faces: ") + hipGetErrorString(e));
    return FRP_OK;
}

// the fused stem's view of the detector source (the resident frames or their resize) and of the canvas
StemParams stem_params(const frp_handle* h, uint32_t flags) {
    StemParams sp{};
    sp.frames = h->det_scaled ? (const uint8_t*)h->scaled.p : (const uint8_t*)h->frames.p;
    sp.B = h->rB; sp.H = h->dH; sp.W = h->dW;
    sp.row_stride = (long)h->dW * 3; sp.frame_stride = (long)h->dH * h->dW * 3;
    sp.Hc = h->canvas_h; sp.Wc = h->canvas_w; sp.Ho = sp.Hc / 2; sp.Wo = sp.Wc / 2;
    sp.rgb_in = (flags & FRP_FLAG_RGB) ? 1 : 0;
    return sp;
}

// Winograd family for the detector's wide 128 / 256-channel layers: from two rounds of 8 x 30 tiles on its stride-8 maps on
// (1080p: four frames; below that the direct family with its quarter tiles and weight prefetch: single-image latency)
bool det_wino(const frp_handle* h) {
    return (long)h->rB * (h->canvas_h / 8) * (h->canvas_w / 8) >= 2L * 240 * (h->n_cu > 0 ? h->n_cu : 256);
}

// detector, decode + NMS, compact face list of the resident frames; touches no Pass state: the caller begins the pass.
// With `out` the detections go there and the result buffers, the compact face list included, stay as they are.
int run_detect(frp_handle* h, const Switches& sw, int K, float det_thresh, float nms_iou, uint32_t flags, const DetOut* out = nullptr) {
    if (!h->have_weights) return fail(h, FRP_ERR_NO_WEIGHTS, "no weights loaded");
    if (h->rB <= 0) return fail(h, FRP_ERR_INVALID, "no resident frames (call frp_upload_frames)");
    if (K <= 0 || K > FRP_MAX_FACES_CAP) return fail(h, FRP_ERR_INVALID, "max_faces out of range");
    const int B = h->rB, Hc = h->canvas_h, Wc = h->canvas_w;
    // The detector's first layer reads the u8 frames directly (fused normalise + conv) whenever
    // the program starts with the standard 3x3 s2 3->32 stem; FRP_NO_FUSED_STEM keeps the
    // two-kernel path (preprocess to an NHWC8 blob, then the generic conv) for A/B runs.
    const bool fused = h->det.det_stem && !sw.no_fused_stem;
    FRPCHK(plan_net(h, h->det, B, Hc, Wc, fused));
    if (!out) FRPCHK(ensure_results(h, B, K));
    const StemParams sp = stem_params(h, flags);
    if (!fused) {
        hipError_t e = launch_preprocess(sp.frames, B, sp.H, sp.W, sp.row_stride, sp.frame_stride, (_Float16*)h->det.bufs[h->det.in_buf].p, Hc, Wc,
                                         sp.rgb_in, h->stream);
        if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("preprocess: ") + hipGetErrorString(e));
    }
    rec(h, EV_PRE);
    FRPCHK(run_net(h, sw, h->det, B, Hc, Wc, &h->ctr.det_conv_flops, &h->ctr.det_conv_launches, fused ? &sp : nullptr, nullptr, det_wino(h)));
    rec(h, EV_DET);
    const void* head[3];
    int dims[3][2];
    for (int l = 0; l < 3; ++l) {
        const int bi = (int)h->hdr.det_head_buf[l];
        head[l] = h->det.bufs[bi].p;
        dims[l][0] = h->det.dims[bi].h;
        dims[l][1] = h->det.dims[bi].w;
        if (h->det.dims[bi].c != 32) return fail(h, FRP_ERR_BLOB, "detector head must have 32 channels");
    }
    FRPCHK(run_decode(h, head, dims, B, K, det_thresh, nms_iou, flags, out));
    if (!out && !(flags & FRP_FLAG_TRACK)) FRPCHK(compact_faces(h, B, K));          // (a tracked pass: track_begin lists the faces, run_faces)
    rec(h, EV_DEC);
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
    FRPCHK(stage_queries(h, n));          // zeroed: the l2norm writes the n rows
    hipError_t e = launch_l2norm((float*)h->emb.bufs[h->hdr.emb_out_buf].p, (_Float16*)h->m.q16.p, n, FRP_EMB_DIM, h->stream,
                                 fc.ksplit != 0 && fc.ksplit != 1 ? (const float*)h->splitk_ws.p : nullptr, fc.ksplit, fc.bias, n_dev, fc.ktot,
                                 h->n_cu);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("l2norm: ") + hipGetErrorString(e));
    rec(h, EV_L2);
    return FRP_OK;
}

// The align launch on the resident frames with the landmarks in h->kps, chips to `chips`.  K > 0: the faces of the compact face list
// (counts, face_slot; K slots per frame) - n of them, or, with n_dev, the count in device memory and n the capacity.
// K == 0: n faces of frame 0, landmark row i = face i.
int run_align(frp_handle* h, int K, int n, const int32_t* n_dev, uint32_t flags, void* chips) {
    AlignParams ap{};
    ap.frames = (const uint8_t*)h->frames.p;
    ap.B = h->rB; ap.H = h->rH; ap.W = h->rW;
    ap.row_stride = (long)h->rW * 3;
    ap.frame_stride = (long)h->rH * h->rW * 3;
    ap.kps = (const float*)h->kps.p;
    if (K > 0) {
        ap.counts = (const int32_t*)h->counts.p;
        ap.face_slot = (const int32_t*)h->face_slot.p;
    }
    ap.max_faces = K > 0 ? K : n;
    ap.n_faces = n;
    ap.n_dev = n_dev;
    ap.rgb_in = (flags & FRP_FLAG_RGB) ? 1 : 0;
    ap.chips = (_Float16*)chips;
    hipError_t e = launch_align(ap, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("align: ") + hipGetErrorString(e));
    return FRP_OK;
}

// align + embed + match for the faces listed in h->kps / h->counts / h->face_slot (device), always from
// the full-resolution resident frames.  n_known >= 0: face count known on the host.  This is where a pass begins.
// FRP_FLAG_TRACK (checked by the caller: track_check): the face list is the tracker's - the detections that continue no identified
// track - so the count is known on the device only, whatever the caller knew; behind the matcher every live slot gets its result
int run_faces(frp_handle* h, const Switches& sw, int K, int n_known, uint32_t flags) {
    const int B = h->rB;
    const bool tracked = (flags & FRP_FLAG_TRACK) != 0;
    if (tracked) n_known = -1;
    const bool want_within = (flags & FRP_FLAG_WITHIN) && !(flags & FRP_FLAG_NO_MATCH);
    const bool want_groups = (flags & FRP_FLAG_GROUPS) != 0;          // (checked by the caller: check_match_flags)
    // a device-count pass that nobody fetched or synchronised yet (two process calls queued back to back): its count and its
    // counter corrections live in single slots (h_nfaces, Pass) this pass is about to reuse - settle it first
    FRPCHK(settle_count(h, false));
    if (tracked) FRPCHK(track_begin(h, B, K));
    // Threshold mode (the reference's loop, routes/camera.py:232-259): how many faces the detector kept is known on the
    // device only.  It STAYS there: align, the embedder's kernels, the l2norm and the matcher are launched for the capacity
    // B x K and read the count from device memory (grids sized for the capacity; workgroups beyond the real tiles leave at
    // once), so the pipeline has no host round trip.  The host learns the count with the results (frp_fetch_results).
    // FRP_HOST_COUNT keeps the former path (copy the count, wait, launch for exactly n) for A/B runs - both give the
    // same bits.  More than FRP_MATCH_TOP1_MAX slots: the per-tile matcher has no device-count form, former path.
    // (FRP_MATCH_V1 pins the per-tile matcher for A/B runs: it has no device-count form either)
    const bool dev_count = n_known < 0 && round_up(B * K, 32) <= FRP_MATCH_TOP1_MAX && !sw.host_count && !sw.match_v1;
    const int32_t* n_dev = dev_count ? (const int32_t*)h->nfaces.p : nullptr;
    if (n_known < 0) HIPCHK(h, hipMemcpyAsync(h->h_nfaces, h->nfaces.p, 4, hipMemcpyDeviceToHost, h->stream));   // read after the next wait
    h->pass = Pass{};
    h->pass.B = B; h->pass.K = K;
    h->pass.within_cap = want_within ? h->m.within_cap : 0;
    h->pass.nfaces = n_known < 0 ? -1 : n_known;          // -1: pending
    h->pass.cap = n_known < 0 ? B * K : n_known;
    h->pass.tracked = tracked;
    h->pass.track_matched = tracked && !(flags & FRP_FLAG_NO_MATCH) && h->g_rows > 0;
    if (n_known < 0 && !dev_count) FRPCHK(settle_count(h, false));   // the former path waits now (and counts the faces ahead of the launches)
    const int n = dev_count ? B * K : h->pass.nfaces;          // the faces everything below is launched for
    const double flops0 = h->ctr.emb_conv_flops, f8flops0 = h->ctr.f8_conv_flops;
    if (n > 0) {
        FRPCHK(plan_net(h, h->emb, n, FRP_CHIP, FRP_CHIP));
        FRPCHK(run_align(h, K, n, n_dev, flags, h->emb.bufs[h->emb.in_buf].p));
        rec(h, EV_ALIGN);
        FRPCHK(run_embed(h, sw, n, n_dev, n_known >= 0 ? n_known : B * K));
        if (!(flags & FRP_FLAG_NO_MATCH) && h->g_rows > 0) FRPCHK(match_pass(h, sw, n, n_dev, want_within, want_groups));
        rec(h, EV_MATCH);
    } else {
        rec(h, EV_ALIGN); rec(h, EV_EMB); rec(h, EV_L2); rec(h, EV_MATCH);
    }
    if (tracked) FRPCHK(track_finish(h, h->pass.matched));          // (also when nothing was embedded: the reused slots, the tables)
    h->ctr.frames += B;
    if (n_dev) {
        h->pass.pend_flops = h->ctr.emb_conv_flops - flops0;      // charged for the capacity: corrected once the count is known
        h->pass.pend_f8flops = h->ctr.f8_conv_flops - f8flops0;
        h->pass.pend_cap = n;
    } else if (n_known >= 0) {
        h->ctr.faces += n;          // (a count that came from the device, now or later: settle_count)
    }
    return FRP_OK;
}

// a detect-only call has replaced the last pass's detections (the stream has been waited for): B x K slots, no face embedded or matched
int begin_detect_only_pass(frp_handle* h, int B, int K) {
    const int rc = settle_count(h, true);          // a pass queued before and never fetched: its count reaches the counters
    h->pass = Pass{};
    h->pass.B = B; h->pass.K = K;
    return rc;
}

// a flagged pass needs frp_set_within / frp_set_frame_groups for its B frames; checked before a pass launches anything or overwrites
// anything of the last one
int check_match_flags(frp_handle* h, uint32_t flags, int B) {
    FRPCHK(track_check(h, flags, B));
    if ((flags & FRP_FLAG_WITHIN) && !(flags & FRP_FLAG_NO_MATCH) && h->m.within_cap <= 0)
        return fail(h, FRP_ERR_INVALID, "FRP_FLAG_WITHIN: call frp_set_within first");
    if (flags & FRP_FLAG_GROUPS) {
        if (flags & FRP_FLAG_NO_MATCH) return fail(h, FRP_ERR_INVALID, "FRP_FLAG_GROUPS has no meaning together with FRP_FLAG_NO_MATCH");
        if (h->m.frame_groups.empty()) return fail(h, FRP_ERR_INVALID, "FRP_FLAG_GROUPS: call frp_set_frame_groups first");
        if ((int)h->m.frame_groups.size() != B) return fail(h, FRP_ERR_INVALID, "FRP_FLAG_GROUPS: frp_set_frame_groups was called for another B");
    }
    return FRP_OK;
}

int run_pipeline(frp_handle* h, int K, float det_thresh, float nms_iou, uint32_t flags) {
    const Switches sw = read_switches();
    FRPCHK(check_match_flags(h, flags, h->rB));
    if (h->det_scaled) FRPCHK(select_det_source(h, h->rH, h->rW));     // the fused path always detects at full size
    FRPCHK(run_detect(h, sw, K, det_thresh, nms_iou, flags));
    const long A = (long)h->det.dims[h->hdr.det_head_buf[0]].h * h->det.dims[h->hdr.det_head_buf[0]].w * 2;
    return run_faces(h, sw, K, ((flags & FRP_FLAG_FORCED_K) && A >= K) ? h->rB * K : -1, flags);   // forced-K: count known
}

// The pyramid as one device pass (frp.h: frp_process_pyramid; arguments checked by the caller): per scale the detector source, the
// detector and decode + NMS into the scale's slice of pyr_*, the cross-scale merge into the result buffers, then the faces from
// the full-resolution frames with the count left on the device.  Stage events: every scale records EV_PRE / EV_DET / EV_DEC again
// and the last record stands, so the earlier scales fall between EV_H2D and the last scale's EV_PRE (ms_preprocess).
int run_pyramid(frp_handle* h, int S, const int32_t* det_hw, int P, int K, float det_thresh, float nms_iou, uint32_t flags) {
    const Switches sw = read_switches();
    const int B = h->rB;
    const size_t sl = (size_t)B * P;      // slots of one scale
    // every buffer the launches below point into has its final size before the first of them (ensure() moves what it grows)
    FRPCHK(ensure_results(h, B, K));
    FRPCHK(ensure(h, h->pyr_boxes, S * sl * 16));
    FRPCHK(ensure(h, h->pyr_kps, S * sl * 40));
    FRPCHK(ensure(h, h->pyr_scores, S * sl * 4));
    FRPCHK(ensure(h, h->pyr_counts, (size_t)S * B * 4));
    PyramidMergeParams mp{};
    for (int s = 0; s < S; ++s) {
        mp.det_h[s] = det_hw[2 * s]; mp.det_w[s] = det_hw[2 * s + 1];
        FRPCHK(select_det_source(h, mp.det_h[s], mp.det_w[s]));
        const DetOut out{(float*)h->pyr_boxes.p + s * sl * 4, (float*)h->pyr_kps.p + s * sl * 10, (float*)h->pyr_scores.p + s * sl,
                         (int32_t*)h->pyr_counts.p + (size_t)s * B};
        FRPCHK(run_detect(h, sw, P, det_thresh, nms_iou, flags, &out));
    }
    mp.boxes = (const float*)h->pyr_boxes.p; mp.kps = (const float*)h->pyr_kps.p; mp.scores = (const float*)h->pyr_scores.p;
    mp.counts = (const int32_t*)h->pyr_counts.p;
    mp.S = S; mp.B = B; mp.P = P; mp.max_faces = K;
    mp.frame_h = h->rH; mp.frame_w = h->rW;
    mp.nms_iou = nms_iou;
    mp.out_boxes = (float*)h->boxes.p; mp.out_kps = (float*)h->kps.p; mp.out_scores = (float*)h->scores.p;
    mp.out_anchor = (int32_t*)h->anchor.p; mp.out_counts = (int32_t*)h->counts.p;
    const hipError_t e = launch_pyramid_merge(mp, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("pyramid_merge: ") + hipGetErrorString(e));
    FRPCHK(compact_faces(h, B, K));
    rec(h, EV_DEC);
    return run_faces(h, sw, K, -1, flags);
}

// Stage timers (timers on): stage i runs from event i to event i + 1.  Adds the stages between two events and their span to the counters.
void accumulate_stages(frp_handle* h, int first, int last) {
    static double frp_counters::* const stage_ms[] = {&frp_counters::ms_h2d,   &frp_counters::ms_preprocess, &frp_counters::ms_det_conv,
                                                      &frp_counters::ms_decode, &frp_counters::ms_align,     &frp_counters::ms_emb_conv,
                                                      &frp_counters::ms_l2norm, &frp_counters::ms_match};
    static_assert(EV_START == 0 && EV_MATCH == sizeof(stage_ms) / sizeof(stage_ms[0]), "one stage between consecutive events");
    if (!h->cfg.profile) return;
    auto el = [&](int a, int b) { float ms = 0.f; return hipEventElapsedTime(&ms, h->ev[a], h->ev[b]) == hipSuccess ? (double)ms : 0.0; };
    for (int i = first; i < last; ++i) h->ctr.*stage_ms[i] += el(i, i + 1);
    h->ctr.ms_total += el(first, last);
}
// a whole pass, and the halves of the split entry points (pyramid: frp_detect_resident - its preprocess includes the resize -, frp_finish_faces)
void accumulate_events(frp_handle* h, bool with_h2d) { accumulate_stages(h, with_h2d ? EV_START : EV_H2D, EV_MATCH); }
void accumulate_detect_events(frp_handle* h) { accumulate_stages(h, EV_H2D, EV_DEC); }
void accumulate_face_events(frp_handle* h) { accumulate_stages(h, EV_DEC, EV_MATCH); }

int fetch_results(frp_handle* h, float* boxes, float* kps, float* scores, int32_t* counts, float* emb,
                  int32_t* match_idx, float* match_cos) {
    const int B = h->pass.B, K = h->pass.K;
    if (B <= 0) return fail(h, FRP_ERR_INVALID, "nothing to fetch");
    FRPCHK(settle_count(h, false));          // device-count pass: one short wait for the count, then copy exactly n rows
    const int n = h->pass.nfaces;
    const size_t s = (size_t)B * K;
    const bool tracked = h->pass.tracked;      // every live slot has a result, embedded in this pass or not: the per-slot arrays
    const bool want_emb = tracked ? emb != nullptr : n > 0 && emb;
    const bool want_match = (tracked ? h->pass.track_matched : n > 0 && h->pass.matched) && (match_idx || match_cos);
    const size_t rows = tracked ? s : (size_t)n;          // result rows copied: all slots, or the compact faces
    // staging layout: counts | boxes | kps | scores | emb (compact, n rows) | idx | cos
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_cnt = take((size_t)B * 4), o_box = take(boxes ? s * 16 : 0), o_kps = take(kps ? s * 40 : 0),
                 o_sc = take(scores ? s * 4 : 0), o_emb = take(want_emb ? rows * FRP_EMB_DIM * 4 : 0),
                 o_idx = take(want_match ? rows * 4 : 0), o_cos = take(want_match ? rows * 4 : 0);
    FRPCHK(ensure_pinned(h, off));
    unsigned char* st = h->pin_stage;
    HIPCHK(h, hipMemcpyAsync(st + o_cnt, h->counts.p, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (boxes) HIPCHK(h, hipMemcpyAsync(st + o_box, h->boxes.p, s * 16, hipMemcpyDeviceToHost, h->stream));
    if (kps) HIPCHK(h, hipMemcpyAsync(st + o_kps, h->kps.p, s * 40, hipMemcpyDeviceToHost, h->stream));
    if (scores) HIPCHK(h, hipMemcpyAsync(st + o_sc, h->scores.p, s * 4, hipMemcpyDeviceToHost, h->stream));
    if (want_emb)
        HIPCHK(h, hipMemcpyAsync(st + o_emb, tracked ? h->trk.slot_emb.p : h->emb.bufs[h->hdr.emb_out_buf].p, rows * FRP_EMB_DIM * 4,
                                 hipMemcpyDeviceToHost, h->stream));
    if (want_match) {
        HIPCHK(h, hipMemcpyAsync(st + o_idx, tracked ? h->trk.slot_idx.p : h->m.best_idx.p, rows * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(st + o_cos, tracked ? h->trk.slot_cos.p : h->m.best_cos.p, rows * 4, hipMemcpyDeviceToHost, h->stream));
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
            const bool live = tracked ? k < nb : k < nb && f < n;
            const size_t r = tracked ? slot : (size_t)f;          // the slot's result row
            if (emb) {
                if (live && want_emb) memcpy(emb + slot * FRP_EMB_DIM, cemb + r * FRP_EMB_DIM, FRP_EMB_DIM * 4);
                else memset(emb + slot * FRP_EMB_DIM, 0, FRP_EMB_DIM * 4);
            }
            if (match_idx) match_idx[slot] = (live && want_match) ? cidx[r] : -1;
            if (match_cos) match_cos[slot] = (live && want_match) ? ccos[r] : -1.f;
            if (live) ++f;
        }
    }
    return FRP_OK;
}

// device -> the caller's array, and the wait for it: the tail of the stage and diagnostic entry points
int copy_out(frp_handle* h, void* dst, const void* src, size_t bytes) {
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

// the detections in the handle's result buffers ([B x K] slots, counts [B]) -> the caller's arrays, those it asked for; waits for the stream
int copy_detections_out(frp_handle* h, int B, int K, float* boxes, float* kps, float* scores, int32_t* counts, int32_t* anchor_idx) {
    const size_t s = (size_t)B * K;
    if (boxes) HIPCHK(h, hipMemcpyAsync(boxes, h->boxes.p, s * 16, hipMemcpyDeviceToHost, h->stream));
    if (kps) HIPCHK(h, hipMemcpyAsync(kps, h->kps.p, s * 40, hipMemcpyDeviceToHost, h->stream));
    if (scores) HIPCHK(h, hipMemcpyAsync(scores, h->scores.p, s * 4, hipMemcpyDeviceToHost, h->stream));
    if (counts) HIPCHK(h, hipMemcpyAsync(counts, h->counts.p, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (anchor_idx) HIPCHK(h, hipMemcpyAsync(anchor_idx, h->anchor.p, s * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

// a caller's face list for the resident frames: landmarks [B x K] slots, counts [B] -> n, the faces it lists
int validate_face_list(frp_handle* h, const float* kps, const int32_t* counts, int K, int& n) {
    if (!kps || !counts || K <= 0 || K > FRP_MAX_FACES_CAP) return fail(h, FRP_ERR_INVALID, "bad face list");
    n = 0;
    for (int b = 0; b < h->rB; ++b) {
        if (counts[b] < 0 || counts[b] > K) return fail(h, FRP_ERR_INVALID, "face count out of range");
        n += counts[b];
    }
    return FRP_OK;
}

// ... into the handle's result buffers (boxes and scores where the caller has them), compacted as the detector's own
int upload_face_list(frp_handle* h, int K, const float* boxes, const float* kps, const float* scores, const int32_t* counts, bool compact = true) {
    const int B = h->rB;
    const size_t s = (size_t)B * K;
    FRPCHK(ensure_results(h, B, K));
    HIPCHK(h, hipMemcpyAsync(h->kps.p, kps, s * 40, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->counts.p, counts, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
    if (boxes) HIPCHK(h, hipMemcpyAsync(h->boxes.p, boxes, s * 16, hipMemcpyHostToDevice, h->stream));
    if (scores) HIPCHK(h, hipMemcpyAsync(h->scores.p, scores, s * 4, hipMemcpyHostToDevice, h->stream));
    return compact ? compact_faces(h, B, K) : FRP_OK;
}

}  // namespace

// page-locked staging for the result fetch, grown on demand.  Device -> PAGEABLE host copies go through the runtime's own
// bounce buffers with whole-device synchronisation semantics: next to torch / RCCL in the process they serialised the
// copy stream's upload of the next batch behind the fetch (the overlapped loop lost its overlap: 20 vs 14.7 ms per
// step); device -> pinned copies are plain stream-ordered DMA on the handle's own stream.
int frp::ensure_pinned(frp_handle* h, size_t bytes) {
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

int frp::settle_count(frp_handle* h, bool stream_is_idle) {
    Pass& p = h->pass;
    if (p.nfaces >= 0) return FRP_OK;
    if (!stream_is_idle) HIPCHK(h, hipStreamSynchronize(h->stream));
    int n = *h->h_nfaces;
    const bool corrupt = n < 0 || n > p.cap;
    if (corrupt) n = 0;
    p.nfaces = n;
    h->ctr.faces += n;
    if (p.pend_cap > 0) {
        h->ctr.emb_conv_flops += p.pend_flops * n / p.pend_cap - p.pend_flops;
        h->ctr.f8_conv_flops += p.pend_f8flops * n / p.pend_cap - p.pend_f8flops;
    }
    p.pend_cap = 0;
    p.pend_flops = p.pend_f8flops = 0.0;
    return corrupt ? fail(h, FRP_ERR_HIP, "corrupt face count") : FRP_OK;
}

// frp_process_resident returns without waiting for the device also when the stage timers are on: its events are read
// by whichever entry point next waits for the stream anyway (frp_fetch_results, frp_synchronize), or - with a wait of
// their own - by the first other call on the handle, before it could re-record them.  (Reading them inside
// frp_process_resident cost a full stream drain per step: 0.8 ms of a 15 ms step in bench.py's fetch-every-step loop.)
void frp::settle_events(frp_handle* h, bool stream_is_idle) {
    if (!h->ev_pending) return;
    h->ev_pending = false;
    if (!stream_is_idle && hipStreamSynchronize(h->stream) != hipSuccess) return;
    accumulate_events(h, false);
}

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
    ok = ok && init_ingest(h);
    if (!ok) { frp_destroy(h); return FRP_ERR_HIP; }
    h->ctr.struct_size = sizeof(frp_counters);
    *out = h;
    return FRP_OK;
}

void frp_destroy(frp_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->in.copy_stream) (void)hipStreamSynchronize(h->in.copy_stream);
    dist_shutdown(h);
    drop_graphs(h);
    for (DevBuf& b : h->det.bufs) release(b);
    for (DevBuf& b : h->emb.bufs) release(b);
    DevBuf* all[] = {&h->wdata, &h->frames, &h->boxes, &h->kps, &h->scores, &h->counts, &h->anchor, &h->face_slot, &h->nfaces,
                     &h->pyr_boxes, &h->pyr_kps, &h->pyr_scores, &h->pyr_counts, &h->m.q16, &h->m.part_cos, &h->m.part_idx, &h->m.best_cos, &h->m.best_idx, &h->m.hit_cnt, &h->m.hit_idx, &h->m.hit_cos, &h->m.q_groups, &h->m.frame_groups_dev, &h->g_groups_dev, &h->scratch, &h->splitk_ws, &h->dense_logits, &h->scaled, &h->gallery,
                     &h->g_reserved, &h->gx, &h->gx_q, &h->gx_out, &h->det_hashes, &h->quality_in, &h->quality_out,
                     &h->jenc_in, &h->jenc_coef, &h->jenc_work, &h->jenc_bits, &h->jenc_out, &h->enh_in, &h->enh_out};
    for (DevBuf* b : all) release(*b);
    for (int i = 0; i < EV_COUNT; ++i) if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    if (h->m.frame_groups_ev) (void)hipEventDestroy(h->m.frame_groups_ev);
    release_tracks(h);
    if (h->h_nfaces) (void)hipHostFree(h->h_nfaces);
    if (h->pin_stage) (void)hipHostFree(h->pin_stage);
    release_ingest(h);
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

// ---------------------------------------------------------------- hot path
// diagnostic: network passes replayed from a captured hipGraph (run_net)
int64_t frp_debug_graph_replays(frp_handle* h) {
    if (!h) return -1;
    Guard g(h);
    return h->graph_replays;
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

int frp_process_pyramid(frp_handle* h, int32_t n_scales, const int32_t* det_hw, int32_t per_scale, int32_t max_faces, float det_thresh,
                        float nms_iou, uint32_t flags) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (flags & FRP_FLAG_TRACK) return fail(h, FRP_ERR_INVALID, "process_pyramid: FRP_FLAG_TRACK is not supported under a cross-scale merge");
    FRPCHK(check_match_flags(h, flags, h->rB));
    if (!h->have_weights) return fail(h, FRP_ERR_INVALID, "process_pyramid: no weights loaded");
    if (h->rB <= 0) return fail(h, FRP_ERR_INVALID, "process_pyramid: no resident frames (call frp_upload_frames)");
    if (n_scales < 1 || n_scales > FRP_PYRAMID_MAX_SCALES || !det_hw) return fail(h, FRP_ERR_INVALID, "process_pyramid: 1 to 4 scales");
    if (per_scale < 1 || per_scale > FRP_MAX_FACES_CAP) return fail(h, FRP_ERR_INVALID, "process_pyramid: per_scale out of range");
    if (max_faces < 1 || max_faces > FRP_MAX_FACES_CAP) return fail(h, FRP_ERR_INVALID, "process_pyramid: max_faces out of range");
    if (n_scales * per_scale > FRP_PYRAMID_MAX_CAND)
        return fail(h, FRP_ERR_INVALID, "process_pyramid: more than 512 candidates per frame (n_scales x per_scale)");
    for (int s = 0; s < n_scales; ++s)
        if (!det_size_ok(det_hw[2 * s], det_hw[2 * s + 1])) return fail(h, FRP_ERR_INVALID, "process_pyramid: bad detector size");
    if (flags & FRP_FLAG_FORCED_K)
        return fail(h, FRP_ERR_INVALID, "process_pyramid: FRP_FLAG_FORCED_K has no meaning under a cross-scale merge");
    rec(h, EV_H2D);
    FRPCHK(run_pyramid(h, n_scales, det_hw, per_scale, max_faces, det_thresh, nms_iou, flags));
    h->ev_pending = h->cfg.profile != 0;
    h->ctr.calls += 1;
    return FRP_OK;
}

int frp_synchronize(frp_handle* h) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    FRPCHK(settle_count(h, true));
    settle_events(h, true);
    return FRP_OK;
}

int frp_fetch_results(frp_handle* h, int32_t B, int32_t max_faces, float* boxes, float* kps, float* scores, int32_t* counts,
                      float* emb, int32_t* match_idx, float* match_cos) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    // the caller sized its buffers for B x max_faces: refuse when another thread's call on this handle changed
    // the shape of the results in between (checked under the handle mutex)
    if (B != h->pass.B || max_faces != h->pass.K)
        return fail(h, FRP_ERR_INVALID, "fetch_results: buffers sized for another batch (results were replaced by a later call)");
    return fetch_results(h, boxes, kps, scores, counts, emb, match_idx, match_cos);
}

int frp_process_frames(frp_handle* h, const uint8_t* bgr, int32_t B, int32_t H, int32_t W, int64_t row_stride,
                       int32_t max_faces, float det_thresh, float nms_iou, uint32_t flags, float* boxes, float* kps,
                       float* scores, int32_t* counts, float* emb, int32_t* match_idx, float* match_cos) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    FRPCHK(check_match_flags(h, flags, B));          // (ahead of the upload: a refused call leaves the resident frames alone too)
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
    FRPCHK(copy_detections_out(h, B, max_faces, boxes, kps, scores, counts, anchor_idx));
    return begin_detect_only_pass(h, B, max_faces);
}

int frp_detect_resident(frp_handle* h, int32_t B, int32_t det_h, int32_t det_w, int32_t max_faces, float det_thresh, float nms_iou,
                        uint32_t flags, float* boxes, float* kps, float* scores, int32_t* counts, int32_t* anchor_idx) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (B != h->rB) return fail(h, FRP_ERR_INVALID, "detect_resident: buffers sized for another resident batch");
    rec(h, EV_H2D);
    FRPCHK(select_det_source(h, det_h, det_w));
    FRPCHK(run_detect(h, read_switches(), max_faces, det_thresh, nms_iou, flags));
    FRPCHK(copy_detections_out(h, B, max_faces, boxes, kps, scores, counts, anchor_idx));
    accumulate_detect_events(h);
    return begin_detect_only_pass(h, B, max_faces);
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
    return copy_out(h, out, h->det_scaled ? h->scaled.p : h->frames.p, (size_t)need);
}

int frp_finish_faces(frp_handle* h, int32_t B_in, const float* boxes, const float* kps, const float* scores, const int32_t* counts,
                     int32_t max_faces, uint32_t flags, float* emb, int32_t* match_idx, float* match_cos) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!h->have_weights) return fail(h, FRP_ERR_NO_WEIGHTS, "no weights loaded");
    if (h->rB <= 0) return fail(h, FRP_ERR_INVALID, "no resident frames (call frp_upload_frames)");
    if (B_in != h->rB) return fail(h, FRP_ERR_INVALID, "finish_faces: face list sized for another resident batch");
    int n;
    FRPCHK(validate_face_list(h, kps, counts, max_faces, n));
    FRPCHK(check_match_flags(h, flags, h->rB));
    if ((flags & FRP_FLAG_TRACK) && !boxes) return fail(h, FRP_ERR_INVALID, "finish_faces: FRP_FLAG_TRACK needs the boxes");
    FRPCHK(upload_face_list(h, max_faces, boxes, kps, scores, counts, !(flags & FRP_FLAG_TRACK)));
    rec(h, EV_DEC);
    FRPCHK(run_faces(h, read_switches(), max_faces, n, flags));
    FRPCHK(fetch_results(h, nullptr, nullptr, nullptr, nullptr, emb, match_idx, match_cos));
    accumulate_face_events(h);
    h->ctr.calls += 1;
    return FRP_OK;
}

int frp_get_head_map(frp_handle* h, int32_t level, void* out_f16, int64_t out_bytes, int32_t* hl, int32_t* wl) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!h->have_weights || level < 0 || level > 2 || h->pass.B <= 0) return fail(h, FRP_ERR_INVALID, "no head map available");
    const int bi = (int)h->hdr.det_head_buf[level];
    const TensorDims d = h->det.dims[bi];
    if (hl) *hl = d.h;
    if (wl) *wl = d.w;
    const int64_t need = (int64_t)h->pass.B * d.h * d.w * d.c * 2;
    if (!out_f16) return FRP_OK;
    if (out_bytes < need) return fail(h, FRP_ERR_INVALID, "head map buffer too small");
    return copy_out(h, out_f16, h->det.bufs[bi].p, (size_t)need);
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
    // (the condition of run_det_stems) both stems in one launch: op 0's map stays in LDS, its buffer is never written
    if (n_ops == 1 && h->det.det_stem12 && (Hc % 4) == 0 && (Wc % 4) == 0 && !sw.no_fused_stem12)
        return fail(h, FRP_ERR_INVALID, "op 0 has no tensor while both stems run as one kernel: set FRP_NO_FUSED_STEM12 to read the stem1 map");
    FRPCHK(plan_net(h, h->det, B, Hc, Wc, fused));
    const StemParams sp = stem_params(h, 0);
    double fl = 0.0;
    int64_t ln = 0;
    h->det_op_limit = n_ops;
    const int rc = run_net(h, sw, h->det, B, Hc, Wc, &fl, &ln, &sp, nullptr, det_wino(h));
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
    return copy_out(h, out_f16, h->det.bufs[op.out_buf].p, (size_t)need);
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
    ScopedBuf tmp[3];
    const int rc = [&]() -> int {
        const void* head[3];
        int dims[3][2];
        for (int l = 0; l < 3; ++l) {
            dims[l][0] = canvas_h / (8 << l);
            dims[l][1] = canvas_w / (8 << l);
            const size_t bytes = (size_t)B * dims[l][0] * dims[l][1] * 32 * 2;
            FRPCHK(ensure(h, tmp[l], bytes));
            if (hipMemcpyAsync(tmp[l]->p, src[l], bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess)
                return fail(h, FRP_ERR_HIP, "head upload failed");
            head[l] = tmp[l]->p;
        }
        FRPCHK(ensure_results(h, B, max_faces));
        FRPCHK(run_decode(h, head, dims, B, max_faces, det_thresh, nms_iou, flags));
        return copy_detections_out(h, B, max_faces, boxes, kps, scores, counts, anchor_idx);
    }();
    if (rc != FRP_OK) (void)hipStreamSynchronize(h->stream);          // the uploads read the caller's maps, tmp[] goes next
    return rc;
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
    return run_align(h, 0, M, nullptr, flags, to_embedder ? h->emb.bufs[h->emb.in_buf].p : h->scratch.p);
}

int frp_align(frp_handle* h, const uint8_t* bgr, int32_t H, int32_t W, int64_t row_stride, const float* kps, int32_t M,
              uint32_t flags, void* chips_f16) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!chips_f16) return fail(h, FRP_ERR_INVALID, "null output");
    FRPCHK(align_common(h, bgr, H, W, row_stride, kps, M, flags, false));
    return copy_out(h, chips_f16, h->scratch.p, (size_t)M * FRP_CHIP_PIX * 8 * 2);
}

// Diagnostic (tests/test_gpu_align_exact.py): the align launch of run_faces - compacted face list, frame of each slot, frame stride, the
// count on the host or in device memory - on the resident frames, into a scratch buffer of B x K chips filled with 0xFF bytes (fp16
// NaN: a chip the launch did not write is recognisable) that is copied back whole.  No weights needed, nothing embedded.
int frp_debug_align_resident(frp_handle* h, const float* kps, const int32_t* counts, int32_t max_faces, uint32_t flags,
                             int32_t device_count, void* chips_f16, int64_t out_bytes) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (h->rB <= 0) return fail(h, FRP_ERR_INVALID, "no resident frames (call frp_upload_frames)");
    const int B = h->rB, K = max_faces;
    int n;
    FRPCHK(validate_face_list(h, kps, counts, K, n));
    const size_t bytes = (size_t)B * K * FRP_CHIP_PIX * 8 * 2;
    if (!chips_f16 || out_bytes < (int64_t)bytes) return fail(h, FRP_ERR_INVALID, "chip buffer too small");
    FRPCHK(settle_count(h, false));           // a device-count pass still owns h->nfaces / h_nfaces: settle it first (as run_faces does)
    FRPCHK(upload_face_list(h, K, nullptr, kps, nullptr, counts));
    FRPCHK(ensure(h, h->scratch, bytes));
    HIPCHK(h, hipMemsetAsync(h->scratch.p, 0xFF, bytes, h->stream));
    FRPCHK(run_align(h, K, device_count ? B * K : n, device_count ? (const int32_t*)h->nfaces.p : nullptr, flags, h->scratch.p));
    return copy_out(h, chips_f16, h->scratch.p, bytes);
}

int frp_embed_faces(frp_handle* h, const uint8_t* bgr, int32_t H, int32_t W, int64_t row_stride, const float* kps, int32_t M,
                    uint32_t flags, float* emb) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!emb) return fail(h, FRP_ERR_INVALID, "null output");
    FRPCHK(align_common(h, bgr, H, W, row_stride, kps, M, flags, true));
    FRPCHK(run_embed(h, read_switches(), M));
    return copy_out(h, emb, h->emb.bufs[h->hdr.emb_out_buf].p, (size_t)M * FRP_EMB_DIM * 4);
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
    return copy_out(h, emb, h->emb.bufs[h->hdr.emb_out_buf].p, (size_t)M * FRP_EMB_DIM * 4);
}

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
