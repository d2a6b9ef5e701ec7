// C-ABI host runtime of libfrp.so: handle, weight/program blob, the detect -> align -> embed -> match
// pipeline on one HIP stream, per-stage HIP-event timing.  Frame ingest: ingest_api.cpp; the gallery snapshots and the
// multi-GPU all-gather: gallery_api.cpp; the stand-alone kernel entry points and the lab hooks: kernel_api.cpp.
// Interface and the reference call sites each entry point replaces: include/frp.h.
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
    h->q16_of_pass = false;
    FRPCHK(ensure(h, h->q16, (size_t)mpad * FRP_EMB_DIM * 2));
    HIPCHK(h, hipMemsetAsync(h->q16.p, 0, (size_t)mpad * FRP_EMB_DIM * 2, h->stream));
    hipError_t e = launch_l2norm((float*)h->emb.bufs[h->hdr.emb_out_buf].p, (_Float16*)h->q16.p, n, FRP_EMB_DIM, h->stream,
                                 fc.ksplit != 0 && fc.ksplit != 1 ? (const float*)h->splitk_ws.p : nullptr, fc.ksplit, fc.bias, n_dev, fc.ktot,
                                 h->n_cu);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("l2norm: ") + hipGetErrorString(e));
    rec(h, EV_L2);
    return FRP_OK;
}

// the "within" epilogue of a match pass (frp_match_within, FRP_FLAG_WITHIN): bound, list size and the device lists [n], [n x cap]
struct WithinArgs {
    float min_cos;
    int cap;
    int32_t* cnt;
    int32_t* idx;
    float* cos;
};
static_assert(FRP_WITHIN_MAX_CAP == FRP_MAX_TOPK, "frp_internal.h: FRP_WITHIN_MAX_CAP");
bool within_args_ok(float min_cos, int cap) { return min_cos >= -2.0f && cap >= 1 && cap <= FRP_MAX_TOPK; }   // (NaN fails the first)

// q16 [mpad,512] holds n unit queries -> best_idx/best_cos [n] (+ the hit lists of `within`, in the same launch)
int run_match(frp_handle* h, const Switches& sw, int n, float* all_scores_dev, const int32_t* n_dev = nullptr,
              const WithinArgs* within = nullptr) {
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
    if (within) {
        HIPCHK(h, hipMemsetAsync(within->cnt, 0, (size_t)n * 4, h->stream));      // counters start at zero before EVERY pass
        mp.min_cos = within->min_cos; mp.cap = within->cap;
        mp.hit_count = within->cnt; mp.hit_idx = within->idx; mp.hit_cos = within->cos;
    }
    hipError_t e = launch_match(mp, sw.match_v1 != 0, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("match: ") + hipGetErrorString(e));
    h->ctr.match_bytes += (double)h->g_rows * FRP_EMB_DIM * 2;
    h->ctr.match_launches += 1;
    return FRP_OK;
}

// Queries `over` (indices into q16 and into the lists) have more than `cap` rows at or above the bound: which of them took the
// slots was a race, so their lists are rebuilt as the first `cap` entries of the matcher's total order - the score rows of those
// queries alone (the per-tile kernel's all_scores epilogue: the same bits), then launch_topk_rows.  All of those entries are hits.
int rebuild_within_lists(frp_handle* h, const _Float16* q16, const std::vector<int>& over, int cap, int32_t* hit_idx, float* hit_cos) {
    const long N = h->g_rows;
    const int total = (int)over.size();
    const int chunk = (int)std::max<long>(1, std::min<long>(total, (1L << 28) / N));      // <= 1 GiB of scores at a time
    const int cpad = round_up(chunk, 32);
    const int n_wg = match_num_workgroups(N);
    ScopedBuf qt, all, pc, pi, bc, bi, tidx, tcos;
    FRPCHK(ensure(h, qt, (size_t)cpad * FRP_EMB_DIM * 2));
    FRPCHK(ensure(h, all, (size_t)chunk * N * 4));
    FRPCHK(ensure(h, pc, (size_t)n_wg * cpad * 4));
    FRPCHK(ensure(h, pi, (size_t)n_wg * cpad * 4));
    FRPCHK(ensure(h, bc, (size_t)cpad * 4));
    FRPCHK(ensure(h, bi, (size_t)cpad * 4));
    FRPCHK(ensure(h, tidx, (size_t)chunk * cap * 4));
    FRPCHK(ensure(h, tcos, (size_t)chunk * cap * 4));
    for (int m0 = 0; m0 < total; m0 += chunk) {
        const int m = std::min(chunk, total - m0);
        HIPCHK(h, hipMemsetAsync(qt->p, 0, (size_t)cpad * FRP_EMB_DIM * 2, h->stream));
        for (int i = 0; i < m; ++i)
            HIPCHK(h, hipMemcpyAsync((_Float16*)qt->p + (size_t)i * FRP_EMB_DIM, q16 + (size_t)over[m0 + i] * FRP_EMB_DIM, FRP_EMB_DIM * 2,
                                     hipMemcpyDeviceToDevice, h->stream));
        MatchParams mp{};
        mp.gallery = (const _Float16*)h->gallery.p;
        mp.N = N;
        mp.q = (const _Float16*)qt->p;
        mp.M = m;
        mp.Mpad = round_up(m, 32);
        mp.n_wg = n_wg;
        mp.part_cos = (float*)pc->p; mp.part_idx = (int32_t*)pi->p;
        mp.best_cos = (float*)bc->p; mp.best_idx = (int32_t*)bi->p;
        mp.all_scores = (float*)all->p;
        hipError_t e = launch_match(mp, true, h->stream);
        if (e == hipSuccess) e = launch_topk_rows((const float*)all->p, m, N, cap, (int32_t*)tidx->p, (float*)tcos->p, h->stream);
        if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("match within (overflow): ") + hipGetErrorString(e));
        h->ctr.match_bytes += (double)N * FRP_EMB_DIM * 2;
        h->ctr.match_launches += 1;
        for (int i = 0; i < m; ++i) {
            const size_t dst = (size_t)over[m0 + i] * cap, src = (size_t)i * cap;
            HIPCHK(h, hipMemcpyAsync(hit_idx + dst, (int32_t*)tidx->p + src, (size_t)cap * 4, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(hit_cos + dst, (float*)tcos->p + src, (size_t)cap * 4, hipMemcpyDeviceToDevice, h->stream));
        }
    }
    return FRP_OK;          // stream-ordered: the caller waits for the stream before the scoped buffers go
}

// align + embed + match for the faces listed in h->kps / h->counts / h->face_slot (device), always from
// the full-resolution resident frames.  n_known >= 0: face count known on the host.
int resolve_count(frp_handle* h);
int run_faces(frp_handle* h, const Switches& sw, int K, int n_known, uint32_t flags) {
    const int B = h->rB;
    int n;
    const bool want_within = (flags & FRP_FLAG_WITHIN) && !(flags & FRP_FLAG_NO_MATCH);
    if (want_within && h->within_cap <= 0) return fail(h, FRP_ERR_INVALID, "FRP_FLAG_WITHIN: call frp_set_within first");
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
    h->last_within_cap = want_within ? h->within_cap : 0;
    h->last_within_lists = false;
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
            if (want_within) {          // the same kernel with the hit-list epilogue: one gallery pass for top-1 and the lists
                const int cap = h->within_cap;
                FRPCHK(ensure(h, h->hit_cnt, (size_t)n * 4));
                FRPCHK(ensure(h, h->hit_idx, (size_t)n * cap * 4));
                FRPCHK(ensure(h, h->hit_cos, (size_t)n * cap * 4));
                const WithinArgs w{h->within_min_cos, cap, (int32_t*)h->hit_cnt.p, (int32_t*)h->hit_idx.p, (float*)h->hit_cos.p};
                FRPCHK(run_match(h, sw, n, nullptr, n_dev, &w));
                h->last_within_lists = true;
                h->q16_of_pass = true;
            } else {
                FRPCHK(run_match(h, sw, n, nullptr, n_dev));
            }
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

// the hit lists of the last flagged pass, compact face list -> [B][K] slots (frp.h: frp_fetch_within)
int fetch_within(frp_handle* h, int cap, int32_t* idx, float* cos, int32_t* n_hits) {
    const int B = h->last_B, K = h->last_K;
    if (B <= 0) return fail(h, FRP_ERR_INVALID, "nothing to fetch");
    if (h->last_within_cap <= 0) return fail(h, FRP_ERR_INVALID, "fetch_within: the last pass ran without FRP_FLAG_WITHIN");
    if (cap != h->last_within_cap) return fail(h, FRP_ERR_INVALID, "fetch_within: buffers sized for another list size than the pass used");
    if (!idx || !cos || !n_hits) return fail(h, FRP_ERR_INVALID, "fetch_within: null output");
    if (h->last_nfaces < 0) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        FRPCHK(resolve_count(h));
    }
    const int n = h->last_nfaces;
    const size_t s = (size_t)B * K;
    std::fill(n_hits, n_hits + s, 0);
    std::fill(idx, idx + s * cap, -1);
    std::fill(cos, cos + s * cap, -2.0f);
    if (n <= 0 || !h->last_within_lists) return FRP_OK;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_cnt = take((size_t)B * 4), o_hc = take((size_t)n * 4), o_hi = take((size_t)n * cap * 4), o_hs = take((size_t)n * cap * 4);
    FRPCHK(ensure_pinned(h, off));
    unsigned char* st = h->pin_stage;
    auto copy_lists = [&]() -> int {
        HIPCHK(h, hipMemcpyAsync(st + o_hi, h->hit_idx.p, (size_t)n * cap * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(st + o_hs, h->hit_cos.p, (size_t)n * cap * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return FRP_OK;
    };
    HIPCHK(h, hipMemcpyAsync(st + o_cnt, h->counts.p, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(st + o_hc, h->hit_cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    FRPCHK(copy_lists());
    settle_events(h, true);
    const int32_t* cnt = (const int32_t*)(st + o_cnt);
    const int32_t* hc = (const int32_t*)(st + o_hc);
    std::vector<int> over;
    for (int f = 0; f < n; ++f)
        if (hc[f] > cap) over.push_back(f);
    if (!over.empty()) {
        if (!h->q16_of_pass)
            return fail(h, FRP_ERR_INVALID, "fetch_within: a face has more hits than the list holds and a later call replaced the pass's embeddings");
        int rc = rebuild_within_lists(h, (const _Float16*)h->q16.p, over, cap, (int32_t*)h->hit_idx.p, (float*)h->hit_cos.p);
        if (rc == FRP_OK) rc = copy_lists();
        else (void)hipStreamSynchronize(h->stream);
        FRPCHK(rc);
    }
    const int32_t* hi = (const int32_t*)(st + o_hi);
    const float* hs = (const float*)(st + o_hs);
    int f = 0;
    for (int b = 0; b < B; ++b) {
        const int nb = std::max(0, std::min(cnt[b], K));
        for (int k = 0; k < nb && f < n; ++k, ++f) {
            const size_t slot = (size_t)b * K + k;
            n_hits[slot] = hc[f];
            memcpy(idx + slot * cap, hi + (size_t)f * cap, (size_t)cap * 4);
            memcpy(cos + slot * cap, hs + (size_t)f * cap, (size_t)cap * 4);
        }
    }
    return FRP_OK;
}

}  // namespace

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
                     &h->q16, &h->part_cos, &h->part_idx, &h->best_cos, &h->best_idx, &h->hit_cnt, &h->hit_idx, &h->hit_cos, &h->scratch, &h->splitk_ws, &h->dense_logits, &h->scaled, &h->gallery,
                     &h->g_reserved, &h->gx, &h->gx_q, &h->gx_out, &h->det_hashes, &h->quality_in, &h->quality_out,
                     &h->jenc_in, &h->jenc_coef, &h->jenc_work, &h->jenc_bits, &h->jenc_out};
    for (DevBuf* b : all) release(*b);
    for (int i = 0; i < EV_COUNT; ++i) if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
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

int frp_set_within(frp_handle* h, float min_cos, int32_t cap) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    if (!within_args_ok(min_cos, cap)) return fail(h, FRP_ERR_INVALID, "set_within: min_cos must be >= -2 and cap in 1..FRP_MAX_TOPK");
    h->within_min_cos = min_cos;
    h->within_cap = cap;
    return FRP_OK;
}

int frp_fetch_within(frp_handle* h, int32_t B, int32_t max_faces, int32_t cap, int32_t* idx, float* cos, int32_t* n_hits) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    if (B != h->last_B || max_faces != h->last_K)
        return fail(h, FRP_ERR_INVALID, "fetch_within: buffers sized for another batch (results were replaced by a later call)");
    return fetch_within(h, cap, idx, cos, n_hits);
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
    // (the condition of run_det_stems) both stems in one launch: op 0's map stays in LDS, its buffer is never written
    if (n_ops == 1 && h->det.det_stem12 && (Hc % 4) == 0 && (Wc % 4) == 0 && !sw.no_fused_stem12)
        return fail(h, FRP_ERR_INVALID, "op 0 has no tensor while both stems run as one kernel: set FRP_NO_FUSED_STEM12 to read the stem1 map");
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
    ScopedBuf tmp[3];
    DecodeParams dp{};
    int rc = FRP_OK;
    for (int l = 0; l < 3 && rc == FRP_OK; ++l) {
        dp.hl[l] = canvas_h / (8 << l);
        dp.wl[l] = canvas_w / (8 << l);
        const size_t bytes = (size_t)B * dp.hl[l] * dp.wl[l] * 32 * 2;
        rc = ensure(h, tmp[l], bytes);
        if (rc == FRP_OK && hipMemcpyAsync(tmp[l]->p, src[l], bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess)
            rc = fail(h, FRP_ERR_HIP, "head upload failed");
        dp.head[l] = (const _Float16*)tmp[l]->p;
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

// Diagnostic (tests/test_gpu_align_exact.py): the align launch of run_faces - compacted face list, frame of each slot, frame stride, the
// count on the host or in device memory - on the resident frames, into a scratch buffer of B x K chips filled with 0xFF bytes (fp16
// NaN: a chip the launch did not write is recognisable) that is copied back whole.  No weights needed, nothing embedded.
int frp_debug_align_resident(frp_handle* h, const float* kps, const int32_t* counts, int32_t max_faces, uint32_t flags,
                             int32_t device_count, void* chips_f16, int64_t out_bytes) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (h->rB <= 0) return fail(h, FRP_ERR_INVALID, "no resident frames (call frp_upload_frames)");
    if (!kps || !counts || max_faces <= 0 || max_faces > FRP_MAX_FACES_CAP) return fail(h, FRP_ERR_INVALID, "bad face list");
    const int B = h->rB, K = max_faces;
    int n = 0;
    for (int b = 0; b < B; ++b) {
        if (counts[b] < 0 || counts[b] > K) return fail(h, FRP_ERR_INVALID, "face count out of range");
        n += counts[b];
    }
    const size_t s = (size_t)B * K, bytes = s * FRP_CHIP_PIX * 8 * 2;
    if (!chips_f16 || out_bytes < (int64_t)bytes) return fail(h, FRP_ERR_INVALID, "chip buffer too small");
    if (h->last_nfaces < 0) {           // a device-count pass still owns h->nfaces / h_nfaces: settle it first (as run_faces does)
        HIPCHK(h, hipStreamSynchronize(h->stream));
        FRPCHK(resolve_count(h));
    }
    FRPCHK(ensure_results(h, B, K));
    FRPCHK(ensure(h, h->scratch, bytes));
    HIPCHK(h, hipMemcpyAsync(h->kps.p, kps, s * 40, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->counts.p, counts, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
    hipError_t e = launch_compact_faces((const int32_t*)h->counts.p, B, K, (int32_t*)h->face_slot.p, (int32_t*)h->nfaces.p, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("compact_faces: ") + hipGetErrorString(e));
    HIPCHK(h, hipMemsetAsync(h->scratch.p, 0xFF, bytes, h->stream));
    AlignParams ap{};
    ap.frames = (const uint8_t*)h->frames.p;
    ap.B = B; ap.H = h->rH; ap.W = h->rW;
    ap.row_stride = (long)h->rW * 3;
    ap.frame_stride = (long)h->rH * h->rW * 3;
    ap.kps = (const float*)h->kps.p;
    ap.counts = (const int32_t*)h->counts.p;
    ap.max_faces = K;
    ap.face_slot = (const int32_t*)h->face_slot.p;
    ap.n_faces = device_count ? B * K : n;
    ap.n_dev = device_count ? (const int32_t*)h->nfaces.p : nullptr;
    ap.rgb_in = (flags & FRP_FLAG_RGB) ? 1 : 0;
    ap.chips = (_Float16*)h->scratch.p;
    e = launch_align(ap, h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("align: ") + hipGetErrorString(e));
    HIPCHK(h, hipMemcpyAsync(chips_f16, h->scratch.p, bytes, hipMemcpyDeviceToHost, h->stream));
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
    h->q16_of_pass = false;
    FRPCHK(ensure(h, h->q16, (size_t)mpad * FRP_EMB_DIM * 2));
    HIPCHK(h, hipMemsetAsync(h->q16.p, 0, (size_t)mpad * FRP_EMB_DIM * 2, h->stream));
    FRPCHK(upload_rows_normalized(h, q, M, (_Float16*)h->q16.p));
    ScopedBuf all;
    if (all_scores_host) FRPCHK(ensure(h, all, (size_t)M * h->g_rows * 4));
    int rc = run_match(h, sw, M, (float*)all->p);
    hipError_t e = hipSuccess;
    if (rc == FRP_OK) {
        if (idx) e = hipMemcpyAsync(idx, h->best_idx.p, (size_t)M * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && cos) e = hipMemcpyAsync(cos, h->best_cos.p, (size_t)M * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && all_scores_host)
            e = hipMemcpyAsync(all_scores_host, all->p, (size_t)M * h->g_rows * 4, hipMemcpyDeviceToHost, h->stream);
    }
    hipError_t e2 = hipStreamSynchronize(h->stream);
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
    h->q16_of_pass = false;
    int chunk = (int)std::max<long>(1, std::min<long>(M, (1L << 28) / N));
    ScopedBuf all, didx, dcos;
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
        if (rc == FRP_OK) rc = run_match(h, sw, m, (float*)all->p);
        if (rc != FRP_OK) break;
        e = launch_topk_rows((const float*)all->p, m, N, topk, (int32_t*)didx->p, (float*)dcos->p, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(idx + (size_t)m0 * topk, didx->p, (size_t)m * topk * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cos + (size_t)m0 * topk, dcos->p, (size_t)m * topk * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    (void)hipStreamSynchronize(h->stream);
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

int frp_match_within(frp_handle* h, const float* q, int32_t M, float min_cos, int32_t cap, int32_t* idx, float* cos, int32_t* n_hits) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!within_args_ok(min_cos, cap)) return fail(h, FRP_ERR_INVALID, "match_within: min_cos must be >= -2 and cap in 1..FRP_MAX_TOPK");
    if (!q || !idx || !cos || !n_hits || M <= 0 || M > (1 << 20)) return fail(h, FRP_ERR_INVALID, "bad query arguments");
    if (h->g_rows <= 0) return fail(h, FRP_ERR_NO_GALLERY, "gallery is empty");
    const Switches sw = read_switches();
    h->q16_of_pass = false;
    const int chunk = std::min<int>(M, 65536);
    ScopedBuf dcnt, didx, dcos;
    int rc = ensure(h, dcnt, (size_t)chunk * 4);
    if (rc == FRP_OK) rc = ensure(h, didx, (size_t)chunk * cap * 4);
    if (rc == FRP_OK) rc = ensure(h, dcos, (size_t)chunk * cap * 4);
    hipError_t e = hipSuccess;
    std::vector<int> over;
    for (int m0 = 0; rc == FRP_OK && e == hipSuccess && m0 < M; m0 += chunk) {
        const int m = std::min(chunk, M - m0);
        const int mpad = round_up(m, 32);
        int32_t* nh = n_hits + m0;
        rc = ensure(h, h->q16, (size_t)mpad * FRP_EMB_DIM * 2);
        if (rc != FRP_OK) break;
        e = hipMemsetAsync(h->q16.p, 0, (size_t)mpad * FRP_EMB_DIM * 2, h->stream);
        if (e != hipSuccess) break;
        rc = upload_rows_normalized(h, q + (size_t)m0 * FRP_EMB_DIM, m, (_Float16*)h->q16.p);
        const WithinArgs w{min_cos, cap, (int32_t*)dcnt->p, (int32_t*)didx->p, (float*)dcos->p};
        if (rc == FRP_OK) rc = run_match(h, sw, m, nullptr, nullptr, &w);
        if (rc != FRP_OK) break;
        e = hipMemcpyAsync(nh, dcnt->p, (size_t)m * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) break;
        over.clear();                       // the counts are on the host: lists that overflowed are rebuilt from their score rows
        for (int i = 0; i < m; ++i)
            if (nh[i] > cap) over.push_back(i);
        if (!over.empty()) rc = rebuild_within_lists(h, (const _Float16*)h->q16.p, over, cap, (int32_t*)didx->p, (float*)dcos->p);
        if (rc != FRP_OK) break;
        e = hipMemcpyAsync(idx + (size_t)m0 * cap, didx->p, (size_t)m * cap * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cos + (size_t)m0 * cap, dcos->p, (size_t)m * cap * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    (void)hipStreamSynchronize(h->stream);
    if (rc != FRP_OK) return rc;
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("match within: ") + hipGetErrorString(e));
    return FRP_OK;
}

// Diagnostic (tests/test_gpu_match_exact.py): run_match on queries handed over as fp16 bits - no normalisation, so a test chooses both
// operands of every product - with the count on the host (n_device < 0: with `scores` the per-tile kernel and its all_scores epilogue,
// without what launch_match routes) or in device memory (n_device >= 0: launched for the capacity M, as the threshold-mode pipeline
// does; refused wherever launch_match has no such form).  The result buffers are filled with 0xFF bytes before the launch and M
// entries are copied back: an entry no kernel wrote is recognisable.
int frp_debug_match_f16(frp_handle* h, const void* q_f16, int32_t M, int32_t n_device, int32_t* idx, float* cos, float* scores,
                        int64_t n_cols) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!q_f16 || !idx || !cos || M <= 0 || M > (1 << 20)) return fail(h, FRP_ERR_INVALID, "bad query arguments");
    if (h->g_rows <= 0) return fail(h, FRP_ERR_NO_GALLERY, "gallery is empty");
    if (scores && n_cols != h->g_rows) return fail(h, FRP_ERR_INVALID, "debug_match_f16: output sized for another gallery size");
    const Switches sw = read_switches();
    const int mpad = round_up(M, 32);
    if (n_device >= 0 && (scores || mpad > FRP_MATCH_TOP1_MAX || sw.match_v1 || n_device > M))
        return fail(h, FRP_ERR_INVALID, "debug_match_f16: no device-count form of this launch");
    h->q16_of_pass = false;
    FRPCHK(ensure(h, h->q16, (size_t)mpad * FRP_EMB_DIM * 2));
    FRPCHK(ensure(h, h->best_cos, (size_t)mpad * 4));
    FRPCHK(ensure(h, h->best_idx, (size_t)mpad * 4));
    ScopedBuf all, count;
    if (scores) FRPCHK(ensure(h, all, (size_t)M * h->g_rows * 4));
    if (n_device >= 0) FRPCHK(ensure(h, count, 4));
    HIPCHK(h, hipMemsetAsync(h->q16.p, 0, (size_t)mpad * FRP_EMB_DIM * 2, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->q16.p, q_f16, (size_t)M * FRP_EMB_DIM * 2, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->best_cos.p, 0xFF, (size_t)mpad * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(h->best_idx.p, 0xFF, (size_t)mpad * 4, h->stream));
    if (scores) HIPCHK(h, hipMemsetAsync(all->p, 0xFF, (size_t)M * h->g_rows * 4, h->stream));
    const int32_t n_host = n_device;          // (read by the copy below: alive until the synchronize at the end)
    hipError_t e = hipSuccess;
    if (n_device >= 0) e = hipMemcpyAsync(count->p, &n_host, 4, hipMemcpyHostToDevice, h->stream);
    int rc = e == hipSuccess ? run_match(h, sw, M, (float*)all->p, n_device >= 0 ? (const int32_t*)count->p : nullptr) : FRP_OK;
    if (rc == FRP_OK && e == hipSuccess) {
        e = hipMemcpyAsync(idx, h->best_idx.p, (size_t)M * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cos, h->best_cos.p, (size_t)M * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && scores) e = hipMemcpyAsync(scores, all->p, (size_t)M * h->g_rows * 4, hipMemcpyDeviceToHost, h->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(h->stream);
    if (rc != FRP_OK) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return fail(h, FRP_ERR_HIP, "debug_match_f16: copy failed");
    return FRP_OK;
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
