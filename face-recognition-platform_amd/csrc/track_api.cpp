// Face tracks, host half (frp.h: frp_track_config ...; kernels, table layout and the race argument: track_kernels.hip): configuration
// and tables, the stream of every frame, the two launch pairs of a flagged pass (track_begin in front of the embedder, track_finish
// behind the matcher: run_faces, frp_api.cpp), the fetches, and the stand-alone step of the parity tests.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "frp.h"
#include "frp_internal.h"
#include "frp_handle.h"

using namespace frp;

namespace {

int hip_rc(frp_handle* h, hipError_t e, const char* what) {
    return e == hipSuccess ? FRP_OK : fail(h, FRP_ERR_HIP, std::string(what) + hipGetErrorString(e));
}

// stream_of_frame [B] -> the streams that occur, each once, in order of first occurrence; false: an entry outside [-1, max_streams)
bool present_streams(const int32_t* s, int B, int max_streams, std::vector<int32_t>& present) {
    bool seen[FRP_TRACK_MAX_STREAMS] = {};
    present.clear();
    for (int b = 0; b < B; ++b) {
        if (s[b] < -1 || s[b] >= max_streams) return false;
        if (s[b] >= 0 && !seen[s[b]]) { seen[s[b]] = true; present.push_back(s[b]); }
    }
    return true;
}

int ensure_slots(frp_handle* h, int B, int K) {
    Tracks& t = h->trk;
    const size_t s = (size_t)B * K;
    FRPCHK(ensure(h, t.slot_i32, s * 5 * 4));
    FRPCHK(ensure(h, t.slot_emb, s * FRP_EMB_DIM * 4));
    FRPCHK(ensure(h, t.slot_idx, s * 4));
    FRPCHK(ensure(h, t.slot_cos, s * 4));
    return FRP_OK;
}

// configuration, state and the per-slot arrays (ensure_slots) of a pass over B x K slots; the caller adds the batch and the results
TrackParams base_params(frp_handle* h, int B, int K) {
    Tracks& t = h->trk;
    TrackParams p{};
    p.max_streams = t.max_streams; p.iou_min = t.iou_min; p.refresh = t.refresh; p.max_missed = t.max_missed; p.stale = t.stale ? 1 : 0;
    p.hdr = (TrackHeader*)t.hdr.p; p.meta = (TrackEntry*)t.meta.p; p.tab_emb = (float*)t.tab_emb.p; p.plan = (TrackPlan*)t.plan.p;
    p.totals = (int64_t*)t.totals.p;
    p.B = B; p.K = K;
    const size_t s = (size_t)B * K;
    int32_t* i32 = (int32_t*)t.slot_i32.p;
    p.track_id = i32; p.reused = i32 + s; p.age = i32 + 2 * s; p.src = i32 + 3 * s; p.pos = i32 + 4 * s;
    p.slot_emb = (float*)t.slot_emb.p; p.slot_idx = (int32_t*)t.slot_idx.p; p.slot_cos = (float*)t.slot_cos.p;
    return p;
}

// ... of a pass of the pipeline: the frame streams of frp_set_frame_streams, the detections and the embed list of the handle
TrackParams pass_params(frp_handle* h, int B, int K) {
    TrackParams p = base_params(h, B, K);
    p.streams = (const int32_t*)h->trk.streams_dev.p;
    p.present = p.streams + B;
    p.n_present = (int)h->trk.present.size();
    p.boxes = (const float*)h->boxes.p; p.counts = (const int32_t*)h->counts.p;
    p.face_slot = (int32_t*)h->face_slot.p; p.nfaces = (int32_t*)h->nfaces.p;
    return p;
}

int wait_streams_copy(frp_handle* h) {
    Tracks& t = h->trk;
    if (t.streams_copying) {          // a pass's upload may still be reading the vector
        HIPCHK(h, hipEventSynchronize(t.streams_ev));
        t.streams_copying = false;
    }
    return FRP_OK;
}

}  // namespace

int frp::track_check(frp_handle* h, uint32_t flags, int B) {
    if (!(flags & FRP_FLAG_TRACK)) return FRP_OK;
    const Tracks& t = h->trk;
    if (t.max_streams <= 0) return fail(h, FRP_ERR_INVALID, "FRP_FLAG_TRACK: call frp_track_config first");
    if (flags & (FRP_FLAG_WITHIN | FRP_FLAG_GROUPS)) return fail(h, FRP_ERR_INVALID, "FRP_FLAG_TRACK does not combine with FRP_FLAG_WITHIN / FRP_FLAG_GROUPS");
    if (t.streams.empty()) return fail(h, FRP_ERR_INVALID, "FRP_FLAG_TRACK: call frp_set_frame_streams first");
    if ((int)t.streams.size() - (int)t.present.size() != B) return fail(h, FRP_ERR_INVALID, "FRP_FLAG_TRACK: frp_set_frame_streams was called for another B");
    if (B > 1024) return fail(h, FRP_ERR_INVALID, "FRP_FLAG_TRACK: more than 1024 frames");
    return FRP_OK;
}

int frp::track_begin(frp_handle* h, int B, int K) {
    Tracks& t = h->trk;
    FRPCHK(ensure_slots(h, B, K));
    FRPCHK(ensure(h, t.streams_dev, t.streams.size() * 4));
    if (t.streams_dirty) {
        HIPCHK(h, hipMemcpyAsync(t.streams_dev.p, t.streams.data(), t.streams.size() * 4, hipMemcpyHostToDevice, h->stream));
        if (!t.streams_ev) HIPCHK(h, hipEventCreateWithFlags(&t.streams_ev, hipEventDisableTiming));
        HIPCHK(h, hipEventRecord(t.streams_ev, h->stream));
        t.streams_copying = true;
        t.streams_dirty = false;
    }
    const TrackParams p = pass_params(h, B, K);
    FRPCHK(hip_rc(h, launch_track_associate(p, h->stream), "track_associate: "));
    t.stale = false;          // this pass embeds every face; the next one may reuse
    t.B = B; t.K = K;
    return FRP_OK;
}

int frp::track_finish(frp_handle* h, bool matched) {
    TrackParams p = pass_params(h, h->trk.B, h->trk.K);
    const void* e = h->hdr.emb_out_buf < h->emb.bufs.size() ? h->emb.bufs[h->hdr.emb_out_buf].p : nullptr;
    p.emb = e ? (const float*)e : p.slot_emb;          // (no embedder buffer yet: nothing was ever embedded, no slot has a compact position)
    if (matched) { p.best_idx = (const int32_t*)h->m.best_idx.p; p.best_cos = (const float*)h->m.best_cos.p; }
    return hip_rc(h, launch_track_resolve(p, h->stream), "track_resolve: ");
}

void frp::release_tracks(frp_handle* h) {
    Tracks& t = h->trk;
    DevBuf* all[] = {&t.hdr, &t.meta, &t.tab_emb, &t.plan, &t.totals, &t.streams_dev, &t.slot_i32, &t.slot_emb, &t.slot_idx, &t.slot_cos};
    for (DevBuf* b : all) release(*b);
    if (t.streams_ev) (void)hipEventDestroy(t.streams_ev);
    t = Tracks{};
}

extern "C" {

int frp_track_config(frp_handle* h, int32_t max_streams, float iou_min, int32_t refresh, int32_t max_missed) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    Tracks& t = h->trk;
    if (max_streams == 0) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        release_tracks(h);
        return FRP_OK;
    }
    if (max_streams < 1 || max_streams > FRP_TRACK_MAX_STREAMS || !(iou_min > 0.f && iou_min <= 1.f) || refresh < 1 || max_missed < 0)
        return fail(h, FRP_ERR_INVALID, "track_config: max_streams 1..64, 0 < iou_min <= 1, refresh >= 1, max_missed >= 0");
    const size_t rows = (size_t)max_streams * 2 * FRP_TRACK_SLOTS;
    FRPCHK(ensure(h, t.hdr, (size_t)max_streams * sizeof(TrackHeader)));
    FRPCHK(ensure(h, t.plan, (size_t)max_streams * sizeof(TrackPlan)));
    FRPCHK(ensure(h, t.meta, rows * sizeof(TrackEntry)));
    FRPCHK(ensure(h, t.tab_emb, rows * FRP_EMB_DIM * 4));
    FRPCHK(ensure(h, t.totals, 16));
    HIPCHK(h, hipMemsetAsync(t.hdr.p, 0, (size_t)max_streams * sizeof(TrackHeader), h->stream));
    HIPCHK(h, hipMemsetAsync(t.plan.p, 0, (size_t)max_streams * sizeof(TrackPlan), h->stream));
    HIPCHK(h, hipMemsetAsync(t.totals.p, 0, 16, h->stream));
    if (max_streams != t.max_streams) {          // the frame streams were checked against the former range
        FRPCHK(wait_streams_copy(h));
        t.streams.clear(); t.present.clear();
    }
    t.max_streams = max_streams; t.iou_min = iou_min; t.refresh = refresh; t.max_missed = max_missed;
    t.stale = true;
    return FRP_OK;
}

int frp_set_frame_streams(frp_handle* h, const int32_t* stream_of_frame, int32_t B) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    Tracks& t = h->trk;
    if (t.max_streams <= 0) return fail(h, FRP_ERR_INVALID, "set_frame_streams: call frp_track_config first");
    if (!stream_of_frame || B <= 0 || B > 1024) return fail(h, FRP_ERR_INVALID, "set_frame_streams: B streams, 1 <= B <= 1024");
    std::vector<int32_t> present;
    if (!present_streams(stream_of_frame, B, t.max_streams, present)) return fail(h, FRP_ERR_INVALID, "set_frame_streams: a stream outside [-1, max_streams)");
    if ((int)t.streams.size() == B + (int)present.size() && std::equal(stream_of_frame, stream_of_frame + B, t.streams.begin())) return FRP_OK;
    FRPCHK(wait_streams_copy(h));
    t.streams.assign(stream_of_frame, stream_of_frame + B);          // [B streams | the streams that occur]
    t.streams.insert(t.streams.end(), present.begin(), present.end());
    t.present = present;
    t.streams_dirty = true;
    return FRP_OK;
}

int frp_track_reset(frp_handle* h, int32_t stream) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    Tracks& t = h->trk;
    if (t.max_streams <= 0) return fail(h, FRP_ERR_INVALID, "track_reset: call frp_track_config first");
    if (stream < -1 || stream >= t.max_streams) return fail(h, FRP_ERR_INVALID, "track_reset: stream out of range");
    if (stream < 0) HIPCHK(h, hipMemsetAsync(t.hdr.p, 0, (size_t)t.max_streams * sizeof(TrackHeader), h->stream));
    else HIPCHK(h, hipMemsetAsync((TrackHeader*)t.hdr.p + stream, 0, sizeof(TrackHeader), h->stream));
    return FRP_OK;
}

int frp_fetch_tracks(frp_handle* h, int32_t B, int32_t max_faces, int32_t* track_id, int32_t* reused, int32_t* age) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    Tracks& t = h->trk;
    if (t.B <= 0) return fail(h, FRP_ERR_INVALID, "fetch_tracks: no tracked pass");
    if (B != t.B || max_faces != t.K) return fail(h, FRP_ERR_INVALID, "fetch_tracks: buffers sized for another batch");
    const size_t s = (size_t)B * max_faces;
    const int32_t* i32 = (const int32_t*)t.slot_i32.p;
    if (track_id) HIPCHK(h, hipMemcpyAsync(track_id, i32, s * 4, hipMemcpyDeviceToHost, h->stream));
    if (reused) HIPCHK(h, hipMemcpyAsync(reused, i32 + s, s * 4, hipMemcpyDeviceToHost, h->stream));
    if (age) HIPCHK(h, hipMemcpyAsync(age, i32 + 2 * s, s * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

int frp_track_stats(frp_handle* h, int64_t* embedded, int64_t* reused) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    if (h->trk.max_streams <= 0) return fail(h, FRP_ERR_INVALID, "track_stats: call frp_track_config first");
    int64_t v[2] = {0, 0};
    HIPCHK(h, hipMemcpyAsync(v, h->trk.totals.p, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (embedded) *embedded = v[0];
    if (reused) *reused = v[1];
    return FRP_OK;
}

int frp_debug_track_step(frp_handle* h, const int32_t* streams, const float* boxes, const int32_t* counts, int32_t B, int32_t K,
                         const float* emb_in, const int32_t* idx_in, const float* cos_in, int32_t* track_id, int32_t* reused,
                         int32_t* age, int32_t* face_slot, int32_t* n_embed, float* emb, int32_t* idx, float* cos) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    Tracks& t = h->trk;
    if (t.max_streams <= 0) return fail(h, FRP_ERR_INVALID, "debug_track_step: call frp_track_config first");
    if (!streams || !boxes || !counts || !emb_in || !idx_in || !cos_in || B <= 0 || B > 1024 || K <= 0 || K > FRP_MAX_FACES_CAP)
        return fail(h, FRP_ERR_INVALID, "debug_track_step: bad arguments");
    std::vector<int32_t> present;
    if (!present_streams(streams, B, t.max_streams, present)) return fail(h, FRP_ERR_INVALID, "debug_track_step: a stream outside [-1, max_streams)");
    const size_t s = (size_t)B * K;
    // in: streams | present | counts | face_slot | nfaces, boxes; the stand-in results, compact
    std::vector<int32_t> hi(B + present.size() + B);
    memcpy(hi.data(), streams, (size_t)B * 4);
    if (!present.empty()) memcpy(hi.data() + B, present.data(), present.size() * 4);
    memcpy(hi.data() + B + present.size(), counts, (size_t)B * 4);
    ScopedBuf di, dbox, demb, didx, dcos;
    const int rc = [&]() -> int {
        FRPCHK(ensure_slots(h, B, K));
        FRPCHK(ensure(h, di, (hi.size() + s + 4) * 4));
        FRPCHK(ensure(h, dbox, s * 16));
        FRPCHK(ensure(h, demb, s * FRP_EMB_DIM * 4));
        FRPCHK(ensure(h, didx, s * 4));
        FRPCHK(ensure(h, dcos, s * 4));
        HIPCHK(h, hipMemcpyAsync(di->p, hi.data(), hi.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(dbox->p, boxes, s * 16, hipMemcpyHostToDevice, h->stream));
        TrackParams p = base_params(h, B, K);
        int32_t* d = (int32_t*)di->p;
        p.streams = d; p.present = d + B; p.n_present = (int)present.size();
        p.counts = d + B + present.size();
        p.face_slot = d + hi.size(); p.nfaces = p.face_slot + s;
        p.boxes = (const float*)dbox->p;
        FRPCHK(hip_rc(h, launch_track_associate(p, h->stream), "track_associate: "));
        t.stale = false;
        t.B = B; t.K = K;
        std::vector<int32_t> fs(s + 1);
        HIPCHK(h, hipMemcpyAsync(fs.data(), p.face_slot, (s + 1) * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const int n = fs[s];
        if (n < 0 || n > (int)s) return fail(h, FRP_ERR_HIP, "debug_track_step: corrupt embed count");
        std::vector<float> ce((size_t)std::max(n, 1) * FRP_EMB_DIM), cc(std::max(n, 1));
        std::vector<int32_t> ci(std::max(n, 1));
        for (int f = 0; f < n; ++f) {
            const int sl = fs[f];
            if (sl < 0 || sl >= (int)s) return fail(h, FRP_ERR_HIP, "debug_track_step: corrupt embed list");
            memcpy(&ce[(size_t)f * FRP_EMB_DIM], emb_in + (size_t)sl * FRP_EMB_DIM, FRP_EMB_DIM * 4);
            ci[f] = idx_in[sl]; cc[f] = cos_in[sl];
        }
        if (n > 0) {
            HIPCHK(h, hipMemcpyAsync(demb->p, ce.data(), (size_t)n * FRP_EMB_DIM * 4, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(didx->p, ci.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(dcos->p, cc.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        }
        p.emb = (const float*)demb->p; p.best_idx = (const int32_t*)didx->p; p.best_cos = (const float*)dcos->p;
        FRPCHK(hip_rc(h, launch_track_resolve(p, h->stream), "track_resolve: "));
        if (track_id) HIPCHK(h, hipMemcpyAsync(track_id, p.track_id, s * 4, hipMemcpyDeviceToHost, h->stream));
        if (reused) HIPCHK(h, hipMemcpyAsync(reused, p.reused, s * 4, hipMemcpyDeviceToHost, h->stream));
        if (age) HIPCHK(h, hipMemcpyAsync(age, p.age, s * 4, hipMemcpyDeviceToHost, h->stream));
        if (emb) HIPCHK(h, hipMemcpyAsync(emb, p.slot_emb, s * FRP_EMB_DIM * 4, hipMemcpyDeviceToHost, h->stream));
        if (idx) HIPCHK(h, hipMemcpyAsync(idx, p.slot_idx, s * 4, hipMemcpyDeviceToHost, h->stream));
        if (cos) HIPCHK(h, hipMemcpyAsync(cos, p.slot_cos, s * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (face_slot)
            for (size_t f = 0; f < s; ++f) face_slot[f] = (int)f < n ? fs[f] : -1;
        if (n_embed) *n_embed = n;
        return FRP_OK;
    }();
    if (rc != FRP_OK) (void)hipStreamSynchronize(h->stream);          // the uploads read the caller's arrays, the temporaries go next
    return rc;
}

}  // extern "C"
