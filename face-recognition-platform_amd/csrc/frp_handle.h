// The engine handle and the helpers every host translation unit uses on it (host only: the kernels' shared header is frp_internal.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "frp.h"
#include "frp_blob.h"
#include "frp_internal.h"
#include "net_program.h"

enum { EV_START = 0, EV_H2D, EV_PRE, EV_DET, EV_DEC, EV_ALIGN, EV_EMB, EV_L2, EV_MATCH, EV_D2H, EV_COUNT };

struct Ingest {   // frame ingest (ingest_api.cpp: nothing else reads or writes these; init_ingest / release_ingest make and free them)
    // overlapped ingest: the NEXT batch is copied on its own stream while the current one is processed
    frp::DevBuf frames_next;
    int nB = 0, nH = 0, nW = 0;
    bool next_valid = false;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_next_ready = nullptr, ev_next_free = nullptr;
    std::vector<void*> pinned;       // frp_host_alloc blocks, freed with the handle
    // JPEG ingest (frp_upload_jpeg_async): page-locked coefficient staging, device coefficients / tables / sample planes
    // (two staging buffers in turn: the host decodes batch t+1 while the copy of batch t still reads the other one)
    void* jpeg_pin[2] = {nullptr, nullptr};
    size_t jpeg_pin_cap[2] = {0, 0};
    int jpeg_turn = 0;
    frp::DevBuf jpeg_coef, jpeg_planes;
    int64_t ctr_jpeg_device_batches = 0;   // batches whose entropy decode ran on the device (frp_debug_jpeg_device_batches)
    frp::DevBuf jpeg_scan, jpeg_err;      // device entropy decode (restart-interval streams): compressed scans + interval offsets + tables; per-image error flags
    // self-synchronising entropy decode (streams without restart markers; frp_set_jpeg_selfsync, default: FRP_JPEG_SELFSYNC): per
    // subsequence its entry / exit state, blocks completed and first block, the workgroups' boundary states (ingest_api.cpp: decode_selfsync);
    // jpeg_err then holds [B][4] statistics with the error flag last
    bool jpeg_selfsync = false;
    int jpeg_selfsync_bytes = 0;            // subsequence size where the caller set one (measurements), 0: the product's
    int64_t ctr_jpeg_selfsync_batches = 0;  // batches decoded by it (frp_debug_jpeg_selfsync_batches)
    frp::DevBuf jpeg_ss;
    hipEvent_t ev_jpeg_h2d[2] = {nullptr, nullptr};     // the copy out of jpeg_pin[i] has finished
    bool jpeg_h2d_pending[2] = {false, false};
    // YUV 4:2:0 ingest (frp_upload_yuv / frp_upload_yuv_async): host planes are copied into yuv_stage (packed, W * H * 3 / 2 bytes per
    // frame); the kernel finds every frame's planes - there or in the caller's device surfaces - through a table of addresses.  The table
    // has two turns: yuv_pin (page-locked, both turns) is the source of an asynchronous copy into the turn's half of yuv_tab, and
    // ev_yuv[turn], recorded behind the turn's kernel, says that the copy has read the one and the kernel the other (and yuv_stage).
    frp::DevBuf yuv_stage, yuv_tab;
    void* yuv_pin = nullptr;
    int yuv_turn = 0;
    hipEvent_t ev_yuv[2] = {nullptr, nullptr};
    bool yuv_pending[2] = {false, false};
};

// The matcher's host half (match_api.cpp).  Other readers: fetch_results (frp_api.cpp) copies best_idx / best_cos of the pass out,
// the pipeline refuses a flagged pass while within_cap is 0, frp_destroy releases the buffers.
struct Matcher {
    frp::DevBuf q16;                                     // [round_up(n, 32), 512] unit fp16 queries, zero padded (stage_queries)
    frp::DevBuf part_cos, part_idx, best_cos, best_idx;  // per-workgroup partial and final top-1 (fill_match_params)
    // radius match (frp_set_within, FRP_FLAG_WITHIN): bound and list size for the flagged passes to come; the lists of the last one
    float within_min_cos = 0.f;
    int within_cap = 0;                                  // 0: frp_set_within has not been called
    frp::DevBuf hit_cnt, hit_idx, hit_cos;               // [n], [n x cap], [n x cap] per compact face of the last flagged pass
    // gallery groups (frp_match_groups, FRP_FLAG_GROUPS): the query masks of the last grouped launch, [round_up(n, 32)] - of a pass:
    // one per compact face (launch_face_groups), alive as long as q16 holds the pass's queries (a rebuilt list needs both)
    frp::DevBuf q_groups;
    // frp_set_frame_groups: the frame masks for the flagged passes to come (empty: not set) and their device copy, uploaded by the
    // first pass after a change; frame_groups_ev: that copy has read the host vector (waited for before the vector changes again)
    std::vector<uint32_t> frame_groups;
    frp::DevBuf frame_groups_dev;
    bool frame_groups_dirty = false, frame_groups_copying = false;
    hipEvent_t frame_groups_ev = nullptr;
};

// Face tracks (track_api.cpp; kernels and table layout: track_kernels.hip).  Other readers: run_faces and fetch_results (frp_api.cpp)
// through track_begin / track_finish / the per-slot arrays; the gallery entry points set `stale`; frp_destroy releases the buffers.
struct Tracks {
    int max_streams = 0;                 // 0: frp_track_config has not been called (or released everything)
    float iou_min = 0.f;
    int refresh = 0, max_missed = 0;
    // the next tracked pass embeds every face: a cached match_idx must never outlive a row move (set by frp_track_config, every
    // gallery mutation and frp_gallery_exact; cleared where a tracked pass is queued)
    bool stale = false;
    frp::DevBuf hdr, meta, tab_emb, plan, totals;      // TrackParams: per-stream headers, table halves, plans; the two totals
    // frp_set_frame_streams: the stream of every frame for the flagged passes to come (empty: not set), the streams that occur, and
    // their device copy [B + n_present], uploaded by the first pass after a change (life cycle of Matcher::frame_groups)
    std::vector<int32_t> streams, present;
    frp::DevBuf streams_dev;
    bool streams_dirty = false, streams_copying = false;
    hipEvent_t streams_ev = nullptr;
    // the last tracked pass: its shape and its per-slot arrays - slot_i32 = track_id | reused | age | src | pos, [B x K] each
    int B = 0, K = 0;
    frp::DevBuf slot_i32, slot_emb, slot_idx, slot_cos;
};

// Everything that describes the last pass, i.e. what the handle's result buffers hold.  Started as a whole where a pass begins
// (run_faces; the detect-only entry points), never field by field: a new pass cannot inherit a flag of the one before.
struct Pass {
    int B = 0, K = 0;            // shape of the result slots
    int nfaces = 0;              // faces of the pass; -1: the count is still on the device (settle_count)
    int cap = 0;                 // the most faces it can hold: the count where the host knew it at the start, else B x K
    bool matched = false;        // best_idx / best_cos hold its top-1
    int within_cap = 0;          // list size of the pass, 0: it ran without FRP_FLAG_WITHIN
    bool within_lists = false;   // ... and it matched (faces and a gallery): hit_* hold its lists
    bool q16_of_pass = false;    // q16 still holds its queries (a list that overflowed is rebuilt from them at fetch time)
    bool groups = false;         // it matched with FRP_FLAG_GROUPS: q_groups holds its faces' masks
    // FRP_FLAG_TRACK: nfaces counts the EMBEDDED faces; every live slot's emb / idx / cos are in Tracks' per-slot arrays (fetch_results
    // reads them instead of scattering the compact results).  track_matched: the pass wanted a match (flags and a gallery) - reused
    // slots carry one also where nothing was embedded, so `matched` alone does not say it
    bool tracked = false, track_matched = false;
    // device-count pass: the embedder's FLOPs were charged for pend_cap faces, corrected once the count is known (settle_count)
    int pend_cap = 0;
    double pend_flops = 0.0, pend_f8flops = 0.0;
};

struct frp_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string err;
    frp_config cfg{};
    // weights
    bool have_weights = false;
    frp_blob_header hdr{};
    frp::DevBuf wdata;
    frp::Net det, emb;
    // resident frames (tightly packed u8 [B,H,W,3])
    frp::DevBuf frames;
    int rB = 0, rH = 0, rW = 0;
    int n_cu = 256;                   // compute units of the device (queried once at create)
    Ingest in;                        // the staged NEXT batch, the copy stream, the JPEG staging
    // detector source: the resident frames, or a resized copy of them (pyramid scales)
    frp::DevBuf scaled;
    int dH = 0, dW = 0;              // dims of the detector source
    bool det_scaled = false;
    int canvas_h = 0, canvas_w = 0;
    int det_op_limit = -1;           // >= 0: frp_debug_det_prefix - the detector program stops behind this many ops
    // captured passes (run_net): graphs, the keys seen once (a pass is captured the SECOND time it is asked for: the first allocates and
    // sets kernel attributes), the keys whose capture failed, the allocation epoch
    std::vector<frp::NetGraph> graphs;
    std::vector<std::string> graph_seen, graph_bad;
    uint64_t alloc_epoch = 1;
    int64_t graph_replays = 0;
    // multi-GPU (frp_dist_init): this handle's RCCL communicator, rank and world size
    void* comm = nullptr;
    int dist_rank = 0, dist_world = 0;
    frp::DevBuf det_hashes;               // frp_debug_det_hashes: one 64-bit hash per detector op, taken right behind the op
    bool det_hash_on = false;
    // per-call results (device)
    frp::DevBuf boxes, kps, scores, counts, anchor, face_slot, nfaces, scratch, splitk_ws, dense_logits;
    // frp_process_pyramid: every scale's detections, scale-major [S][B][P]... (the merge kernel's input; the merged faces go to the buffers above)
    frp::DevBuf pyr_boxes, pyr_kps, pyr_scores, pyr_counts;
    Matcher m;                 // queries, work buffers and hit lists of the matcher
    Pass pass;                 // what the buffers above hold: the last pass
    Tracks trk;                // face tracks: configuration, per-stream tables, the last tracked pass's per-slot results
    bool ev_pending = false;   // frp_process_resident's stage events are recorded but not yet read (see settle_events)
    // frp_face_quality: rectangles + tile prefix in, per-tile partials + per-rectangle sums out (its own: the last pass's results stay)
    frp::DevBuf quality_in, quality_out;
    // frp_encode_jpeg: rectangles + tables in, quantised coefficients, the scans' work arrays, the unstuffed bit stream, the files (its own)
    frp::DevBuf jenc_in, jenc_coef, jenc_work, jenc_bits, jenc_out;
    // frp_enhance_pixels / frp_encode_jpeg_enhanced: images + tap tables in, the enhanced pixels (the encoder's source in the second) (its own)
    frp::DevBuf enh_in, enh_out;
    int32_t* h_nfaces = nullptr;   // pinned: the face count of a device-count pass, copied behind it (read by settle_count alone)
    unsigned char* pin_stage = nullptr;   // pinned staging of the result fetch
    size_t pin_cap = 0;
    // gallery snapshot
    frp::DevBuf gallery;
    int64_t g_rows = 0;
    frp::DevBuf g_reserved;               // frp_gallery_reserve: filled by the caller, swapped in by frp_gallery_commit
    // exact compat rows (frp_gallery_exact): float64 [g_rows x 512] as enrolled, next to the unit fp16 snapshot
    bool g_exact = false;
    frp::DevBuf gx, gx_q, gx_out;
    // gallery groups: one mask per row, ALL unless frp_gallery_set_groups said otherwise.  The host table is what the entry points
    // edit and read; g_groups_dev is its device copy for the grouped kernels - [>= round_up(g_rows, 32)], rows >= g_rows hold 0 -
    // built by the first grouped match behind a new snapshot (row_groups_device) and patched in place by the single-row updates
    std::vector<uint32_t> g_groups;
    frp::DevBuf g_groups_dev;
    bool g_groups_dev_ok = false;
    // profiling
    hipEvent_t ev[EV_COUNT]{};
    frp_counters ctr{};
};

namespace frp {

inline int fail(frp_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

#define HIPCHK(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            return fail(h, FRP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
    } while (0)

#define FRPCHK(expr)                 \
    do {                             \
        int _r = (expr);             \
        if (_r != FRP_OK) return _r; \
    } while (0)

inline int ensure(frp_handle* h, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap && b.p) return FRP_OK;
    if (b.p) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    const size_t want = std::max<size_t>(bytes, 256);
    ++h->alloc_epoch;                   // (captured passes hold device pointers)
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(h, FRP_ERR_OOM, std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
    }
    b.cap = want;
    return FRP_OK;
}

inline void release(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

#define FRP_LOCAL __attribute__((visibility("hidden")))   // shared between the host files, not one of the library's exports

// A function-local device buffer: freed when it goes out of scope, on error returns too.  The only ways at the allocation are
// ensure() below, reads through ->, and take(), which hands it on to a handle member: no copy can leave a second owner.
// (A free behind unfinished work relies on hipFree waiting for the device, as release() always did.)
class FRP_LOCAL ScopedBuf {
    DevBuf b;
    friend int ensure(frp_handle* h, ScopedBuf& s, size_t bytes) { return ensure(h, s.b, bytes); }

public:
    ScopedBuf() = default;
    ScopedBuf(const ScopedBuf&) = delete;
    ScopedBuf& operator=(const ScopedBuf&) = delete;
    ~ScopedBuf() { release(b); }
    const DevBuf* operator->() const { return &b; }
    DevBuf take() { return std::exchange(b, DevBuf()); }
};

// What the files of entry points share (frp_api.cpp, match_api.cpp, ingest_api.cpp, gallery_api.cpp, kernel_api.cpp, quality_api.cpp,
// jpeg_encode_api.cpp, enhance_api.cpp)
FRP_LOCAL void settle_events(frp_handle* h, bool stream_is_idle);   // frp_api.cpp
// frp_api.cpp: the pending face count of a device-count pass - waits for the stream unless it is idle, reads the count, corrects the
// counters.  Called by whatever reuses or discards the pass's slots (h_nfaces, Pass) or needs its count; a no-op otherwise.
FRP_LOCAL int settle_count(frp_handle* h, bool stream_is_idle);
FRP_LOCAL int ensure_pinned(frp_handle* h, size_t bytes);           // frp_api.cpp: h->pin_stage, the page-locked staging of the fetches
// match_api.cpp: q16 holds n zero-padded queries behind this - unit rows made of `rows` (host fp32), the fp16 bits `f16` (host) as they
// are, or, with neither, whatever the caller launches next (run_embed: the l2norm); the last pass's queries are gone
FRP_LOCAL int stage_queries(frp_handle* h, int n, const float* rows = nullptr, const void* f16 = nullptr);
// match_api.cpp: the match of a pass (run_faces) - top-1 of the n queries in q16 (n_dev: the count in device memory) and, `within`,
// the hit lists of frp_set_within in the same launch; marks the pass as matched
// `groups`: over the rows the frame mask of each face permits (frp_set_frame_groups; the caller has checked that B masks are set)
FRP_LOCAL int match_pass(frp_handle* h, const frp::Switches& sw, int n, const int32_t* n_dev, bool within, bool groups);
// match_api.cpp: the score rows of the n unit fp16 queries at q16 (device, [round_up(n, 32), 512], zero padded) against the gallery ->
// all_scores [n x g_rows] (device), by the per-tile kernel's all_scores epilogue: the bits frp_match_scores returns; counted in ctr.match_*.
// work: the launch's partial / top-1 buffers, grown to fit - the caller's own, so the handle's last results stay (frp_gallery_cluster)
FRP_LOCAL int match_score_rows(frp_handle* h, const void* q16, int n, ScopedBuf (&work)[4], float* all_scores, const char* what);
// gallery_api.cpp: the row masks in device memory, for a grouped match launch (built or brought up to date where they are not)
FRP_LOCAL int row_groups_device(frp_handle* h, const uint32_t** out);
inline void rec(frp_handle* h, int which) { if (h->cfg.profile) (void)hipEventRecord(h->ev[which], h->stream); }   // a stage event (timers on)
// track_api.cpp: a pass with FRP_FLAG_TRACK over B frames can run (configured, streams set for B, no flag it does not combine with)
FRP_LOCAL int track_check(frp_handle* h, uint32_t flags, int B);
// ... its associate + compact launches on the detections in h->boxes / h->counts: face_slot / nfaces list the faces to embed
FRP_LOCAL int track_begin(frp_handle* h, int B, int K);
// ... its resolve + store launches behind the matcher (`matched`: best_idx / best_cos hold the embedded faces' top-1)
FRP_LOCAL int track_finish(frp_handle* h, bool matched);
FRP_LOCAL void release_tracks(frp_handle* h);                       // frp_destroy
FRP_LOCAL bool init_ingest(frp_handle* h);                          // ingest_api.cpp: the copy stream and its events (frp_create)
FRP_LOCAL void release_ingest(frp_handle* h);                       // ... and everything `in` holds (frp_destroy)
FRP_LOCAL int upload_frames(frp_handle* h, const uint8_t* bgr, int B, int H, int W, int64_t row_stride);   // into the resident buffer, stream-ordered
FRP_LOCAL void set_resident(frp_handle* h, int B, int H, int W);    // B frames of H x W are resident now; the detector reads them at full size
// host fp32 rows -> unit fp16 rows at dst (device), via the scratch buffer (gallery_api.cpp)
FRP_LOCAL int upload_rows_normalized(frp_handle* h, const float* rows, int64_t n, _Float16* dst);
FRP_LOCAL void dist_shutdown(frp_handle* h);                        // gallery_api.cpp: drops the handle's RCCL communicator, if any
// jpeg_encode_api.cpp, shared with enhance_api.cpp.  The rectangle check of frp_encode_jpeg (FRP_ERR_INVALID and a message that names
// rectangle i); then the encoder on n images that lie in a device buffer other than the resident frames: plan_buffer checks the
// encoder's arguments and lays the images out (nothing launched), the caller sets p.frames / p.total_bytes and queues whatever
// fills the buffer, files queues the encoder behind it and waits (offsets / out as in frp_encode_jpeg; optimize: FRP_FLAG_JPEG_OPTIMIZE)
struct JpegEncSource { long long pix0; int pitch, w, h; };          // first pixel (index into the buffer), pixels per row, size
FRP_LOCAL int jpeg_enc_check_rect(frp_handle* h, const std::string& who, const int32_t* rects, int32_t i);
FRP_LOCAL int jpeg_enc_plan_buffer(frp_handle* h, const std::string& who, const JpegEncSource* src, int32_t n, int quality, int subsampling,
                                   int restart_mcus, uint32_t flags, std::vector<JpegEncImage>& img, JpegEncParams& p);
FRP_LOCAL int jpeg_enc_files(frp_handle* h, const std::string& who, const std::vector<JpegEncImage>& img, JpegEncParams& p, int quality,
                             bool optimize, uint8_t* out, int64_t out_cap, int64_t* offsets);

// every entry point's first statement: the handle's mutex, its device, and - unless the call only touches the copy stream - the stage
// events of a pass nobody has read yet
struct Guard {
    std::lock_guard<std::mutex> lk;
    explicit Guard(frp_handle* h, bool settle = true) : lk(h->mu) {
        (void)hipSetDevice(h->device);
        if (settle) settle_events(h, false);
    }
};

}  // namespace frp
