// Frame ingest of libfrp.so: the blocking upload into the resident buffer, the staged upload of the NEXT batch on the copy stream (raw
// frames out of pageable or page-locked memory; JPEG stills with the entropy decode on host threads or on the device; YUV 4:2:0 surfaces
// of a decoder out of host or device memory), the swap that
// makes the staged batch resident.  Everything here works on h->in (frp_handle.h: struct Ingest); the pass that reads the resident
// frames: frp_api.cpp.  Sizes and offsets of the JPEG buffers: jpeg_host.cpp (jpeg_batch_layout, jpeg_device_stage_layout).
#include <atomic>
#include <cstring>
#include <initializer_list>
#include <thread>

#include "frp_handle.h"
#include "jpeg_host.h"
#include "jpeg_selfsync.h"

using namespace frp;

bool frp::init_ingest(frp_handle* h) {
    Ingest& in = h->in;
    in.jpeg_selfsync = process_switches().jpeg_selfsync;
    // The copy stream gets its own PRIORITY class: the runtime multiplexes the streams of one class onto a few hardware
    // queues (4 by default), and next to torch's and RCCL's streams in the process the staged upload shared a queue with
    // the compute stream and serialised behind the step's kernels (overlapped loop 18.7-20.6 instead of 14.7 ms per
    // step; GPU_MAX_HW_QUEUES=8 restored it).  A stream of another priority class is not pooled with them.
    int lo = 0, hi = 0;
    bool ok;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo)
        ok = hipStreamCreateWithPriority(&in.copy_stream, hipStreamNonBlocking, hi) == hipSuccess;
    else
        ok = hipStreamCreateWithFlags(&in.copy_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&in.ev_next_ready, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&in.ev_next_free, hipEventDisableTiming) == hipSuccess;
    return ok;
}

void frp::release_ingest(frp_handle* h) {       // (frp_destroy has waited for both streams)
    Ingest& in = h->in;
    for (DevBuf* b : {&in.frames_next, &in.jpeg_coef, &in.jpeg_planes, &in.jpeg_scan, &in.jpeg_err, &in.jpeg_ss, &in.yuv_stage, &in.yuv_tab}) release(*b);
    if (in.yuv_pin) (void)hipHostFree(in.yuv_pin);
    for (void* p : in.pinned) (void)hipHostFree(p);
    for (void* p : in.jpeg_pin)
        if (p) (void)hipHostFree(p);
    for (hipEvent_t e : {in.ev_jpeg_h2d[0], in.ev_jpeg_h2d[1], in.ev_yuv[0], in.ev_yuv[1], in.ev_next_ready, in.ev_next_free})
        if (e) (void)hipEventDestroy(e);
    if (in.copy_stream) (void)hipStreamDestroy(in.copy_stream);
}

void frp::set_resident(frp_handle* h, int B, int H, int W) {
    h->rB = B; h->rH = H; h->rW = W;
    h->dH = H; h->dW = W; h->det_scaled = false;
    h->canvas_h = round_up(H, 32);
    h->canvas_w = round_up(W, 32);
}

namespace {

int check_frames(frp_handle* h, const uint8_t* bgr, int B, int H, int W, int64_t row_stride) {
    if (!bgr || B <= 0 || H <= 0 || W <= 0 || row_stride < (int64_t)W * 3) return fail(h, FRP_ERR_INVALID, "bad frame arguments");
    if (B > 1024) return fail(h, FRP_ERR_INVALID, "batch too large (max 1024 frames per call)");
    return FRP_OK;
}

// The staging sequence of a batch: grow_staged, begin_staging, its copies and kernels on the copy stream, end_staging (not reached on
// an error return: the staged dims and next_valid stay).  Growing buffers: nothing may still be copying into / computing from them, so
// BOTH streams are waited for first (ensure() waits for the compute stream only: a running staged copy would write into freed memory).
struct Staged { DevBuf* buf; size_t bytes; };
int grow_staged(frp_handle* h, const std::vector<Staged>& bufs) {
    if (std::none_of(bufs.begin(), bufs.end(), [](const Staged& s) { return s.bytes > s.buf->cap || !s.buf->p; })) return FRP_OK;
    HIPCHK(h, hipStreamSynchronize(h->in.copy_stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (const Staged& s : bufs) FRPCHK(ensure(h, *s.buf, s.bytes));
    return FRP_OK;
}
// the staging frame buffer was the resident one until the last swap: the copy stream waits for the work enqueued before it
int begin_staging(frp_handle* h) {
    HIPCHK(h, hipStreamWaitEvent(h->in.copy_stream, h->in.ev_next_free, 0));
    return FRP_OK;
}
int end_staging(frp_handle* h, int B, int H, int W) {
    HIPCHK(h, hipEventRecord(h->in.ev_next_ready, h->in.copy_stream));
    h->in.nB = B; h->in.nH = H; h->in.nW = W;
    h->in.next_valid = true;
    return FRP_OK;
}

// the page-locked JPEG staging block of `turn`, at least `bytes` large: the copy of the batch before the previous one read it
int jpeg_staging_turn(frp_handle* h, int turn, size_t bytes, void** out) {
    Ingest& in = h->in;
    if (in.jpeg_h2d_pending[turn]) HIPCHK(h, hipEventSynchronize(in.ev_jpeg_h2d[turn]));
    in.jpeg_h2d_pending[turn] = false;
    if (bytes > in.jpeg_pin_cap[turn]) {
        if (in.jpeg_pin[turn]) { (void)hipHostFree(in.jpeg_pin[turn]); in.jpeg_pin[turn] = nullptr; in.jpeg_pin_cap[turn] = 0; }
        if (hipHostMalloc(&in.jpeg_pin[turn], bytes, hipHostMallocDefault) != hipSuccess) return fail(h, FRP_ERR_OOM, "hipHostMalloc (JPEG staging) failed");
        in.jpeg_pin_cap[turn] = bytes;
    }
    if (!in.ev_jpeg_h2d[turn]) HIPCHK(h, hipEventCreateWithFlags(&in.ev_jpeg_h2d[turn], hipEventDisableTiming));
    *out = in.jpeg_pin[turn];
    return FRP_OK;
}

const char* const kGeometryDiffers = "geometry differs from image 0 (one batch = one frame size and sampling)";
bool same_geometry(const frp_jpeg_info& a, const frp_jpeg_info& b) {
    return a.width == b.width && a.height == b.height && a.components == b.components && a.h_samp[0] == b.h_samp[0] && a.v_samp[0] == b.v_samp[0];
}

// Who entropy-decodes a JPEG batch.  The device routes move the COMPRESSED scans over PCIe (~0.5 MB per 1080p frame instead of 6.3 MB of
// coefficients) and leave the host its threads: Intervals - frames that all carry the same restart interval, one thread per interval
// (round 5; jpeg_kernels.hip: jpeg_huffman_kernel); Selfsync - frames without restart markers, where the handle asks for it (jpeg_selfsync.h,
// jpeg_selfsync.hip); Host - everything else, one image per task on host threads (jpeg_host.cpp: jpeg_decode_coefficients).
enum class JpegRoute { Host, Intervals, Selfsync };

long intervals_per_image(const frp_jpeg_info& I) { return ((long)I.mcus_x * I.mcus_y + I.restart_interval - 1) / I.restart_interval; }

// The device route that image 0's headers and the switches allow; plan_entropy_batch decides with the whole batch in hand.
JpegRoute candidate_route(const Ingest& in, const frp_jpeg_info& I, int B) {
    if (I.restart_interval <= 0) return in.jpeg_selfsync ? JpegRoute::Selfsync : JpegRoute::Host;
    // When: one thread per interval decodes 32 x 1080p frames in 17.8 ms at one interval per MCU row (120 MCUs), 4.5 ms at 30 MCUs,
    // 1.25 ms at 8 (profiles/r5/jpeg_device_entropy.txt) - the time goes with the LENGTH of an interval, and 16 host threads take
    // 9-12 ms: by default the device decodes streams whose intervals are at most 32 MCUs and the host the others.
    // FRP_JPEG_DEVICE_HUFFMAN=1 (read once): the device whatever the interval (takes the entropy decode off the host's cores; at
    // one interval per row it is slower than the pipeline consumes frames), =0: never.
    const int mode = process_switches().jpeg_device_huffman;
    if (mode < 0 || (mode == 0 && I.restart_interval > 32)) return JpegRoute::Host;
    const long n_int = intervals_per_image(I);
    if ((long)B * n_int < 64 || n_int > 0x7fffff) return JpegRoute::Host;          // too few intervals to fill a wave
    return JpegRoute::Intervals;
}

// Subsequence size of the self-synchronising decoder where the caller names none (frp_upload_jpeg_async; subseq_bytes 0 of
// frp_jpeg_selfsync_coefficients).  32 x 1080p, quality 90: batch resident after 6.84 ms at 64, 7.07 at 128, 6.86 at 256 - the repeats of
// one setting lie within 0.08 ms, so 64 and 256 tie and 128 is behind both (profiles/r6/jpeg_selfsync.txt).
constexpr int kJpegSelfsyncDefaultS = 64;

// A batch as a device route decodes it: every image's scan plan and tables, where the parts lie in the page-locked block and on the device
struct EntropyBatch {
    JpegRoute route = JpegRoute::Host;
    std::vector<JpegScanPlan> plans;
    std::vector<JpegHuffTableDev> tabs;
    JpegDeviceStageLayout SL;
    long off_words = 0;                 // words per image in SL's "offsets" part: the n_int + 1 interval offsets, or the four of img
    std::vector<uint32_t> img;          // Selfsync: [B][4] scan offset, scan bytes, subsequences, first subsequence
    int S = 0;                          // ... subsequence size; the largest image's subsequences; all images', each rounded up to JSS_WG
    uint32_t max_sub = 0;
    size_t n_sub_all = 0;
};

// Plans every image for the route `want` (the host does headers and one pass over the 0xFF bytes of every scan: jpeg_plan_scan) and lays
// the staging out.  -> an error ("JPEG i: ..."), or FRP_OK with eb.route = want, or = Host where this is not a batch of that route: a
// frame of the other kind or with another interval length, scans beyond the 32-bit offsets, more than 2^24 subsequences in all.
int plan_entropy_batch(frp_handle* h, const uint8_t* const* jpegs, const size_t* sizes, int32_t B, const frp_jpeg_info& I, JpegRoute want, int S,
                       EntropyBatch& eb) {
    eb.route = JpegRoute::Host;
    if (want == JpegRoute::Host) return FRP_OK;
    eb.plans.resize((size_t)B);
    eb.tabs.resize((size_t)B * 6);
    std::vector<size_t> scan_bytes((size_t)B);
    for (int i = 0; i < B; ++i) {
        std::string e;
        if (!jpegs[i]) return fail(h, FRP_ERR_INVALID, "JPEG " + std::to_string(i) + ": null image");
        const int rc = jpeg_plan_scan(jpegs[i], sizes[i], eb.plans[i], eb.tabs.data() + (size_t)i * 6, &e);
        const frp_jpeg_info& Ii = eb.plans[i].info;
        if ((Ii.restart_interval != 0) != (I.restart_interval != 0) && Ii.width > 0) return FRP_OK;       // a frame of the other kind
        if (rc != FRP_OK) return fail(h, rc, "JPEG " + std::to_string(i) + ": " + e);
        if (!same_geometry(Ii, I)) return fail(h, FRP_ERR_INVALID, "JPEG " + std::to_string(i) + ": " + kGeometryDiffers);
        if (Ii.restart_interval != I.restart_interval) return FRP_OK;
        scan_bytes[i] = eb.plans[i].scan_bytes;
    }
    eb.off_words = want == JpegRoute::Intervals ? intervals_per_image(I) + 1 : 4;
    eb.SL = jpeg_device_stage_layout(B, eb.off_words - 1, scan_bytes.data());
    if (eb.SL.too_large) return FRP_OK;
    if (want == JpegRoute::Selfsync) {
        eb.S = S;
        eb.img.resize((size_t)B * 4);
        uint64_t n_all = 0;
        for (int i = 0; i < B; ++i) {
            const uint32_t n_sub = jss_subsequences((uint32_t)scan_bytes[i], (uint32_t)S);
            eb.img[4 * i] = (uint32_t)eb.SL.soff[i]; eb.img[4 * i + 1] = (uint32_t)scan_bytes[i]; eb.img[4 * i + 2] = n_sub; eb.img[4 * i + 3] = (uint32_t)n_all;
            n_all += ((uint64_t)n_sub + JSS_WG - 1) / JSS_WG * JSS_WG;
            eb.max_sub = std::max(eb.max_sub, n_sub);
            if (n_all > (1u << 24)) return FRP_OK;
        }
        eb.n_sub_all = (size_t)n_all;
    }
    eb.route = want;
    return FRP_OK;
}

// The staging sequence of a device route, up to its kernels: the page-locked block of `turn` filled (scans | offsets | Huffman tables |
// quantisation tables; `back_bytes` behind them are the route's to read results into) -> *pin; the device buffers grown (ss_bytes: the
// self-synchronising decoder's scratch); one copy to the device, the coefficients zeroed, the quantisation tables copied behind them
// (L.q_off), `err_bytes` of flags zeroed.  for_frames: the batch is being staged (frp_upload_jpeg_async) - the frame and plane buffers are
// grown with the others and the copy stream waits for the staging frame buffer.
int stage_entropy_batch(frp_handle* h, const EntropyBatch& eb, int B, const frp_jpeg_info& I, const JpegBatchLayout& L, int turn, size_t back_bytes,
                        size_t err_bytes, size_t ss_bytes, bool for_frames, char** pin) {
    Ingest& in = h->in;
    const JpegDeviceStageLayout& SL = eb.SL;
    void* block = nullptr;
    FRPCHK(jpeg_staging_turn(h, turn, SL.o_err + back_bytes, &block));
    char* st = (char*)block;
    uint32_t* off = (uint32_t*)(st + SL.o_int);
    for (int i = 0; i < B; ++i) {
        const JpegScanPlan& P = eb.plans[i];
        memcpy(st + SL.soff[i], P.scan, P.scan_bytes);
        for (size_t k = 0; k < P.int_off.size(); ++k) off[(size_t)i * eb.off_words + k] = (uint32_t)(SL.soff[i] + P.int_off[k]);
        memcpy(st + SL.o_q + (size_t)i * 384, P.qtab, 384);
    }
    if (!eb.img.empty()) memcpy(off, eb.img.data(), eb.img.size() * 4);
    memcpy(st + SL.o_tab, eb.tabs.data(), eb.tabs.size() * sizeof(JpegHuffTableDev));
    std::vector<Staged> bufs = {{&in.jpeg_coef, L.total}, {&in.jpeg_scan, SL.o_err}, {&in.jpeg_err, err_bytes}};
    if (for_frames) { bufs.push_back({&in.frames_next, (size_t)B * I.height * I.width * 3}); bufs.push_back({&in.jpeg_planes, (size_t)B * L.plane_img}); }
    if (ss_bytes) bufs.push_back({&in.jpeg_ss, ss_bytes});
    FRPCHK(grow_staged(h, bufs));
    if (for_frames) FRPCHK(begin_staging(h));
    HIPCHK(h, hipMemcpyAsync(in.jpeg_scan.p, st, SL.o_err, hipMemcpyHostToDevice, in.copy_stream));
    HIPCHK(h, hipMemsetAsync(in.jpeg_coef.p, 0, L.q_off, in.copy_stream));
    HIPCHK(h, hipMemcpyAsync((char*)in.jpeg_coef.p + L.q_off, (char*)in.jpeg_scan.p + SL.o_q, (size_t)B * 384, hipMemcpyDeviceToDevice, in.copy_stream));
    HIPCHK(h, hipMemsetAsync(in.jpeg_err.p, 0, err_bytes, in.copy_stream));
    *pin = st;
    return FRP_OK;
}

// After the route's kernels: in.jpeg_err -> `back` (page-locked; `stride` words per image, word `flag` non-zero = a corrupt stream), and the
// host waits for it: this call reports it, as on the host path, before the pixel kernels are queued (the staging block is free again too).
int read_entropy_flags(frp_handle* h, int B, int32_t* back, int stride, int flag) {
    HIPCHK(h, hipMemcpyAsync(back, h->in.jpeg_err.p, (size_t)B * stride * 4, hipMemcpyDeviceToHost, h->in.copy_stream));
    HIPCHK(h, hipStreamSynchronize(h->in.copy_stream));
    for (int i = 0; i < B; ++i)
        if (back[stride * i + flag]) return fail(h, FRP_ERR_INVALID, "JPEG " + std::to_string(i) + ": corrupt or truncated entropy-coded data");
    return FRP_OK;
}

// Route Intervals.  On FRP_OK in.jpeg_coef holds the batch as the host decoder would have staged it (coefficients, tables at L.q_off).
int decode_intervals(frp_handle* h, const EntropyBatch& eb, int B, const frp_jpeg_info& I, const JpegBatchLayout& L, int turn) {
    Ingest& in = h->in;
    char* st = nullptr;
    FRPCHK(stage_entropy_batch(h, eb, B, I, L, turn, (size_t)B * 4, (size_t)B * 4, 0, true, &st));
    JpegHuffParams hp{};
    hp.scan = (const uint8_t*)in.jpeg_scan.p;
    hp.int_off = (const uint32_t*)((const char*)in.jpeg_scan.p + eb.SL.o_int);
    hp.tables = (const JpegHuffTableDev*)((const char*)in.jpeg_scan.p + eb.SL.o_tab);
    hp.coef = (int16_t*)in.jpeg_coef.p;
    hp.err = (int32_t*)in.jpeg_err.p;
    hp.coef_per_image = (long)L.coef_elems;
    hp.B = B; hp.n_int = (int)eb.off_words - 1; hp.ri = I.restart_interval;
    hp.mcus_y = I.mcus_y;
    hp.g = jss_geom(I, L);
    const hipError_t e = launch_jpeg_huffman(hp, in.copy_stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("jpeg huffman: ") + hipGetErrorString(e));
    return read_entropy_flags(h, B, (int32_t*)(st + eb.SL.o_err), 1, 0);
}

// Route Selfsync: every subsequence of S bytes is decoded speculatively and the synchronisation kernel is launched again while a launch
// reports a change - launch k leaves workgroups 0 .. k of every image final, so the loop ends within the largest image's workgroups -; then
// blocks are counted, coefficients written and the DC differences summed.  On FRP_OK in.jpeg_coef holds the batch as above.
// stats: [B][4] or null (frp.h: frp_jpeg_selfsync_coefficients).
int decode_selfsync(frp_handle* h, const EntropyBatch& eb, int B, const frp_jpeg_info& I, const JpegBatchLayout& L, int turn, bool for_frames,
                    int32_t* stats) {
    Ingest& in = h->in;
    // device scratch: entry | exit | wgx (8 bytes each), then cnt | base | rounds (4 bytes each)
    const size_t N = eb.n_sub_all, n_wg_all = N / JSS_WG;
    const size_t o_exit = N * 8, o_wgx = o_exit + N * 8, o_cnt = o_wgx + 2 * n_wg_all * 8, o_base = o_cnt + N * 4, o_rounds = o_base + N * 4;
    const size_t pin_stats = eb.SL.o_err, pin_rounds = pin_stats + (size_t)B * 16;      // read back: [B][4] stats, [B] rounds of a launch
    char* st = nullptr;
    FRPCHK(stage_entropy_batch(h, eb, B, I, L, turn, (size_t)B * 20, (size_t)B * 16, o_rounds + (size_t)B * 4, for_frames, &st));
    JpegSelfsyncParams sp{};
    char* ss = (char*)in.jpeg_ss.p;
    sp.scan = (const uint8_t*)in.jpeg_scan.p;
    sp.img = (const uint32_t*)((const char*)in.jpeg_scan.p + eb.SL.o_int);
    sp.tables = (const JpegHuffTableDev*)((const char*)in.jpeg_scan.p + eb.SL.o_tab);
    sp.entry = (JssState*)ss; sp.exit_ = (JssState*)(ss + o_exit); sp.wgx = (JssState*)(ss + o_wgx);
    sp.cnt = (uint32_t*)(ss + o_cnt); sp.base = (uint32_t*)(ss + o_base); sp.rounds = (int32_t*)(ss + o_rounds);
    sp.stats = (int32_t*)in.jpeg_err.p;
    sp.coef = (int16_t*)in.jpeg_coef.p;
    sp.coef_per_image = (long)L.coef_elems;
    sp.B = B; sp.S = eb.S; sp.max_sub = eb.max_sub; sp.n_wg_all = (uint32_t)n_wg_all;
    sp.g = jss_geom(I, L);
    if (sp.g.bpm > 6 || (long)I.mcus_x * I.mcus_y * sp.g.bpm != (long)L.blocks_per_image) return fail(h, FRP_ERR_INVALID, "JPEG 0: unsupported sampling factors");
    const int32_t* lr = (const int32_t*)(st + pin_rounds);
    std::vector<int32_t> rounds((size_t)B, 0);
    const uint32_t max_wg = (eb.max_sub + JSS_WG - 1) / JSS_WG;
    for (uint32_t k = 0;; ++k) {
        if (k > max_wg) return fail(h, FRP_ERR_HIP, "jpeg selfsync: no fix-point within the workgroups of the largest scan");       // (launch k leaves 0 .. k final)
        HIPCHK(h, hipMemsetAsync(sp.rounds, 0, (size_t)B * 4, in.copy_stream));
        const hipError_t e = launch_jpeg_selfsync_round(sp, (int)k, in.copy_stream);
        if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("jpeg selfsync: ") + hipGetErrorString(e));
        HIPCHK(h, hipMemcpyAsync(st + pin_rounds, sp.rounds, (size_t)B * 4, hipMemcpyDeviceToHost, in.copy_stream));
        HIPCHK(h, hipStreamSynchronize(in.copy_stream));
        bool changed = false;
        for (int i = 0; i < B; ++i) { rounds[i] += lr[i]; changed = changed || lr[i] != 0; }
        if (k == 0 ? max_wg == 1 : !changed) break;            // (one workgroup per image: launch 0 ran to the fix-point)
    }
    const hipError_t e = launch_jpeg_selfsync_finish(sp, in.copy_stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("jpeg selfsync: ") + hipGetErrorString(e));
    int32_t* got = (int32_t*)(st + pin_stats);
    const int rc = read_entropy_flags(h, B, got, 4, 3);
    if (stats && rc != FRP_ERR_HIP)                             // (the statistics of a refused batch too)
        for (int i = 0; i < B; ++i) { stats[4 * i] = got[4 * i]; stats[4 * i + 1] = rounds[i]; stats[4 * i + 2] = got[4 * i + 2]; stats[4 * i + 3] = got[4 * i + 3]; }
    return rc;
}

// Route Host: one image per task on host threads (the images are independent; within one the bit stream is serial) into the page-locked
// block of `turn`, which then goes to the device as it is - coefficients, quantisation tables at L.q_off.
int decode_on_host(frp_handle* h, const uint8_t* const* jpegs, const size_t* sizes, int B, const frp_jpeg_info& I, const JpegBatchLayout& L, int turn) {
    Ingest& in = h->in;
    void* pin = nullptr;
    FRPCHK(jpeg_staging_turn(h, turn, L.total, &pin));
    int16_t* coef = (int16_t*)pin;
    uint16_t* qtab = (uint16_t*)((char*)pin + L.q_off);
    std::vector<int> rcs((size_t)B, FRP_OK);
    std::vector<std::string> errs((size_t)B);
    {
        const int nth = std::max(1, std::min<int>(B, (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()))));
        std::atomic<int> next{0};
        auto work = [&]() {
            for (int i = next.fetch_add(1); i < B; i = next.fetch_add(1)) {
                frp_jpeg_info Ii{};
                if (!jpegs[i]) { rcs[i] = FRP_ERR_INVALID; errs[i] = "null image"; continue; }
                rcs[i] = jpeg_decode_coefficients(jpegs[i], sizes[i], coef + (size_t)i * L.coef_elems, L.coef_elems, qtab + (size_t)i * 192, &Ii, &errs[i]);
                if (rcs[i] == FRP_OK && !same_geometry(Ii, I)) { rcs[i] = FRP_ERR_INVALID; errs[i] = kGeometryDiffers; }
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < nth; ++t) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
    }
    for (int i = 0; i < B; ++i)
        if (rcs[i] != FRP_OK) return fail(h, rcs[i], "JPEG " + std::to_string(i) + ": " + errs[i]);
    FRPCHK(grow_staged(h, {{&in.frames_next, (size_t)B * I.height * I.width * 3}, {&in.jpeg_coef, L.total}, {&in.jpeg_planes, (size_t)B * L.plane_img}}));
    FRPCHK(begin_staging(h));
    HIPCHK(h, hipMemcpyAsync(in.jpeg_coef.p, pin, L.total, hipMemcpyHostToDevice, in.copy_stream));
    HIPCHK(h, hipEventRecord(in.ev_jpeg_h2d[turn], in.copy_stream));
    in.jpeg_h2d_pending[turn] = true;
    return FRP_OK;
}

// ---- YUV 4:2:0 surfaces (frp.h: frp_upload_yuv; the kernels and the arithmetic: yuv_kernels.hip) ----
constexpr int kYuvMaxBatch = 1024;
constexpr size_t kYuvTabBytes = (size_t)kYuvMaxBatch * 3 * sizeof(void*);       // one turn of the plane table
// yoff, cy, cvr, cvg, cug, cub, rnd, sh per FRP_YUV_BT601 / _BT709 / _JFIF (frp.h has the formulas)
const YuvCoef kYuvCoef[3] = {{16, 1220542, 1673527, 852492, 409993, 2116026, 1 << 19, 20},
                             {16, 1220542, 1880097, 558891, 223347, 2214593, 1 << 19, 20},
                             {0, 65536, 91881, 46802, 22554, 116130, 32768, 16}};
bool yuv_semi_planar(int layout) { return layout == FRP_YUV_NV12 || layout == FRP_YUV_NV21; }

int check_yuv(frp_handle* h, const frp_yuv_desc* d, const uint8_t* const* planes, int B) {
    if (!d) return fail(h, FRP_ERR_INVALID, "yuv: desc is null");
    if (!planes) return fail(h, FRP_ERR_INVALID, "yuv: planes is null");
    if (d->struct_size != (int32_t)sizeof(frp_yuv_desc)) return fail(h, FRP_ERR_INVALID, "yuv: struct_size is not sizeof(frp_yuv_desc)");
    if (d->layout < FRP_YUV_NV12 || d->layout > FRP_YUV_YV12) return fail(h, FRP_ERR_INVALID, "yuv: unknown layout");
    if (d->matrix < FRP_YUV_BT601 || d->matrix > FRP_YUV_JFIF) return fail(h, FRP_ERR_INVALID, "yuv: unknown matrix");
    if (d->flags & ~FRP_YUV_DEVICE) return fail(h, FRP_ERR_INVALID, "yuv: unknown bits in flags");
    if (d->width <= 0 || d->width % 2) return fail(h, FRP_ERR_INVALID, "yuv: width must be positive and even");
    if (d->height <= 0 || d->height % 2) return fail(h, FRP_ERR_INVALID, "yuv: height must be positive and even");
    if ((int64_t)d->width * d->height > (1ll << 30)) return fail(h, FRP_ERR_INVALID, "yuv: width * height beyond 2^30 pixels");
    if (d->y_pitch < d->width) return fail(h, FRP_ERR_INVALID, "yuv: y_pitch is smaller than width");
    const bool semi = yuv_semi_planar(d->layout);
    if (d->c_pitch < (semi ? d->width : d->width / 2)) return fail(h, FRP_ERR_INVALID, semi ? "yuv: c_pitch is smaller than width" : "yuv: c_pitch is smaller than width / 2");
    if (B < 1 || B > kYuvMaxBatch) return fail(h, FRP_ERR_INVALID, "yuv: B must be 1 .. 1024");
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < (semi ? 2 : 3); ++k)
            if (!planes[3 * b + k]) return fail(h, FRP_ERR_INVALID, "yuv: planes[" + std::to_string(b) + "][" + std::to_string(k) + "] is null");
    return FRP_OK;
}

// the buffers a YUV batch needs besides its frame buffer (`more`: that one, when it is the staging buffer), and the page-locked table
int prepare_yuv(frp_handle* h, const frp_yuv_desc& d, int B, std::vector<Staged> more) {
    Ingest& in = h->in;
    if (!(d.flags & FRP_YUV_DEVICE)) more.push_back({&in.yuv_stage, (size_t)B * d.width * d.height * 3 / 2});
    more.push_back({&in.yuv_tab, 2 * kYuvTabBytes});
    FRPCHK(grow_staged(h, more));
    if (!in.yuv_pin && hipHostMalloc(&in.yuv_pin, 2 * kYuvTabBytes, hipHostMallocDefault) != hipSuccess) {
        in.yuv_pin = nullptr;
        return fail(h, FRP_ERR_OOM, "hipHostMalloc (YUV plane table) failed");
    }
    return FRP_OK;
}

// Queues the work of one batch on `s` (yuv_to_frames below owns the turn and its event): host planes into in.yuv_stage (neighbouring copies
// that continue each other in the source and in the packed destination go as one - a pool of pitched NV12 surfaces is a single 2-D copy,
// packed frames back to back a single linear one), the plane table of `turn`, the kernel into `dst` [B, H, W, 3].
int queue_yuv_turn(frp_handle* h, const frp_yuv_desc& d, const uint8_t* const* planes, int B, void* dst, hipStream_t s, int turn) {
    Ingest& in = h->in;
    const bool semi = yuv_semi_planar(d.layout), device = (d.flags & FRP_YUV_DEVICE) != 0;
    const size_t W = (size_t)d.width, H = (size_t)d.height, y_bytes = W * H, c_bytes = semi ? y_bytes / 2 : y_bytes / 4;
    const uint8_t** tab = (const uint8_t**)((char*)in.yuv_pin + (size_t)turn * kYuvTabBytes);
    int64_t y_pitch = d.y_pitch, c_pitch = d.c_pitch;
    if (device) {
        for (int i = 0; i < 3 * B; ++i) tab[i] = i % 3 == 2 && semi ? nullptr : planes[i];
    } else {
        if (in.yuv_pending[turn ^ 1]) HIPCHK(h, hipStreamWaitEvent(s, in.ev_yuv[turn ^ 1], 0));       // the previous batch's kernel may still read the stage
        struct Copy { size_t dst; const uint8_t* src; size_t width, rows, pitch; };
        std::vector<Copy> jobs;
        auto add = [&jobs](size_t at, const uint8_t* src, size_t width, size_t rows, size_t pitch) {
            if (pitch == width || rows == 1) { width *= rows; rows = 1; pitch = width; }           // dense: one run of bytes
            if (!jobs.empty()) {
                Copy& j = jobs.back();
                const bool follows = j.dst + j.width * j.rows == at;
                if (follows && j.rows == 1 && rows == 1 && j.src + j.width == src) { j.width += width; j.pitch = j.width; return; }
                if (follows && j.rows > 1 && rows > 1 && j.width == width && j.pitch == pitch && j.src + j.rows * j.pitch == src) { j.rows += rows; return; }
            }
            jobs.push_back({at, src, width, rows, pitch});
        };
        uint8_t* stage = (uint8_t*)in.yuv_stage.p;
        const size_t frame_bytes = y_bytes * 3 / 2, c_w = semi ? W : W / 2;
        for (int b = 0; b < B; ++b) {
            const size_t at = (size_t)b * frame_bytes;
            add(at, planes[3 * b], W, H, (size_t)d.y_pitch);
            add(at + y_bytes, planes[3 * b + 1], c_w, H / 2, (size_t)d.c_pitch);
            if (!semi) add(at + y_bytes + c_bytes, planes[3 * b + 2], c_w, H / 2, (size_t)d.c_pitch);
            tab[3 * b] = stage + at;
            tab[3 * b + 1] = stage + at + y_bytes;
            tab[3 * b + 2] = semi ? nullptr : stage + at + y_bytes + c_bytes;
        }
        for (const Copy& j : jobs) {
            if (j.rows == 1) HIPCHK(h, hipMemcpyAsync(stage + j.dst, j.src, j.width, hipMemcpyHostToDevice, s));
            else HIPCHK(h, hipMemcpy2DAsync(stage + j.dst, j.width, j.src, j.pitch, j.width, j.rows, hipMemcpyHostToDevice, s));
        }
        y_pitch = (int64_t)W;
        c_pitch = (int64_t)c_w;
    }
    if (d.layout == FRP_YUV_YV12)
        for (int b = 0; b < B; ++b) std::swap(tab[3 * b + 1], tab[3 * b + 2]);          // the kernel's order is Y, U, V
    // the fast path's conditions (yuv_kernels.hip); one frame that misses them sends the whole batch down the general path
    const uintptr_t c_align = semi ? 15 : 7;
    bool fast = W % 16 == 0 && y_pitch % 16 == 0 && (c_pitch & (int64_t)c_align) == 0;
    for (int b = 0; b < B && fast; ++b)
        fast = ((uintptr_t)tab[3 * b] & 15) == 0 && ((uintptr_t)tab[3 * b + 1] & c_align) == 0 && ((uintptr_t)tab[3 * b + 2] & c_align) == 0;
    char* dev_tab = (char*)in.yuv_tab.p + (size_t)turn * kYuvTabBytes;
    HIPCHK(h, hipMemcpyAsync(dev_tab, tab, (size_t)B * 3 * sizeof(void*), hipMemcpyHostToDevice, s));
    YuvParams p{};
    p.tab = (const uint8_t* const*)dev_tab;
    p.frames = (uint8_t*)dst;
    p.B = B; p.W = d.width; p.H = d.height;
    p.y_pitch = y_pitch; p.c_pitch = c_pitch;
    p.ush = d.layout == FRP_YUV_NV21 ? 8 : 0;
    p.k = kYuvCoef[d.matrix];
    const hipError_t e = launch_yuv_to_bgr(p, semi, fast, s);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("yuv to bgr: ") + hipGetErrorString(e));
    return FRP_OK;
}

// One batch on `s` through the next turn of the plane table.  The turn's event is recorded behind whatever queue_yuv_turn queued, also when
// it returns an error half way (copies out of the page-locked table may be in flight then): the next use of the turn waits for them.
int yuv_to_frames(frp_handle* h, const frp_yuv_desc& d, const uint8_t* const* planes, int B, void* dst, hipStream_t s) {
    Ingest& in = h->in;
    const int turn = in.yuv_turn;
    if (in.yuv_pending[turn]) HIPCHK(h, hipEventSynchronize(in.ev_yuv[turn]));         // the table of two batches ago: copied and read
    in.yuv_pending[turn] = false;
    if (!in.ev_yuv[turn]) HIPCHK(h, hipEventCreateWithFlags(&in.ev_yuv[turn], hipEventDisableTiming));
    in.yuv_turn ^= 1;
    const int rc = queue_yuv_turn(h, d, planes, B, dst, s, turn);
    const hipError_t e = hipEventRecord(in.ev_yuv[turn], s);
    in.yuv_pending[turn] = e == hipSuccess;
    if (rc == FRP_OK && e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("hipEventRecord (YUV turn): ") + hipGetErrorString(e));
    return rc;
}

}  // namespace

int frp::upload_frames(frp_handle* h, const uint8_t* bgr, int B, int H, int W, int64_t row_stride) {
    FRPCHK(check_frames(h, bgr, B, H, W, row_stride));
    FRPCHK(ensure(h, h->frames, (size_t)B * H * W * 3));
    rec(h, EV_START);
    HIPCHK(h, hipMemcpy2DAsync(h->frames.p, (size_t)W * 3, bgr, (size_t)row_stride, (size_t)W * 3, (size_t)B * H,
                               hipMemcpyHostToDevice, h->stream));
    rec(h, EV_H2D);
    set_resident(h, B, H, W);
    return FRP_OK;
}

extern "C" {

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
    h->in.pinned.push_back(p);
    return p;
}

void frp_host_free(frp_handle* h, void* p) {
    if (!h || !p) return;
    Guard g(h);
    for (size_t i = 0; i < h->in.pinned.size(); ++i)
        if (h->in.pinned[i] == p) {
            (void)hipStreamSynchronize(h->in.copy_stream);
            (void)hipHostFree(p);
            h->in.pinned.erase(h->in.pinned.begin() + (long)i);
            return;
        }
}

int frp_upload_frames_async(frp_handle* h, const uint8_t* bgr, int32_t B, int32_t H, int32_t W, int64_t row_stride) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);      // copy stream only: does not re-record the stage events, so a pending pass is not drained
                            // (with the timers on, settling here made the upload of batch t+1 wait for batch t)
    FRPCHK(check_frames(h, bgr, B, H, W, row_stride));
    FRPCHK(grow_staged(h, {{&h->in.frames_next, (size_t)B * H * W * 3}}));
    FRPCHK(begin_staging(h));
    HIPCHK(h, hipMemcpy2DAsync(h->in.frames_next.p, (size_t)W * 3, bgr, (size_t)row_stride, (size_t)W * 3, (size_t)B * H,
                               hipMemcpyHostToDevice, h->in.copy_stream));
    return end_staging(h, B, H, W);
}

int frp_jpeg_info_get(const uint8_t* data, size_t size, frp_jpeg_info* info) {
    if (!data || !info) return FRP_ERR_INVALID;
    return jpeg_info(data, size, info, nullptr);
}

int frp_jpeg_coefficients(const uint8_t* data, size_t size, int16_t* coef, size_t coef_elems, uint16_t* qtab, frp_jpeg_info* info) {
    if (!data || !coef || !qtab) return FRP_ERR_INVALID;
    return jpeg_decode_coefficients(data, size, coef, coef_elems, qtab, info, nullptr);
}

int frp_upload_jpeg_async(frp_handle* h, const uint8_t* const* jpegs, const size_t* sizes, int32_t B) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);      // copy stream only (as frp_upload_frames_async)
    if (!jpegs || !sizes || B <= 0 || B > 1024) return fail(h, FRP_ERR_INVALID, "bad JPEG batch arguments");
    frp_jpeg_info I{};
    std::string err;
    if (!jpegs[0] || jpeg_info(jpegs[0], sizes[0], &I, &err) != FRP_OK) return fail(h, FRP_ERR_INVALID, "JPEG 0: " + err);
    const JpegBatchLayout L = jpeg_batch_layout(I, B);
    Ingest& in = h->in;
    const int turn = in.jpeg_turn;      // flips once per call, whichever decoder takes the batch and whether it succeeds
    in.jpeg_turn ^= 1;
    EntropyBatch eb;
    FRPCHK(plan_entropy_batch(h, jpegs, sizes, B, I, candidate_route(in, I, B), in.jpeg_selfsync_bytes ? in.jpeg_selfsync_bytes : kJpegSelfsyncDefaultS, eb));
    switch (eb.route) {                 // entropy decode: in.jpeg_coef <- coefficients and quantisation tables, on the copy stream
        case JpegRoute::Intervals: FRPCHK(decode_intervals(h, eb, B, I, L, turn)); break;
        case JpegRoute::Selfsync: FRPCHK(decode_selfsync(h, eb, B, I, L, turn, true, nullptr)); break;
        case JpegRoute::Host: FRPCHK(decode_on_host(h, jpegs, sizes, B, I, L, turn)); break;
    }
    // the pixel kernels (dequantise, inverse DCT, upsample, YCbCr -> BGR) from the device coefficients into the staging frame buffer
    JpegParams p{};
    p.coef = (const int16_t*)in.jpeg_coef.p;
    p.qtab = (const uint16_t*)((const char*)in.jpeg_coef.p + L.q_off);
    p.planes = (uint8_t*)in.jpeg_planes.p;
    p.frames = (uint8_t*)in.frames_next.p;
    p.B = B; p.W = I.width; p.H = I.height; p.components = I.components;
    p.hs = I.h_samp[0]; p.vs = I.v_samp[0];
    p.cw = L.cw; p.ch = L.ch; p.blocks_per_image = L.blocks_per_image; p.plane_img = L.plane_img;
    for (int c = 0; c < 3; ++c) { p.bx[c] = L.bx[c]; p.by[c] = L.by[c]; p.plane_off[c] = L.plane_off[c]; }
    const hipError_t e = launch_jpeg_decode(p, in.copy_stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("jpeg decode: ") + hipGetErrorString(e));
    FRPCHK(end_staging(h, B, I.height, I.width));
    if (eb.route == JpegRoute::Intervals) in.ctr_jpeg_device_batches += 1;
    if (eb.route == JpegRoute::Selfsync) in.ctr_jpeg_selfsync_batches += 1;
    return FRP_OK;
}

// diagnostic: how many frp_upload_jpeg_async batches had their entropy decode on the device (restart-interval streams)
int64_t frp_debug_jpeg_device_batches(frp_handle* h) {
    if (!h) return -1;
    Guard g(h, false);
    return h->in.ctr_jpeg_device_batches;
}

int frp_set_jpeg_selfsync(frp_handle* h, int32_t on) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    if (on < 0 || (on > 1 && (on < 16 || on > 1024 || on % 16 != 0))) return fail(h, FRP_ERR_INVALID, "frp_set_jpeg_selfsync: 0, 1 or a subsequence size (a multiple of 16 in 16 .. 1024)");
    h->in.jpeg_selfsync = on != 0;
    h->in.jpeg_selfsync_bytes = on > 1 ? on : 0;
    return FRP_OK;
}

int64_t frp_debug_jpeg_selfsync_batches(frp_handle* h) {
    if (!h) return -1;
    Guard g(h, false);
    return h->in.ctr_jpeg_selfsync_batches;
}

int frp_jpeg_selfsync_coefficients(frp_handle* h, const uint8_t* const* jpegs, const size_t* sizes, int32_t B, int32_t subseq_bytes, int16_t* coef,
                                   int64_t coef_elems, int32_t* stats) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);      // copy stream only (as frp_upload_jpeg_async)
    if (!jpegs || !sizes || !coef || B <= 0 || B > 1024) return fail(h, FRP_ERR_INVALID, "bad JPEG batch arguments");
    if (subseq_bytes != 0 && (subseq_bytes < 16 || subseq_bytes > 1024 || subseq_bytes % 16 != 0))
        return fail(h, FRP_ERR_INVALID, "subseq_bytes must be 0 or a multiple of 16 in 16 .. 1024");
    frp_jpeg_info I{};
    std::string err;
    if (!jpegs[0] || jpeg_info(jpegs[0], sizes[0], &I, &err) != FRP_OK) return fail(h, FRP_ERR_INVALID, "JPEG 0: " + err);
    const JpegBatchLayout L = jpeg_batch_layout(I, B);
    if (coef_elems < 0 || (uint64_t)coef_elems < (uint64_t)B * L.coef_elems) return fail(h, FRP_ERR_INVALID, "coefficient buffer too small");
    Ingest& in = h->in;
    const int turn = in.jpeg_turn;      // a staging block of its own turn, as every JPEG batch
    in.jpeg_turn ^= 1;
    EntropyBatch eb;
    FRPCHK(plan_entropy_batch(h, jpegs, sizes, B, I, I.restart_interval == 0 ? JpegRoute::Selfsync : JpegRoute::Host,
                              subseq_bytes ? subseq_bytes : kJpegSelfsyncDefaultS, eb));
    if (eb.route != JpegRoute::Selfsync) return fail(h, FRP_ERR_INVALID, "not a batch of the self-synchronising decoder (a frame carries restart intervals, or the scans are too large)");
    FRPCHK(decode_selfsync(h, eb, B, I, L, turn, false, stats));
    HIPCHK(h, hipMemcpyAsync(coef, in.jpeg_coef.p, L.coef_bytes, hipMemcpyDeviceToHost, in.copy_stream));
    HIPCHK(h, hipStreamSynchronize(in.copy_stream));
    return FRP_OK;
}

int frp_upload_yuv(frp_handle* h, const frp_yuv_desc* desc, const uint8_t* const* planes, int32_t B) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    FRPCHK(check_yuv(h, desc, planes, B));
    FRPCHK(prepare_yuv(h, *desc, B, {}));
    FRPCHK(ensure(h, h->frames, (size_t)B * desc->height * desc->width * 3));
    rec(h, EV_START);
    FRPCHK(yuv_to_frames(h, *desc, planes, B, h->frames.p, h->stream));
    rec(h, EV_H2D);
    set_resident(h, B, desc->height, desc->width);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

int frp_upload_yuv_async(frp_handle* h, const frp_yuv_desc* desc, const uint8_t* const* planes, int32_t B) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);      // copy stream only (as frp_upload_frames_async)
    FRPCHK(check_yuv(h, desc, planes, B));
    FRPCHK(prepare_yuv(h, *desc, B, {{&h->in.frames_next, (size_t)B * desc->height * desc->width * 3}}));
    FRPCHK(begin_staging(h));
    FRPCHK(yuv_to_frames(h, *desc, planes, B, h->in.frames_next.p, h->in.copy_stream));
    return end_staging(h, B, desc->height, desc->width);
}

int frp_get_frames(frp_handle* h, uint8_t* out, int64_t out_bytes, int32_t first, int32_t n) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (h->rB <= 0 || !h->frames.p) return fail(h, FRP_ERR_INVALID, "no resident frames");
    if (first < 0 || n <= 0 || (int64_t)first + n > h->rB) return fail(h, FRP_ERR_INVALID, "get_frames: first / n outside the resident batch");
    const int64_t frame_bytes = (int64_t)h->rH * h->rW * 3;
    if (!out || out_bytes < n * frame_bytes) return fail(h, FRP_ERR_INVALID, "get_frames: out_bytes too small");
    HIPCHK(h, hipMemcpyAsync(out, (const char*)h->frames.p + first * frame_bytes, (size_t)(n * frame_bytes), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return FRP_OK;
}

int frp_swap_frames(frp_handle* h) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);      // enqueues a wait + an event on the compute stream; the stage events stay as recorded
    Ingest& in = h->in;
    if (!in.next_valid) return fail(h, FRP_ERR_INVALID, "no staged frames (call frp_upload_frames_async)");
    HIPCHK(h, hipStreamWaitEvent(h->stream, in.ev_next_ready, 0));     // compute waits for the staged copy
    std::swap(h->frames, in.frames_next);
    HIPCHK(h, hipEventRecord(in.ev_next_free, h->stream));            // ... and the old resident buffer is free after
    set_resident(h, in.nB, in.nH, in.nW);                              // everything enqueued so far
    in.next_valid = false;
    return FRP_OK;
}

}  // extern "C"
