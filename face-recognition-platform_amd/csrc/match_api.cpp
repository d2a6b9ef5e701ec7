// The matcher's host half: staging of the queries in q16, the launch parameters, the match of a pipeline pass (run_faces), the
// stand-alone match entry points (top-1, top-k, score matrix, radius match, the fp16 diagnostic) and the radius match's hit lists
// (frp_set_within, frp_fetch_within, the rebuild of lists that overflowed).  Kernels: match.hip; the handle's fields: Matcher.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "frp.h"
#include "frp_internal.h"
#include "frp_handle.h"

using namespace frp;

int frp::stage_queries(frp_handle* h, int n, const float* rows, const void* f16) {
    const size_t bytes = (size_t)round_up(n, 32) * FRP_EMB_DIM * 2;
    h->pass.q16_of_pass = false;
    FRPCHK(ensure(h, h->m.q16, bytes));
    HIPCHK(h, hipMemsetAsync(h->m.q16.p, 0, bytes, h->stream));
    if (rows) FRPCHK(upload_rows_normalized(h, rows, n, (_Float16*)h->m.q16.p));
    if (f16) HIPCHK(h, hipMemcpyAsync(h->m.q16.p, f16, (size_t)n * FRP_EMB_DIM * 2, hipMemcpyHostToDevice, h->stream));
    return FRP_OK;
}

namespace {

int hip_rc(frp_handle* h, hipError_t e, const char* what) {
    return e == hipSuccess ? FRP_OK : fail(h, FRP_ERR_HIP, std::string(what) + hipGetErrorString(e));
}

bool queries_ok(const void* q, int M) { return q && M > 0 && M <= (1 << 20); }

// the "within" epilogue of a match launch (frp_match_within, FRP_FLAG_WITHIN): bound, list size and the device lists [n], [n x cap]
struct WithinArgs {
    float min_cos;
    int cap;
    int32_t* cnt;
    int32_t* idx;
    float* cos;
};
static_assert(FRP_WITHIN_MAX_CAP == FRP_MAX_TOPK, "frp_internal.h: FRP_WITHIN_MAX_CAP");
bool within_args_ok(float min_cos, int cap) { return min_cos >= -2.0f && cap >= 1 && cap <= FRP_MAX_TOPK; }   // (NaN fails the first)

void* dev_ptr(const DevBuf& b) { return b.p; }
void* dev_ptr(const ScopedBuf& b) { return b->p; }

// The parameters of a match of the n queries at q (zero padded to a multiple of 32) against the gallery, with work buffers grown to
// fit: the handle's (Buf = DevBuf) or the scoped ones of the overflow rebuild (ScopedBuf).
template <class Buf>
int fill_match_params(frp_handle* h, const void* q, int n, Buf& part_cos, Buf& part_idx, Buf& best_cos, Buf& best_idx, MatchParams& mp) {
    mp = MatchParams{};
    mp.gallery = (const _Float16*)h->gallery.p;
    mp.N = h->g_rows;
    mp.q = (const _Float16*)q;
    mp.M = n;
    mp.Mpad = round_up(n, 32);
    mp.n_wg = match_num_workgroups(h->g_rows);
    FRPCHK(ensure(h, part_cos, (size_t)mp.n_wg * mp.Mpad * 4));
    FRPCHK(ensure(h, part_idx, (size_t)mp.n_wg * mp.Mpad * 4));
    FRPCHK(ensure(h, best_cos, (size_t)mp.Mpad * 4));
    FRPCHK(ensure(h, best_idx, (size_t)mp.Mpad * 4));
    mp.part_cos = (float*)dev_ptr(part_cos); mp.part_idx = (int32_t*)dev_ptr(part_idx);
    mp.best_cos = (float*)dev_ptr(best_cos); mp.best_idx = (int32_t*)dev_ptr(best_idx);
    return FRP_OK;
}

// the masks of a grouped launch: the row masks (brought to the device where they are not) and the n query masks in m.q_groups - copied
// there from the host (`q_groups`), or, without, whatever the caller launches next (match_pass: launch_face_groups)
int stage_groups(frp_handle* h, int n, const uint32_t* q_groups, MatchGroups& mg) {
    FRPCHK(ensure(h, h->m.q_groups, (size_t)round_up(n, 32) * 4));
    if (q_groups) HIPCHK(h, hipMemcpyAsync(h->m.q_groups.p, q_groups, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    mg.q_groups = (const uint32_t*)h->m.q_groups.p;
    return row_groups_device(h, &mg.row_groups);
}

int launch_counted(frp_handle* h, const MatchParams& mp, bool per_tile_only, const char* what, const MatchGroups* mg = nullptr) {
    FRPCHK(hip_rc(h, mg ? launch_match(mp, per_tile_only, h->stream, *mg) : launch_match(mp, per_tile_only, h->stream), what));
    h->ctr.match_bytes += (double)mp.N * (FRP_EMB_DIM * 2 + (mg ? 4 : 0));
    h->ctr.match_launches += 1;
    return FRP_OK;
}

// q16 [mpad,512] holds n unit queries -> best_idx/best_cos [n] (+ the hit lists of `within`, in the same launch)
// mg: the GROUPS form of the same launch (stage_groups)
int run_match(frp_handle* h, const Switches& sw, int n, float* all_scores_dev, const int32_t* n_dev = nullptr,
              const WithinArgs* within = nullptr, const MatchGroups* mg = nullptr) {
    if (n <= 0) return FRP_OK;
    if (h->g_rows <= 0) return fail(h, FRP_ERR_NO_GALLERY, "gallery is empty");
    Matcher& m = h->m;
    MatchParams mp;
    FRPCHK(fill_match_params(h, m.q16.p, n, m.part_cos, m.part_idx, m.best_cos, m.best_idx, mp));
    mp.all_scores = all_scores_dev;
    mp.n_dev = n_dev;
    if (within) {
        HIPCHK(h, hipMemsetAsync(within->cnt, 0, (size_t)n * 4, h->stream));      // counters start at zero before EVERY pass
        mp.min_cos = within->min_cos; mp.cap = within->cap;
        mp.hit_count = within->cnt; mp.hit_idx = within->idx; mp.hit_cos = within->cos;
    }
    return launch_counted(h, mp, sw.match_v1 != 0, "match: ", mg);
}

// Queries `over` (indices into q16 and into the lists) have more than `cap` rows at or above the bound: which of them took the
// slots was a race, so their lists are rebuilt as the first `cap` entries of the matcher's total order - the score rows of those
// queries alone (the per-tile kernel's all_scores epilogue: the same bits), then launch_topk_rows.  All of those entries are hits.
// q_groups (device, indexed like q16; null: an ungrouped match): the rebuild is grouped as well - the score rows hold a NaN where a
// row is not permitted, which launch_topk_rows never selects.
int rebuild_within_lists(frp_handle* h, const std::vector<int>& over, int cap, int32_t* hit_idx, float* hit_cos,
                         const uint32_t* q_groups = nullptr) {
    const _Float16* q16 = (const _Float16*)h->m.q16.p;
    const long N = h->g_rows;
    const int total = (int)over.size();
    const int chunk = (int)std::max<long>(1, std::min<long>(total, (1L << 28) / N));      // <= 1 GiB of scores at a time
    const size_t qbytes = (size_t)round_up(chunk, 32) * FRP_EMB_DIM * 2;
    ScopedBuf qt, all, pc, pi, bc, bi, tidx, tcos, qg;
    MatchGroups mg{nullptr, nullptr};
    if (q_groups) {
        FRPCHK(ensure(h, qg, (size_t)round_up(chunk, 32) * 4));
        FRPCHK(row_groups_device(h, &mg.row_groups));
        mg.q_groups = (const uint32_t*)qg->p;
    }
    FRPCHK(ensure(h, qt, qbytes));
    FRPCHK(ensure(h, all, (size_t)chunk * N * 4));
    FRPCHK(ensure(h, tidx, (size_t)chunk * cap * 4));
    FRPCHK(ensure(h, tcos, (size_t)chunk * cap * 4));
    for (int m0 = 0; m0 < total; m0 += chunk) {
        const int m = std::min(chunk, total - m0);
        HIPCHK(h, hipMemsetAsync(qt->p, 0, qbytes, h->stream));
        for (int i = 0; i < m; ++i)
            HIPCHK(h, hipMemcpyAsync((_Float16*)qt->p + (size_t)i * FRP_EMB_DIM, q16 + (size_t)over[m0 + i] * FRP_EMB_DIM, FRP_EMB_DIM * 2,
                                     hipMemcpyDeviceToDevice, h->stream));
        for (int i = 0; q_groups && i < m; ++i)
            HIPCHK(h, hipMemcpyAsync((uint32_t*)qg->p + i, q_groups + over[m0 + i], 4, hipMemcpyDeviceToDevice, h->stream));
        MatchParams mp;
        FRPCHK(fill_match_params(h, qt->p, m, pc, pi, bc, bi, mp));       // (the first chunk is the largest: it sizes the buffers)
        mp.all_scores = (float*)all->p;
        FRPCHK(launch_counted(h, mp, true, "match within (overflow): ", q_groups ? &mg : nullptr));
        FRPCHK(hip_rc(h, launch_topk_rows((const float*)all->p, m, N, cap, (int32_t*)tidx->p, (float*)tcos->p, h->stream),
                      "match within (overflow): "));
        for (int i = 0; i < m; ++i) {
            const size_t dst = (size_t)over[m0 + i] * cap, src = (size_t)i * cap;
            HIPCHK(h, hipMemcpyAsync(hit_idx + dst, (int32_t*)tidx->p + src, (size_t)cap * 4, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(hit_cos + dst, (float*)tcos->p + src, (size_t)cap * 4, hipMemcpyDeviceToDevice, h->stream));
        }
    }
    return FRP_OK;          // stream-ordered: the caller waits for the stream before the scoped buffers go
}

// Behind a stand-alone run_match (its rc): top-1 of the M queries and, where asked for, the score matrix to the host.  Waits for the
// stream on every path: the caller's scoped buffers go next.
int match_out(frp_handle* h, int rc, int M, int32_t* idx, float* cos, float* scores, const void* scores_dev, const char* what) {
    hipError_t e = hipSuccess;
    if (rc == FRP_OK) {
        if (idx) e = hipMemcpyAsync(idx, h->m.best_idx.p, (size_t)M * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && cos) e = hipMemcpyAsync(cos, h->m.best_cos.p, (size_t)M * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && scores) e = hipMemcpyAsync(scores, scores_dev, (size_t)M * h->g_rows * 4, hipMemcpyDeviceToHost, h->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(h->stream);
    if (rc != FRP_OK) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return fail(h, FRP_ERR_HIP, what);
    return FRP_OK;
}

int match_common(frp_handle* h, const float* q, int M, float* all_scores_host, int32_t* idx, float* cos, const uint32_t* q_groups = nullptr) {
    if (!queries_ok(q, M)) return fail(h, FRP_ERR_INVALID, "bad query arguments");
    if (h->g_rows <= 0) return fail(h, FRP_ERR_NO_GALLERY, "gallery is empty");
    FRPCHK(stage_queries(h, M, q));
    MatchGroups mg{nullptr, nullptr};
    if (q_groups) FRPCHK(stage_groups(h, M, q_groups, mg));
    ScopedBuf all;
    if (all_scores_host) FRPCHK(ensure(h, all, (size_t)M * h->g_rows * 4));
    const int rc = run_match(h, read_switches(), M, (float*)all->p, nullptr, nullptr, q_groups ? &mg : nullptr);
    return match_out(h, rc, M, idx, cos, all_scores_host, all->p, "match result copy failed");
}

// The chunked form of a match: the M queries in blocks of `chunk`, each staged in q16 and handed to block(m0, m), which matches it
// and brings its results to the host.  Waits for the stream on every path: the caller's scoped buffers go next.
template <class Block>
int match_in_chunks(frp_handle* h, const float* q, int M, int chunk, Block block) {
    int rc = FRP_OK;
    for (int m0 = 0; rc == FRP_OK && m0 < M; m0 += chunk) {
        const int m = std::min(chunk, M - m0);
        rc = stage_queries(h, m, q + (size_t)m0 * FRP_EMB_DIM);
        if (rc == FRP_OK) rc = block(m0, m);
    }
    (void)hipStreamSynchronize(h->stream);
    return rc;
}

// frp_match / frp_match_groups (q_groups: one mask per query, null: ungrouped)
int match_topk(frp_handle* h, const float* q, int M, const uint32_t* q_groups, int topk, int32_t* idx, float* cos) {
    if (topk < 1 || topk > FRP_MAX_TOPK) return fail(h, FRP_ERR_INVALID, "topk must be in 1..FRP_MAX_TOPK");
    if (topk == 1) return match_common(h, q, M, nullptr, idx, cos, q_groups);
    // k > 1: score matrix on the device (query chunks of <= 1 GiB of scores), then k selection passes per row
    if (!queries_ok(q, M) || !idx || !cos) return fail(h, FRP_ERR_INVALID, "bad query arguments");
    if (h->g_rows <= 0) return fail(h, FRP_ERR_NO_GALLERY, "gallery is empty");
    const long N = h->g_rows;
    const Switches sw = read_switches();
    const int chunk = (int)std::max<long>(1, std::min<long>(M, (1L << 28) / N));
    ScopedBuf all, didx, dcos;
    FRPCHK(ensure(h, all, (size_t)chunk * N * 4));
    FRPCHK(ensure(h, didx, (size_t)chunk * topk * 4));
    FRPCHK(ensure(h, dcos, (size_t)chunk * topk * 4));
    return match_in_chunks(h, q, M, chunk, [&](int m0, int m) -> int {
        MatchGroups mg{nullptr, nullptr};
        if (q_groups) FRPCHK(stage_groups(h, m, q_groups + m0, mg));
        FRPCHK(run_match(h, sw, m, (float*)all->p, nullptr, nullptr, q_groups ? &mg : nullptr));
        hipError_t e = launch_topk_rows((const float*)all->p, m, N, topk, (int32_t*)didx->p, (float*)dcos->p, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(idx + (size_t)m0 * topk, didx->p, (size_t)m * topk * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cos + (size_t)m0 * topk, dcos->p, (size_t)m * topk * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        return hip_rc(h, e, "match top-k: ");
    });
}

// frp_match_within / frp_match_within_groups
int match_within(frp_handle* h, const float* q, int M, const uint32_t* q_groups, float min_cos, int cap, int32_t* idx, float* cos, int32_t* n_hits) {
    if (!within_args_ok(min_cos, cap)) return fail(h, FRP_ERR_INVALID, "match_within: min_cos must be >= -2 and cap in 1..FRP_MAX_TOPK");
    if (!queries_ok(q, M) || !idx || !cos || !n_hits) return fail(h, FRP_ERR_INVALID, "bad query arguments");
    if (h->g_rows <= 0) return fail(h, FRP_ERR_NO_GALLERY, "gallery is empty");
    const Switches sw = read_switches();
    const int chunk = std::min<int>(M, 65536);
    ScopedBuf dcnt, didx, dcos;
    FRPCHK(ensure(h, dcnt, (size_t)chunk * 4));
    FRPCHK(ensure(h, didx, (size_t)chunk * cap * 4));
    FRPCHK(ensure(h, dcos, (size_t)chunk * cap * 4));
    std::vector<int> over;
    return match_in_chunks(h, q, M, chunk, [&](int m0, int m) -> int {
        int32_t* nh = n_hits + m0;
        const WithinArgs w{min_cos, cap, (int32_t*)dcnt->p, (int32_t*)didx->p, (float*)dcos->p};
        MatchGroups mg{nullptr, nullptr};
        if (q_groups) FRPCHK(stage_groups(h, m, q_groups + m0, mg));
        FRPCHK(run_match(h, sw, m, nullptr, nullptr, &w, q_groups ? &mg : nullptr));
        hipError_t e = hipMemcpyAsync(nh, dcnt->p, (size_t)m * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        FRPCHK(hip_rc(h, e, "match within: "));
        over.clear();                       // the counts are on the host: lists that overflowed are rebuilt from their score rows
        for (int i = 0; i < m; ++i)
            if (nh[i] > cap) over.push_back(i);
        if (!over.empty()) FRPCHK(rebuild_within_lists(h, over, cap, (int32_t*)didx->p, (float*)dcos->p, mg.q_groups));
        e = hipMemcpyAsync(idx + (size_t)m0 * cap, didx->p, (size_t)m * cap * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cos + (size_t)m0 * cap, dcos->p, (size_t)m * cap * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        return hip_rc(h, e, "match within: ");
    });
}

// the hit lists of the last flagged pass, compact face list -> [B][K] slots (frp.h: frp_fetch_within)
int fetch_within(frp_handle* h, int cap, int32_t* idx, float* cos, int32_t* n_hits) {
    const Matcher& m = h->m;
    const int B = h->pass.B, K = h->pass.K;
    if (B <= 0) return fail(h, FRP_ERR_INVALID, "nothing to fetch");
    if (h->pass.within_cap <= 0) return fail(h, FRP_ERR_INVALID, "fetch_within: the last pass ran without FRP_FLAG_WITHIN");
    if (cap != h->pass.within_cap) return fail(h, FRP_ERR_INVALID, "fetch_within: buffers sized for another list size than the pass used");
    if (!idx || !cos || !n_hits) return fail(h, FRP_ERR_INVALID, "fetch_within: null output");
    FRPCHK(settle_count(h, false));
    const int n = h->pass.nfaces;
    const size_t s = (size_t)B * K;
    std::fill(n_hits, n_hits + s, 0);
    std::fill(idx, idx + s * cap, -1);
    std::fill(cos, cos + s * cap, -2.0f);
    if (n <= 0 || !h->pass.within_lists) return FRP_OK;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_cnt = take((size_t)B * 4), o_hc = take((size_t)n * 4), o_hi = take((size_t)n * cap * 4), o_hs = take((size_t)n * cap * 4);
    FRPCHK(ensure_pinned(h, off));
    unsigned char* st = h->pin_stage;
    auto copy_lists = [&]() -> int {
        HIPCHK(h, hipMemcpyAsync(st + o_hi, m.hit_idx.p, (size_t)n * cap * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(st + o_hs, m.hit_cos.p, (size_t)n * cap * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return FRP_OK;
    };
    HIPCHK(h, hipMemcpyAsync(st + o_cnt, h->counts.p, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(st + o_hc, m.hit_cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    FRPCHK(copy_lists());
    settle_events(h, true);
    const int32_t* cnt = (const int32_t*)(st + o_cnt);
    const int32_t* hc = (const int32_t*)(st + o_hc);
    std::vector<int> over;
    for (int f = 0; f < n; ++f)
        if (hc[f] > cap) over.push_back(f);
    if (!over.empty()) {
        if (!h->pass.q16_of_pass)
            return fail(h, FRP_ERR_INVALID, "fetch_within: a face has more hits than the list holds and a later call replaced the pass's embeddings");
        int rc = rebuild_within_lists(h, over, cap, (int32_t*)m.hit_idx.p, (float*)m.hit_cos.p,
                                      h->pass.groups ? (const uint32_t*)m.q_groups.p : nullptr);      // (q_groups lives as long as q16_of_pass)
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

int frp::match_score_rows(frp_handle* h, const void* q16, int n, ScopedBuf (&work)[4], float* all_scores, const char* what) {
    MatchParams mp;
    FRPCHK(fill_match_params(h, q16, n, work[0], work[1], work[2], work[3], mp));
    mp.all_scores = all_scores;
    return launch_counted(h, mp, true, what);
}

int frp::match_pass(frp_handle* h, const Switches& sw, int n, const int32_t* n_dev, bool within, bool groups) {
    Matcher& m = h->m;
    MatchGroups mg{nullptr, nullptr};
    if (groups) {          // the faces' masks from their frames' (the compact face list is on the device: so is the count, with n_dev)
        const int B = h->pass.B;
        if ((int)m.frame_groups.size() != B) return fail(h, FRP_ERR_INVALID, "FRP_FLAG_GROUPS: frame masks set for another batch size");
        FRPCHK(ensure(h, m.frame_groups_dev, (size_t)B * 4));
        if (m.frame_groups_dirty) {
            HIPCHK(h, hipMemcpyAsync(m.frame_groups_dev.p, m.frame_groups.data(), (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
            if (!m.frame_groups_ev) HIPCHK(h, hipEventCreateWithFlags(&m.frame_groups_ev, hipEventDisableTiming));
            HIPCHK(h, hipEventRecord(m.frame_groups_ev, h->stream));
            m.frame_groups_copying = true;
            m.frame_groups_dirty = false;
        }
        FRPCHK(stage_groups(h, n, nullptr, mg));
        FRPCHK(hip_rc(h, launch_face_groups((const uint32_t*)m.frame_groups_dev.p, B, (const int32_t*)h->face_slot.p, h->pass.K, n, n_dev,
                                            (uint32_t*)m.q_groups.p, h->stream), "face_groups: "));
    }
    const MatchGroups* pmg = groups ? &mg : nullptr;
    if (within) {          // the same kernel with the hit-list epilogue: one gallery pass for top-1 and the lists
        const int cap = m.within_cap;
        FRPCHK(ensure(h, m.hit_cnt, (size_t)n * 4));
        FRPCHK(ensure(h, m.hit_idx, (size_t)n * cap * 4));
        FRPCHK(ensure(h, m.hit_cos, (size_t)n * cap * 4));
        const WithinArgs w{m.within_min_cos, cap, (int32_t*)m.hit_cnt.p, (int32_t*)m.hit_idx.p, (float*)m.hit_cos.p};
        FRPCHK(run_match(h, sw, n, nullptr, n_dev, &w, pmg));
        h->pass.within_lists = true;
        h->pass.q16_of_pass = true;
    } else {
        FRPCHK(run_match(h, sw, n, nullptr, n_dev, nullptr, pmg));
    }
    h->pass.matched = true;
    h->pass.groups = groups;
    return FRP_OK;
}

extern "C" {

int frp_match(frp_handle* h, const float* q, int32_t M, int32_t topk, int32_t* idx, float* cos) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    return match_topk(h, q, M, nullptr, topk, idx, cos);
}

int frp_match_groups(frp_handle* h, const float* q, int32_t M, const uint32_t* q_groups, int32_t topk, int32_t* idx, float* cos) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!q_groups || !idx || !cos) return fail(h, FRP_ERR_INVALID, "match_groups: null argument");
    return match_topk(h, q, M, q_groups, topk, idx, cos);
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
    return match_within(h, q, M, nullptr, min_cos, cap, idx, cos, n_hits);
}

int frp_match_within_groups(frp_handle* h, const float* q, int32_t M, const uint32_t* q_groups, float min_cos, int32_t cap,
                            int32_t* idx, float* cos, int32_t* n_hits) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!q_groups) return fail(h, FRP_ERR_INVALID, "match_within_groups: null masks");
    return match_within(h, q, M, q_groups, min_cos, cap, idx, cos, n_hits);
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
    if (!queries_ok(q_f16, M) || !idx || !cos) return fail(h, FRP_ERR_INVALID, "bad query arguments");
    if (h->g_rows <= 0) return fail(h, FRP_ERR_NO_GALLERY, "gallery is empty");
    if (scores && n_cols != h->g_rows) return fail(h, FRP_ERR_INVALID, "debug_match_f16: output sized for another gallery size");
    const Switches sw = read_switches();
    const int mpad = round_up(M, 32);
    if (n_device >= 0 && (scores || mpad > FRP_MATCH_TOP1_MAX || sw.match_v1 || n_device > M))
        return fail(h, FRP_ERR_INVALID, "debug_match_f16: no device-count form of this launch");
    Matcher& m = h->m;
    FRPCHK(stage_queries(h, M, nullptr, q_f16));
    FRPCHK(ensure(h, m.best_cos, (size_t)mpad * 4));
    FRPCHK(ensure(h, m.best_idx, (size_t)mpad * 4));
    ScopedBuf all, count;
    if (scores) FRPCHK(ensure(h, all, (size_t)M * h->g_rows * 4));
    if (n_device >= 0) FRPCHK(ensure(h, count, 4));
    HIPCHK(h, hipMemsetAsync(m.best_cos.p, 0xFF, (size_t)mpad * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(m.best_idx.p, 0xFF, (size_t)mpad * 4, h->stream));
    if (scores) HIPCHK(h, hipMemsetAsync(all->p, 0xFF, (size_t)M * h->g_rows * 4, h->stream));
    const int32_t n_host = n_device;          // (read by the copy below: alive until match_out has waited for the stream)
    int rc = FRP_OK;
    if (n_device >= 0 && hipMemcpyAsync(count->p, &n_host, 4, hipMemcpyHostToDevice, h->stream) != hipSuccess)
        rc = fail(h, FRP_ERR_HIP, "debug_match_f16: copy failed");
    if (rc == FRP_OK) rc = run_match(h, sw, M, (float*)all->p, n_device >= 0 ? (const int32_t*)count->p : nullptr);
    return match_out(h, rc, M, idx, cos, scores, all->p, "debug_match_f16: copy failed");
}

int frp_set_within(frp_handle* h, float min_cos, int32_t cap) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    if (!within_args_ok(min_cos, cap)) return fail(h, FRP_ERR_INVALID, "set_within: min_cos must be >= -2 and cap in 1..FRP_MAX_TOPK");
    h->m.within_min_cos = min_cos;
    h->m.within_cap = cap;
    return FRP_OK;
}

int frp_set_frame_groups(frp_handle* h, const uint32_t* masks, int32_t B) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    if (!masks || B <= 0 || B > 65536) return fail(h, FRP_ERR_INVALID, "set_frame_groups: B masks, B >= 1");
    Matcher& m = h->m;
    if ((int)m.frame_groups.size() == B && std::equal(masks, masks + B, m.frame_groups.begin())) return FRP_OK;      // the device copy stands
    if (m.frame_groups_copying) {          // a pass's upload may still be reading the vector
        HIPCHK(h, hipEventSynchronize(m.frame_groups_ev));
        m.frame_groups_copying = false;
    }
    m.frame_groups.assign(masks, masks + B);
    m.frame_groups_dirty = true;
    return FRP_OK;
}

int frp_fetch_within(frp_handle* h, int32_t B, int32_t max_faces, int32_t cap, int32_t* idx, float* cos, int32_t* n_hits) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    if (B != h->pass.B || max_faces != h->pass.K)
        return fail(h, FRP_ERR_INVALID, "fetch_within: buffers sized for another batch (results were replaced by a later call)");
    return fetch_within(h, cap, idx, cos, n_hits);
}

}  // extern "C"
