// frp_gallery_cluster (include/frp.h): the greedy sweep of cluster_faces on the device.  This file is the control loop - the number
// of tiles depends on the data - and the argument checks; kernels: cluster_kernels.hip, the scores: match.hip, launched unchanged.
// Per tile the host reads two words back (candidate count, cursor); no score row and no label leaves the device inside the loop.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "frp.h"
#include "frp_internal.h"
#include "frp_handle.h"

using namespace frp;

static_assert(FRP_CLUSTER_MAX_TILE == CLUSTER_MAX_TILE, "frp_internal.h: CLUSTER_MAX_TILE");

namespace {

int hip_rc(frp_handle* h, hipError_t e, const char* what) {
    return e == hipSuccess ? FRP_OK : fail(h, FRP_ERR_HIP, std::string(what) + hipGetErrorString(e));
}

// the sweep behind the argument checks; everything it allocates is scoped.  Returns FRP_OK with the stream idle.
int cluster_sweep(frp_handle* h, const int32_t* order, int n, float min_cos, double max_dist, int tile, bool exact, int32_t* seed_pos,
                  int32_t* n_clusters) {
    const long N = h->g_rows;
    ScopedBuf d_order, d_seed, d_ctl, score, q, q32, work[4];
    FRPCHK(ensure(h, d_order, (size_t)n * 4));
    FRPCHK(ensure(h, d_seed, (size_t)n * 4));
    FRPCHK(ensure(h, d_ctl, (size_t)CLUSTER_CTL_WORDS * 4));
    FRPCHK(ensure(h, score, (size_t)tile * N * (exact ? 8 : 4)));
    const size_t qbytes = exact ? (size_t)tile * FRP_EMB_DIM * 8 : (size_t)round_up(tile, 32) * FRP_EMB_DIM * 2;
    FRPCHK(ensure(h, q, qbytes));
    if (!exact) FRPCHK(ensure(h, q32, (size_t)tile * FRP_EMB_DIM * 4));
    FRPCHK(ensure_pinned(h, 256));
    int32_t* back = (int32_t*)h->pin_stage;          // [count, cursor] of the tile, then the number of clusters
    HIPCHK(h, hipMemcpyAsync(d_order->p, order, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(d_seed->p, 0xFF, (size_t)n * 4, h->stream));          // -1: unassigned
    HIPCHK(h, hipMemsetAsync(d_ctl->p, 0, (size_t)CLUSTER_CTL_WORDS * 4, h->stream));
    const ClusterParams cp{(const int32_t*)d_order->p, n, N, tile, (int32_t*)d_seed->p, (int32_t*)d_ctl->p};
    for (;;) {
        FRPCHK(hip_rc(h, launch_cluster_pick(cp, h->stream), "cluster pick: "));
        HIPCHK(h, hipMemcpyAsync(back, d_ctl->p, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const int count = back[CLUSTER_CTL_COUNT], cursor = back[CLUSTER_CTL_CURSOR];
        if (count < 0 || count > tile || cursor < 0 || cursor > n) return fail(h, FRP_ERR_HIP, "cluster: candidate pick out of range");
        if (count == 0) break;
        if (exact) {
            FRPCHK(hip_rc(h, launch_cluster_stage_f64(cp, (const double*)h->gx.p, (double*)q->p, h->stream), "cluster stage: "));
            FRPCHK(hip_rc(h, launch_gallery_distances((const double*)h->gx.p, N, (const double*)q->p, count, (double*)score->p, h->stream),
                          "cluster distances: "));
            FRPCHK(hip_rc(h, launch_cluster_sweep_dist(cp, (const double*)score->p, max_dist, h->stream), "cluster sweep: "));
        } else {
            HIPCHK(h, hipMemsetAsync(q->p, 0, qbytes, h->stream));          // rows >= count of the query block are zero
            FRPCHK(hip_rc(h, launch_cluster_stage_f16(cp, (const _Float16*)h->gallery.p, (float*)q32->p, h->stream), "cluster stage: "));
            FRPCHK(hip_rc(h, launch_gallery_normalize((const float*)q32->p, (_Float16*)q->p, count, FRP_EMB_DIM, h->stream), "cluster stage: "));
            FRPCHK(match_score_rows(h, q->p, count, work, (float*)score->p, "cluster scores: "));
            FRPCHK(hip_rc(h, launch_cluster_sweep_cos(cp, (const float*)score->p, min_cos, h->stream), "cluster sweep: "));
        }
        if (cursor >= n) break;          // the tile took the last unassigned position
    }
    HIPCHK(h, hipMemcpyAsync(seed_pos, d_seed->p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(back, (const int32_t*)d_ctl->p + CLUSTER_CTL_NCLUSTERS, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_clusters = back[0];
    return FRP_OK;
}

}  // namespace

extern "C" {

int frp_gallery_cluster(frp_handle* h, const int32_t* order, int64_t n, float min_cos, double max_dist, int32_t tile, uint32_t flags,
                        int32_t* seed_pos, int32_t* n_clusters) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h);
    if (!order || !seed_pos || !n_clusters) return fail(h, FRP_ERR_INVALID, "gallery_cluster: null argument");
    if (flags & ~FRP_CLUSTER_EXACT) return fail(h, FRP_ERR_INVALID, "gallery_cluster: unknown flag");
    if (tile == 0) tile = FRP_CLUSTER_MAX_TILE;
    if (tile < 1 || tile > FRP_CLUSTER_MAX_TILE) return fail(h, FRP_ERR_INVALID, "gallery_cluster: tile must be in 1..FRP_CLUSTER_MAX_TILE (0: the largest)");
    if (h->g_rows <= 0) return fail(h, FRP_ERR_NO_GALLERY, "gallery is empty");
    const bool exact = (flags & FRP_CLUSTER_EXACT) != 0;
    if (exact && !h->g_exact) return fail(h, FRP_ERR_INVALID, "gallery_cluster: FRP_CLUSTER_EXACT without exact rows (frp_gallery_exact)");
    if (n <= 0 || n > h->g_rows) return fail(h, FRP_ERR_INVALID, "gallery_cluster: order must hold 1..gallery size distinct rows");
    std::vector<uint8_t> seen((size_t)h->g_rows, 0);
    for (int64_t p = 0; p < n; ++p) {
        const int64_t r = order[p];
        if (r < 0 || r >= h->g_rows) return fail(h, FRP_ERR_INVALID, "gallery_cluster: order[" + std::to_string(p) + "] is not a gallery row");
        if (seen[(size_t)r]) return fail(h, FRP_ERR_INVALID, "gallery_cluster: order[" + std::to_string(p) + "] lists a row a second time");
        seen[(size_t)r] = 1;
    }
    const int rc = cluster_sweep(h, order, (int)n, min_cos, max_dist, tile, exact, seed_pos, n_clusters);
    if (rc != FRP_OK) (void)hipStreamSynchronize(h->stream);          // (nothing queued still reads or writes the caller's arrays)
    return rc;
}

}  // extern "C"
