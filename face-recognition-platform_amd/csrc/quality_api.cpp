// frp_face_quality (include/frp.h): the blur / lighting sums of rectangles of the resident frames (quality_kernels.hip).
#include <hip/hip_runtime.h>

#include <cstring>

#include "frp.h"
#include "frp_handle.h"

using namespace frp;

extern "C" {

int frp_face_quality(frp_handle* h, const int32_t* rects, int32_t n, uint32_t flags, int64_t* sums) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);      // queued behind whatever pass is pending; its stage events are read after this call's own wait
    if (h->rB <= 0 || !h->frames.p) return fail(h, FRP_ERR_INVALID, "face_quality: no resident frames");
    if (n < 0) return fail(h, FRP_ERR_INVALID, "face_quality: n < 0");
    if (flags & ~FRP_FLAG_RGB) return fail(h, FRP_ERR_INVALID, "face_quality: flags other than FRP_FLAG_RGB");
    if (n == 0) return FRP_OK;
    if (!rects || !sums) return fail(h, FRP_ERR_INVALID, "face_quality: null rects / sums");
    // rectangles and, behind them, the prefix of their tile counts: one upload
    std::vector<int32_t> up((size_t)n * 5 + (size_t)n + 1);
    std::memcpy(up.data(), rects, (size_t)n * 5 * sizeof(int32_t));
    int32_t* prefix = up.data() + (size_t)n * 5;
    int64_t tiles = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t *r = rects + (size_t)i * 5, f = r[0], top = r[1], right = r[2], bottom = r[3], left = r[4];
        if (!(f >= 0 && f < h->rB && top >= 0 && top < bottom && bottom <= h->rH && left >= 0 && left < right && right <= h->rW))
            return fail(h, FRP_ERR_INVALID, "face_quality: rectangle " + std::to_string(i) + " (frame " + std::to_string(f) + ", top " +
                        std::to_string(top) + ", right " + std::to_string(right) + ", bottom " + std::to_string(bottom) + ", left " +
                        std::to_string(left) + ") is empty or outside the " + std::to_string(h->rB) + " resident frames of " +
                        std::to_string(h->rH) + " x " + std::to_string(h->rW));
        prefix[i] = (int32_t)tiles;
        tiles += (int64_t)((bottom - top + QUALITY_TILE_H - 1) / QUALITY_TILE_H) * ((right - left + QUALITY_TILE_W - 1) / QUALITY_TILE_W);
        if (tiles > 0x7fffffffLL) return fail(h, FRP_ERR_INVALID, "face_quality: more than 2^31 - 1 tiles in one call");
    }
    prefix[n] = (int32_t)tiles;
    const size_t in_bytes = up.size() * sizeof(int32_t), part_bytes = (size_t)tiles * 4 * sizeof(int64_t), sum_bytes = (size_t)n * 4 * sizeof(int64_t);
    FRPCHK(ensure(h, h->quality_in, in_bytes));
    FRPCHK(ensure(h, h->quality_out, part_bytes + sum_bytes));
    QualityParams p{};
    p.frames = (const uint8_t*)h->frames.p;
    p.B = h->rB; p.H = h->rH; p.W = h->rW;
    p.total_bytes = (long long)h->rB * h->rH * h->rW * 3;
    p.rgb_in = (flags & FRP_FLAG_RGB) ? 1 : 0;
    p.rects = (const int32_t*)h->quality_in.p;
    p.tile_prefix = p.rects + (size_t)n * 5;
    p.n = n;
    p.n_tiles = (int)tiles;
    p.partials = (long long*)h->quality_out.p;
    p.sums = p.partials + (size_t)tiles * 4;
    hipError_t e = hipMemcpyAsync(h->quality_in.p, up.data(), in_bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = launch_face_quality(p, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sums, p.sums, sum_bytes, hipMemcpyDeviceToHost, h->stream);
    hipError_t e2 = hipStreamSynchronize(h->stream);      // (`up` and `sums` are the caller's / this frame's until here)
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("face_quality: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("face_quality sync: ") + hipGetErrorString(e2));
    settle_events(h, true);
    return FRP_OK;
}

}  // extern "C"
