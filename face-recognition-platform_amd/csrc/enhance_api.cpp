// frp_enhance_pixels, frp_encode_jpeg_enhanced (include/frp.h): Pillow's resize(BICUBIC) + UnsharpMask of rectangles of the resident
// frames (enhance_kernels.hip), as pixels or - through the encoder of jpeg_encode_api.cpp, device buffer to device buffer - as JPEG files.
// The floating-point half of Pillow's arithmetic is here: the resample's tap tables (Resample.c: precompute_coeffs + normalize_coeffs_8bpc,
// in double) and the blur's box radius and weights (BoxBlur.c).  The kernels do integer work only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <map>

#include "frp.h"
#include "frp_handle.h"

using namespace frp;

namespace {

#pragma clang fp contract(off)      // every product and sum rounds on its own, as in Pillow's build

double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// the taps of one axis, n_out >= n_in (support 2, never widened: at most 5 per sample); an axis that keeps its size is not
// resampled by Pillow: one tap of 2^22, which the kernel's rounding turns into the sample itself
void axis_taps(int n_in, int n_out, EnhanceTap* t) {
    for (int xx = 0; xx < n_out; ++xx) {
        EnhanceTap& e = t[xx];
        e = EnhanceTap{};
        if (n_in == n_out) {
            e.first = xx; e.count = 1; e.k[0] = 1 << 22;
            continue;
        }
        const double scale = (double)n_in / (double)n_out, support = 2.0;
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > n_in) xmax = n_in;
        xmax -= xmin;
        if (xmax > ENH_MAX_TAPS) xmax = ENH_MAX_TAPS;          // (never: 2 * support + 1)
        double w[ENH_MAX_TAPS], ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = bicubic(x + xmin - center + 0.5);
            ww += w[x];
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) w[x] /= ww;
            e.k[x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << 22)) : (int)(0.5 + w[x] * (1 << 22));
        }
        e.first = xmin; e.count = xmax;
    }
}

// GaussianBlur(radius) = three box passes per axis of this (fractional) radius: its integer part and the two weights of a pass
void box_params(float radius, int& r, uint32_t& ww, uint32_t& fw) {
    const double sigma2 = (double)radius * (double)radius / 3;
    const double L = std::sqrt(12 * sigma2 + 1);
    const double l = std::floor((L - 1) / 2);
    const double a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2) / (6 * (sigma2 - (l + 1) * (l + 1)));
    const float fr = (float)(l + a);
    r = (int)fr;
    ww = (uint32_t)((float)(1 << 24) / (fr * 2 + 1));
    fw = ((1u << 24) - (uint32_t)(2 * r + 1) * ww) / 2;
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

struct Plan {
    std::vector<EnhanceImage> img;
    std::vector<EnhanceTap> taps;
    EnhanceParams p{};
};

// every check of the two entry points' shared arguments, the images' geometry and tables; nothing is launched.  FRP_OK with n == 0: nothing to do
int plan(frp_handle* h, const std::string& w, const int32_t* rects, const int32_t* sizes, int32_t n, const frp_enhance_params* prm, uint32_t flags,
         uint32_t allowed, Plan& pl) {
    if (h->rB <= 0 || !h->frames.p) return fail(h, FRP_ERR_INVALID, w + ": no resident frames");
    if (n < 0) return fail(h, FRP_ERR_INVALID, w + ": n < 0");
    if (flags & ~allowed)
        return fail(h, FRP_ERR_INVALID, w + ": flags other than FRP_FLAG_RGB" + ((allowed & FRP_FLAG_JPEG_OPTIMIZE) ? " and FRP_FLAG_JPEG_OPTIMIZE" : ""));
    if (!prm) return fail(h, FRP_ERR_INVALID, w + ": null params");
    if (!(prm->radius >= 0.f && prm->radius <= FRP_ENHANCE_MAX_RADIUS))      // (NaN fails both)
        return fail(h, FRP_ERR_INVALID, w + ": radius outside 0.." + std::to_string(FRP_ENHANCE_MAX_RADIUS));
    if (prm->percent < 0) return fail(h, FRP_ERR_INVALID, w + ": percent < 0");
    if (prm->threshold < 0) return fail(h, FRP_ERR_INVALID, w + ": threshold < 0");
    EnhanceParams& p = pl.p;
    p.sharpen = prm->sharpen ? 1 : 0;
    p.percent = prm->percent; p.threshold = prm->threshold;
    box_params(prm->radius, p.box_r, p.ww, p.fw);
    if (p.box_r < 0 || p.box_r > ENH_MAX_BOX_R) return fail(h, FRP_ERR_INVALID, w + ": radius beyond the kernel's halo");
    if (n == 0) return FRP_OK;
    if (!rects || !sizes) return fail(h, FRP_ERR_INVALID, w + ": null rects / sizes");
    pl.img.resize((size_t)n);
    std::map<std::pair<int, int>, int> seen;        // (in, out) -> first entry of the axis' taps: crops of one size share them
    long long tiles = 0, out_bytes = 0;
    for (int32_t i = 0; i < n; ++i) {
        FRPCHK(jpeg_enc_check_rect(h, w, rects, i));
        const int32_t *r = rects + (size_t)i * 5, ow = sizes[2 * (size_t)i], oh = sizes[2 * (size_t)i + 1];
        EnhanceImage& I = pl.img[(size_t)i];
        I = EnhanceImage{};
        I.frame = r[0]; I.top = r[1]; I.left = r[4]; I.h = r[3] - r[1]; I.w = r[2] - r[4];
        if (ow < I.w || oh < I.h || ow > 65535 || oh > 65535 || (long long)ow * oh > FRP_ENHANCE_MAX_PIXELS)
            return fail(h, FRP_ERR_INVALID, w + ": rectangle " + std::to_string(i) + " (" + std::to_string(I.w) + " x " + std::to_string(I.h) +
                        ") cannot become " + std::to_string(ow) + " x " + std::to_string(oh) + ": the output is at least the rectangle, at most 65535 a side and " +
                        std::to_string(FRP_ENHANCE_MAX_PIXELS) + " pixels");
        I.ow = ow; I.oh = oh;
        I.tiles_x = (ow + ENH_TILE_W - 1) / ENH_TILE_W;
        I.tile0 = (int)tiles;
        tiles += (long long)I.tiles_x * ((oh + ENH_TILE_H - 1) / ENH_TILE_H);
        I.out0 = out_bytes;
        out_bytes += (long long)ow * oh * 3;
        for (int axis = 0; axis < 2; ++axis) {
            const int n_in = axis ? I.h : I.w, n_out = axis ? oh : ow;
            auto it = seen.find({n_in, n_out});
            if (it == seen.end()) {
                it = seen.insert({{n_in, n_out}, (int)pl.taps.size()}).first;
                pl.taps.resize(pl.taps.size() + (size_t)n_out);
                axis_taps(n_in, n_out, pl.taps.data() + it->second);
            }
            (axis ? I.ytap : I.xtap) = it->second;
        }
        if (tiles > 0x7fffffffLL || pl.taps.size() > 0x7fffffffull / sizeof(EnhanceTap))
            return fail(h, FRP_ERR_INVALID, w + ": more than 2^31 - 1 tiles or table bytes in one call");
    }
    p.frames = (const uint8_t*)h->frames.p;
    p.B = h->rB; p.H = h->rH; p.W = h->rW;
    p.total_bytes = (long long)h->rB * h->rH * h->rW * 3;
    p.n = n;
    p.n_tiles = (int)tiles;
    p.n_taps = (int)pl.taps.size();
    p.out_bytes = out_bytes;
    return FRP_OK;
}

// images + tables to the device, the kernel queued; `up` is read by the copy until the caller has waited
int enqueue(frp_handle* h, Plan& pl, std::vector<uint8_t>& up) {
    const size_t img_bytes = align16(pl.img.size() * sizeof(EnhanceImage)), tap_bytes = pl.taps.size() * sizeof(EnhanceTap);
    up.assign(img_bytes + tap_bytes, 0);
    std::memcpy(up.data(), pl.img.data(), pl.img.size() * sizeof(EnhanceImage));
    std::memcpy(up.data() + img_bytes, pl.taps.data(), tap_bytes);
    FRPCHK(ensure(h, h->enh_in, up.size()));
    FRPCHK(ensure(h, h->enh_out, align16((size_t)pl.p.out_bytes)));
    pl.p.img = (const EnhanceImage*)h->enh_in.p;
    pl.p.taps = (const EnhanceTap*)((const uint8_t*)h->enh_in.p + img_bytes);
    pl.p.out = (uint8_t*)h->enh_out.p;
    HIPCHK(h, hipMemcpyAsync(h->enh_in.p, up.data(), up.size(), hipMemcpyHostToDevice, h->stream));
    hipError_t e = launch_enhance(pl.p, h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        settle_events(h, true);
        return fail(h, FRP_ERR_HIP, std::string("enhance: ") + hipGetErrorString(e));
    }
    return FRP_OK;
}

}  // namespace

extern "C" {

int frp_enhance_pixels(frp_handle* h, const int32_t* rects, const int32_t* sizes, int32_t n, const frp_enhance_params* params, uint32_t flags,
                       uint8_t* out, int64_t out_cap, int64_t* offsets) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);      // queued behind whatever pass is pending; its stage events are read after this call's own wait
    Plan pl;
    FRPCHK(plan(h, "enhance_pixels", rects, sizes, n, params, flags, FRP_FLAG_RGB, pl));
    if (out_cap < 0) return fail(h, FRP_ERR_INVALID, "enhance_pixels: out_cap < 0");
    if (!offsets) return fail(h, FRP_ERR_INVALID, "enhance_pixels: null offsets");
    if (n == 0) {
        offsets[0] = 0;
        return FRP_OK;
    }
    for (int32_t i = 0; i < n; ++i) offsets[i] = pl.img[(size_t)i].out0;
    offsets[n] = pl.p.out_bytes;
    if (pl.p.out_bytes > out_cap)
        return fail(h, FRP_ERR_INVALID, "enhance_pixels: the images take " + std::to_string(pl.p.out_bytes) + " bytes, out_cap is " + std::to_string(out_cap));
    if (!out) return fail(h, FRP_ERR_INVALID, "enhance_pixels: null out");
    std::vector<uint8_t> up;
    FRPCHK(enqueue(h, pl, up));
    hipError_t e = hipMemcpyAsync(out, pl.p.out, (size_t)pl.p.out_bytes, hipMemcpyDeviceToHost, h->stream);
    hipError_t e2 = hipStreamSynchronize(h->stream);      // (`up` and `out` are this frame's / the caller's until here)
    settle_events(h, true);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("enhance_pixels: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("enhance_pixels sync: ") + hipGetErrorString(e2));
    return FRP_OK;
}

int frp_encode_jpeg_enhanced(frp_handle* h, const int32_t* rects, const int32_t* sizes, int32_t n, const frp_enhance_params* params, int32_t quality,
                             int32_t subsampling, int32_t restart_mcus, uint32_t flags, uint8_t* out, int64_t out_cap, int64_t* offsets) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    const std::string w("encode_jpeg_enhanced");
    Plan pl;
    FRPCHK(plan(h, w, rects, sizes, n, params, flags, FRP_FLAG_RGB | FRP_FLAG_JPEG_OPTIMIZE, pl));
    std::vector<JpegEncSource> src((size_t)std::max(n, 0));
    for (int32_t i = 0; i < n; ++i) src[(size_t)i] = JpegEncSource{pl.img[(size_t)i].out0 / 3, pl.img[(size_t)i].ow, pl.img[(size_t)i].ow, pl.img[(size_t)i].oh};
    std::vector<JpegEncImage> img;
    JpegEncParams jp;
    FRPCHK(jpeg_enc_plan_buffer(h, w, src.data(), n, quality, subsampling, restart_mcus, flags, img, jp));
    if (out_cap < 0) return fail(h, FRP_ERR_INVALID, w + ": out_cap < 0");
    if (!offsets) return fail(h, FRP_ERR_INVALID, w + ": null offsets");
    if (n == 0) {
        offsets[0] = 0;
        return FRP_OK;
    }
    std::vector<uint8_t> up;
    FRPCHK(enqueue(h, pl, up));
    jp.frames = pl.p.out;                                   // the enhanced pixels never leave the device: the encoder reads them where they are
    jp.total_bytes = pl.p.out_bytes;
    return jpeg_enc_files(h, w, img, jp, quality, (flags & FRP_FLAG_JPEG_OPTIMIZE) != 0, out, out_cap, offsets);      // (waits also on its error paths: `up` lives long enough)
}

}  // extern "C"
