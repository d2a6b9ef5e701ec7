// One conv launch on the host: derive (argument checks, derived fields), pick (the kernel family), launch (the family's launcher,
// which ends in conv_common.h: conv_launch).  What a family covers - its constants and 32-bit reach limits - stays in its kernel's file
// (conv3x3_*_eligible, conv3x3_wino_form); the ORDER of preference between the families is conv_pick() and nowhere else.
#include "conv_common.h"

namespace frp {

// Argument checks and the derived fields of `p`; *ncu: the CU count the tile-class rules (conv_small_m) go by.
//
// Three CU counts meet in a launch, and they stay three (tests/test_conv_routes_host.py records launches at two stubbed counts to hold
// this):  *ncu here is p.n_cu as the engine set it, and the device's for the stand-alone entry points, which leave p.n_cu = 0;  the pay
// rules of the 64 -> 64 and the Winograd 2-D kernels read p.n_cu itself and take 0 as 256, so that a stand-alone call routes as on an
// MI355X whatever it runs on;  the grid (conv_launch) always goes by the device's count, and the generic kernel's launcher writes
// that one into p.n_cu for the kernel's own split-K choice - the only launcher that touches the field.
hipError_t conv_derive(ConvParams& p, int* ncu) {
    if (!(p.KS == 1 || p.KS == 3) || !(p.stride == 1 || p.stride == 2)) return hipErrorInvalidValue;
    if (p.Cin < 8 || (p.Cin & 7) || (p.Cout & 7) || p.N <= 0 || p.H <= 0 || p.W <= 0) return hipErrorInvalidValue;
    p.pad = p.KS / 2;
    p.Ho = (p.H + 2 * p.pad - p.KS) / p.stride + 1;
    p.Wo = (p.W + 2 * p.pad - p.KS) / p.stride + 1;
    const long M = (long)p.N * p.Ho * p.Wo;
    if (M <= 0 || M > 0x7fffffffL) return hipErrorInvalidValue;
    p.M = (int)M;
    p.Ktot = p.KS * p.KS * p.Cin;
    p.x2_bytes = 0;
    p.x2_shift = 0;
    if (p.x2) {                                  // K-concat: generic kernel, whole channel blocks, plain fp16 epilogue input
        if (p.KS != 3 || (p.Cin & 63) || p.Cin2 <= 0 || (p.Cin2 & 63) || !(p.Cin == p.Cin2 || p.Cin == 2 * p.Cin2) || p.ksplit > 1 ||
            (p.flags & (FRP_FLAG_F8 | FRP_FLAG_BORDER_BIAS)) || p.wino_w)
            return hipErrorInvalidValue;
        const long x2b = (long)p.N * p.H * p.W * p.Cin2 * 2;
        if (x2b >= 0x7fffffffL) return hipErrorInvalidValue;
        p.x2_bytes = (unsigned)x2b;
        p.x2_shift = p.Cin == p.Cin2 ? 0 : 1;
        p.Ktot += p.Cin2;
    }
    p.nk = (p.Ktot + 63) / 64;
    if (p.ksplit < 0 && !(p.n_dev && (p.flags & FRP_FLAG_OUT_F32) && !p.res && !(p.Cin & 63))) return hipErrorInvalidValue;
    if (p.ksplit == 0) p.ksplit = 1;
    if (p.ksplit > 1 && (p.nk % p.ksplit != 0 || !(p.flags & FRP_FLAG_OUT_F32) || p.res || (p.Cin & 63)))
        return hipErrorInvalidValue;             // split-K: exact slices, fp32 slabs, aligned path only
    // buffer descriptors carry 32-bit sizes and the kernels do signed 32-bit offset math
    const bool f8 = (p.flags & FRP_FLAG_F8) != 0;
    const int es = f8 ? 1 : 2;
    const long xb = (long)p.N * p.H * p.W * p.Cin * es, wb = (long)p.Cout * p.Ktot * es;
    if (xb >= 0x7fffffffL || wb >= 0x7fffffffL) return hipErrorInvalidValue;
    if ((p.flags & FRP_FLAG_OUT_FP8) && !f8) return hipErrorInvalidValue;
    if ((p.out2 || f8) && ((p.flags & FRP_FLAG_OUT_F32) || p.ksplit != 1 || !(p.out_scale > 0.f))) return hipErrorInvalidValue;
    p.x_bytes = (unsigned)xb;
    p.w_bytes = (unsigned)wb;
    p.cin_shift = 0;
    if (p.Cin & 63) {
        if (p.Cin & (p.Cin - 1)) return hipErrorInvalidValue;   // small path needs power-of-two Cin
        while ((1 << p.cin_shift) < p.Cin) ++p.cin_shift;
    }
    if ((p.flags & FRP_FLAG_BORDER_BIAS) && !(p.KS == 3 && p.stride == 1 && p.Ho >= 2 && p.Wo >= 2))
        return hipErrorInvalidValue;
    if ((p.flags & FRP_FLAG_RES_UP2) && (!p.res || p.Hr * 2 != p.Ho || p.Wr * 2 != p.Wo)) return hipErrorInvalidValue;
    if (!p.x || !p.w || !p.bias || !p.out) return hipErrorInvalidValue;
    if (p.act == FRP_ACT_PRELU && !p.slope) return hipErrorInvalidValue;
    *ncu = p.n_cu;
    int dev = 0;
    return p.n_cu > 0 ? hipSuccess : conv_device(&dev, ncu);
}

// The order of preference between the kernel families: Winograd -> opt-in stride-2 -> fused-stem 64 -> 64 -> 64 -> 64 -> row patch -> generic.
ConvRoute conv_pick(const ConvParams& p, int ncu) {
    ConvRoute r{ConvFamily::Invalid, false, 0, {}};
    const bool direct = (p.dbg & CONV_DBG_GENERIC) == 0;         // CONV_DBG_GENERIC: the generic kernel also where a specialised one covers the shape
    if (p.flags & FRP_FLAG_F8) {                                 // fp8 operands: only the static-loop row-patch kernel covers them
        if (conv3x3_rows_eligible(p) && !(p.Cin & 127) && p.wscale && p.in_scale > 0.f) r.family = ConvFamily::RowPatch;
        return r;
    }
    // few 256 x 128 tiles (small pyramid scales, a handful of faces): quarter tiles, two workgroups per CU (conv_small_m; the row-patch
    // family: by its own default tiles, below)
    r.few = conv_small_m(p, (long)((p.M + 255) / 256) * ((p.Cout + 127) / 128), ncu);
    // Winograd F(2,3) along the rows, 1.5 x fewer MFMAs.  (A caller that hands over the Winograd image has chosen the kernel FAMILY -
    // net_program.cpp: run_embed, by the slots of the call -; the tile count of a single launch does not overrule it: the families
    // differ in the last bits)
    if (p.wino_w && !p.x2 && direct && (r.wino_form = conv3x3_wino_form(p)) != 0) r.family = ConvFamily::Wino;
    // 3x3 stride-2 layers: row patches with shared neighbour entries (conv3x3_s2.hip).  OPT-IN (CONV_DBG_S2: FRP_S2 in the engine,
    // flags bit 21 of frp_conv2d_nhwc): on the headline shapes it measures 9-13 % SLOWER than the generic kernel's per-tap images
    // (profiles/r5/s2_probe.txt)
    else if ((p.dbg & CONV_DBG_S2) && direct && !r.few && conv3x3_s2_eligible(p)) r.family = ConvFamily::S2;
    // the embedder's stem fused into the conv behind it: only conv3x3_c64.hip does that (the caller asked conv3x3_c64_fuses_stem first)
    else if (p.stem_x) r.family = p.small_m <= 0 && conv3x3_c64_eligible(p, &r.c64) ? ConvFamily::C64 : ConvFamily::Invalid;
    // 64 -> 64 layers on large maps: weights in registers, 2-D tiles (conv3x3_c64.hip; CONV_DBG_NO_C64: the row-patch kernel instead -
    // A/B runs; bit-identical results either way)
    else if (direct && !(p.dbg & CONV_DBG_NO_C64) && p.small_m <= 0 && conv3x3_c64_eligible(p, &r.c64)) r.family = ConvFamily::C64;
    // 3x3 stride-1 layers with whole 64-channel blocks: row-patch kernel (a third of the LDS-DMA traffic)
    else if (direct && !p.x2 && conv3x3_rows_eligible(p)) {
        r.family = ConvFamily::RowPatch;
        r.few = conv_small_m(p, conv3x3_lean_default_tiles(p), ncu);
    } else r.family = ConvFamily::Generic;
    return r;
}

#ifdef FRP_LAB   // lab build: dbg bits select the first-generation row-patch kernel and its timing ablations (conv3x3_rows.hip), else it hands on to the lean one
constexpr auto launch_row_patch = launch_conv3x3_rows;
#else
constexpr auto launch_row_patch = launch_conv3x3_lean;
#endif

// Returns hipErrorInvalidValue on a shape no kernel covers instead of launching (a faulting kernel can take the node down).
hipError_t launch_conv(const ConvParams& in, hipStream_t stream) {
    ConvParams p = in;
    int ncu = 0;
    const hipError_t e = conv_derive(p, &ncu);
    if (e != hipSuccess) return e;
    const ConvRoute r = conv_pick(p, ncu);
    switch (r.family) {
        case ConvFamily::Wino: p.w = p.wino_w; return launch_conv3x3_wino(p, r.wino_form, stream);
        case ConvFamily::S2: return launch_conv3x3_s2(p, stream);
        case ConvFamily::C64: return launch_conv3x3_c64(p, r.c64, stream);
        case ConvFamily::RowPatch: return (p.flags & FRP_FLAG_F8) ? launch_conv3x3_lean(p, false, stream) : launch_row_patch(p, r.few, stream);
        case ConvFamily::Generic: return launch_conv_generic(p, r.few, stream);
        case ConvFamily::Invalid: break;
    }
    return hipErrorInvalidValue;
}

}  // namespace frp
