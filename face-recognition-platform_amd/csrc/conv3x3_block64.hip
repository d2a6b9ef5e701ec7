// K2f: a whole residual block of two 3x3 stride-1 64 -> 64 convolutions in ONE launch:  out = act2(conv2(act1(conv1(x))) + x).
//
// Why.  On the largest maps (the detector's 272 x 480 stage, the embedder's 56 x 56 stage) the two launches of such a block write the
// intermediate tensor to HBM, read it straight back, and fetch the residual a second time: five passes over a map of which the result
// needs two.  Time on these layers is memory time PLUS matrix time (profiles/r5/c64_probe.txt), so deleted bytes are deleted time.
// Here the intermediate lives in LDS only and the residual is the centre of the input rows that are in LDS anyway.
//
// Shape of the work.  A work item is (image, strip of 30 output columns, segment of rows); a workgroup marches down its strip four
// rows per step.  The intermediate row of a strip is 30 + 2 halo columns = exactly one 32-pixel MFMA block; conv2's output row uses 30
// of the 32 lanes of a block; the input row is 34 pixels.
//   * Waves specialised by layer: waves 0-3 hold conv1's weights, waves 4-7 conv2's (32 couts x K = 576 = 144 registers each, as in
//     conv3x3_c64.hip - both layers' 288 registers would not fit one wave at two waves per SIMD).  Wave w and w + 4 share a SIMD, so
//     every SIMD hosts one wave of each layer and one wave's MFMAs run under its partner's epilogue.  Within a layer: 2 pixel groups
//     (rows 2 wp, 2 wp + 1 of the step) x 2 cout groups.  A wave runs 2 pixel blocks x 36 k-slices per step: the inner loop is c64's.
//   * Step k of an item (segment rows ys .. ye - 1, K = ceil((ye - ys + 2) / 4), steps 0 .. K):
//       conv1 (k < K)  computes intermediate rows ys - 1 + 4k .. + 3 from input rows ys - 2 + 4k .. ys + 3 + 4k,
//       conv2 (k >= 1) computes output rows      ys - 6 + 4k .. + 3 from intermediate rows ys - 7 + 4k .. ys - 2 + 4k
//     (conv2 runs one step + two rows behind: the rows it needs are complete at the barrier in front of its step.  Its first two rows
//     and whatever lies beyond ye are computed and not stored: unconditional buffer stores with an out-of-range offset.)
//     A segment recomputes the intermediate rows at its seams (ys - 1 and ye) from real input rows.
//   * Rings in LDS, indices relative to the item:
//       input rows  i = y - (ys - 6) in groups of four, group g in slot g & 3 (20 KiB each: 4 rows x 34 pixels x 144 B + the tail of the
//                   20th LDS-DMA piece).  Group g arrives by LDS-DMA (conv1's waves, five pieces each); pixels outside the image are
//                   zero-filled by the DMA itself (out-of-range source offsets): conv1's padding.
//       intermediate rows  m = y - (ys - 7), row m in slot m & 15 (32 pixels x 144 B), written by conv1's epilogue as fp16 - rounded
//                   exactly where the unfused launch rounds its output - with ZEROS for pixels outside the image (row -1, row H,
//                   columns outside [0, W)): they are conv2's padding, not conv1 evaluated on padding.
//     Both keep the 144-byte pixel pitch of conv3x3_c64.hip: every fragment read is a row base + an immediate, conflict-free.
//   * One barrier per step.  In front of it every wave retires its LDS operations (retire_lds_reads: reads returned, epilogue writes
//     done) and conv1's waves wait for their DMA pieces.  Write after read, per ring:
//       input:  step k reads groups k (conv2: residual), k + 1, k + 2 (conv1).  The DMA issued in step k (behind the barrier) fills
//               group k + 3 = slot (k - 1) & 3, whose last readers ran in step k - 1 and retired their reads in front of this
//               barrier.  Group k + 3 is waited for at the barrier in front of step k + 1, where it is first read.
//       intermediate:  conv1 writes rows m = 6 + 4k .. 9 + 4k in step k while conv2 reads rows 4k .. 4k + 5: ten consecutive rows of
//               a 16-row ring, disjoint; the slots conv1 writes held rows m - 16, last read in step k - 2.  conv2 reads them from
//               step k + 1 on, behind the barrier that follows conv1's retired writes.
//     Between two items one more barrier: the next item's first groups go into slots the last step may still be reading.
//   * Same bits as the two launches: accumulation order (kh, kw, 16-channel slice) in fp32, epilogue arithmetic from its one
//     definition (conv_common.h: epi_*; the nine border classes go by the intermediate pixel's true image position).
//     tests/test_gpu_block64.py compares with np.array_equal.
//
// Replaces the same reference calls as conv_mfma.hip (face_recognition.face_locations / face_encodings,
// backend/app/routes/camera.py:232,237).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "frp_internal.h"
#include "conv_common.h"

namespace frp {

#define B64_PITCH 144                          // LDS bytes per pixel (conv3x3_c64.hip: C64_PITCH)
#define B64_IN_ROW (BLOCK64_IN_W * B64_PITCH)  // 4896
#define B64_IN_PIECES 20                       // LDS-DMA pieces per group of four input rows (4 x 4896 = 19584 B <= 20 KiB)
#define B64_IN_GRP (B64_IN_PIECES * 1024)
#define B64_IN_NGRP 4
#define B64_MID_ROW (32 * B64_PITCH)           // 4608
#define B64_MID_ROWS 16
#define B64_OFF_MID (B64_IN_NGRP * B64_IN_GRP)
#define B64_OFF_PAR (B64_OFF_MID + B64_MID_ROWS * B64_MID_ROW + 512)   // (+ the two pixels conv2's unused lanes 30, 31 read past a row)
#define B64_LDS (B64_OFF_PAR + (9 * 64 + 3 * 64) * 4)
static_assert(4 * B64_IN_ROW <= B64_IN_GRP && 4 * BLOCK64_IN_W * 9 <= B64_IN_PIECES * 64, "input group");
static_assert(B64_LDS == BLOCK64_LDS_BYTES && B64_LDS <= 160 * 1024, "LDS budget (frp_internal.h: BLOCK64_LDS_BYTES)");
#ifndef B64_ABL
#define B64_ABL 0                              // lab builds: timing ablations (1: no output stores, 2: no input DMA, 4: no MFMAs; wrong results)
#endif

template <int ACT1, bool BORDER1, int ACT2>
__global__ __launch_bounds__(512, 2) void conv3x3_block64_kernel(Block64Params p_in) {
    extern __shared__ __attribute__((aligned(256))) unsigned char smem[];
    Block64Params p = p_in;
    const int N = p.n_dev ? conv_image_count(*p.n_dev, p.N) : p.N;      // image count known on the device only (threshold mode)
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int layer = wave >> 2, wl = wave & 3, wc = wl & 1, wp = wl >> 1;
    const int fr = lane & 31, fh = lane >> 5;
    const int per_img = p.strips * p.segs;
    const int n_items = N * per_img;
    const int H = p.H, W = p.W;

    const unsigned io_bytes = (unsigned)((long)p.N * H * W * 128);                    // (< 2 GiB: launcher)
    const __amdgpu_buffer_rsrc_t xrsrc = conv_rsrc(p.x, io_bytes);
    const __amdgpu_buffer_rsrc_t orsrc = conv_rsrc(p.out, io_bytes);

    // ---------------- epilogue parameters: conv1 bias [9][64] (class-major) and slope, conv2 bias and slope
    float* lds_bias1 = reinterpret_cast<float*>(smem + B64_OFF_PAR);
    float* lds_slope1 = lds_bias1 + 9 * 64;
    float* lds_bias2 = lds_slope1 + 64;
    float* lds_slope2 = lds_bias2 + 64;
    for (int i = t; i < 9 * 64; i += 512) lds_bias1[i] = (BORDER1 || i < 64) ? p.bias1[i] : 0.f;
    if (t < 64) {
        lds_slope1[t] = (ACT1 == FRP_ACT_PRELU && p.slope1) ? p.slope1[t] : 0.f;
        lds_bias2[t] = p.bias2[t];
        lds_slope2[t] = (ACT2 == FRP_ACT_PRELU && p.slope2) ? p.slope2[t] : 0.f;
    }

    // ---------------- this wave's weights: 32 couts x K = 576 of ITS layer as 36 MFMA A fragments (k-slice s = tap * 4 + kk)
    half8 A[36];
    {
        const _Float16* wrow = (layer ? p.w2 : p.w1) + (long)(wc * 32 + fr) * 576 + 8 * fh;
#pragma unroll
        for (int s = 0; s < 36; ++s) A[s] = *reinterpret_cast<const half8*>(wrow + (s >> 2) * 64 + (s & 3) * 16);
    }
    __syncthreads();                           // parameters visible

    int lane_e = lane;                         // (made opaque per step: the compiler must not keep the DMA lane tables in registers)
    const int lbase = fr * B64_PITCH + fh * 16;
    floatx16 acc[2];

    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const Block64Item wi = block64_item(item, p.strips, p.segs, p.seg_rows, H);
        const int n = wi.n, ys = wi.ys, ye = wi.ye, x0 = wi.x0, K = wi.K;

        // the last step of the item before may still be reading the slots this item's first groups go into
        retire_lds_reads();
        __builtin_amdgcn_s_barrier();

        // the 72 MFMAs of a step: pixel block b, tap (kh, kw), slice kk reads row pointer rp[b + kh] + kw * 144 + kk * 32
        auto multiply = [&](const auto& rp) __attribute__((always_inline)) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[b][e] = 0.f;
            half8 bf[3][2];                    // fragments of k-slices s, s + 1, s + 2 (requested two slices ahead of their MFMAs)
            auto rd = [&](int s, int S) {
                const int tap = s >> 2, kk = s & 3;
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    bf[S][b] = *reinterpret_cast<const half8*>(rp[b + tap / 3] + (tap % 3) * B64_PITCH + kk * 32);
            };
            rd(0, 0);
            rd(1, 1);
#pragma unroll
            for (int s = 0; s < 36; ++s) {
                if (s + 2 < 36) rd(s + 2, (s + 2) % 3);
                if (!(B64_ABL & 4)) {
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[s], bf[s % 3][b], acc[b], 0, 0, 0);
                } else {
                    asm volatile("" ::"v"(bf[s % 3][0]), "v"(bf[s % 3][1]));
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };

        if (layer == 0) {
            // ================= conv1: input rows by LDS-DMA, intermediate rows into LDS
            // group g = input rows ys - 6 + 4g .. + 3: piece j of this wave fills the 16-byte slots 64 (wl + 4j) + lane of the group:
            // slot q = chunk q % 9 (8: the pad) of group pixel R = q / 9 = (row R / 34, column R % 34); column 0 = image column x0 - 2
            auto issue_group = [&](int g) {
                if (B64_ABL & 2) return;
                const int gy = ys - 6 + 4 * g;
                unsigned char* dst = smem + (g & 3) * B64_IN_GRP;
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const int piece = wl + 4 * j;
                    const int sl = piece * 64 + lane_e;
                    const int R = (sl * 7282) >> 16, chunk = sl - 9 * R;            // sl / 9, sl % 9 (exact for sl < 3072)
                    const int py = (R * 241) >> 13, px = R - py * BLOCK64_IN_W;      // R / 34 (exact for R < 384)
                    const int y = gy + py, x = x0 - 2 + px;
                    const bool ok = R < 4 * BLOCK64_IN_W && chunk < 8 && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
                    dma16(xrsrc, dst + piece * 1024, ok ? (unsigned)(((n * H + y) * W + x) * 128 + chunk * 16) : CONV_OOB);
                }
            };
            issue_group(1);
            issue_group(2);
            for (int k = 0; k <= K; ++k) {
                wait_vmcnt<0>();               // this wave's pieces of group k + 2 (issued a whole step ago) have landed
                retire_lds_reads();
                __builtin_amdgcn_s_barrier();
                if (k == K) break;             // (conv2's last step: nothing left for this layer)
                asm volatile("" : "+v"(lane_e));
                if (k + 3 <= K + 1) issue_group(k + 3);
                const int ib = 4 * (k + 1) + 2 * wp;             // relative input row of (block 0, kh 0)
                const unsigned char* rp[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = ib + j;
                    rp[j] = smem + (((i >> 2) & 3) * B64_IN_GRP + (i & 3) * B64_IN_ROW) + lbase;
                }
                multiply(rp);
                // epilogue: lane = intermediate pixel (row my, image column x0 - 1 + fr), registers 4g .. 4g+3 = couts 32 wc + 8g + 4 fh .. + 3
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int my = ys - 1 + 4 * k + 2 * wp + b, mx = x0 - 1 + fr;
                    const bool inimg = (unsigned)my < (unsigned)H && (unsigned)mx < (unsigned)W;
                    int cls = 0;
                    if (BORDER1) cls = epi_border_class(my, mx, H, W);
                    if (!inimg) cls = 0;
                    half4 pk[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        floatx4 v;
                        epi_value<ACT1, 0>(v, 0, acc[b], g, lds_bias1 + cls * 64, lds_slope1, wc * 32 + 8 * g + 4 * fh);
                        pk[g] = epi_half4(v);
                    }
                    const int ms = (6 + 4 * k + 2 * wp + b) & (B64_MID_ROWS - 1);
                    unsigned char* mrow = smem + B64_OFF_MID + ms * B64_MID_ROW + lbase + wc * 64;
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        u32x4 o = epi_chunk(pk[2 * q], pk[2 * q + 1]);              // couts 32 wc + 16 q + 8 fh .. + 7
                        if (!inimg) o = u32x4{0u, 0u, 0u, 0u};                   // conv2's zero padding
                        *reinterpret_cast<u32x4*>(mrow + q * 32) = o;
                    }
                }
            }
        } else {
            // ================= conv2: intermediate rows from LDS, residual = centre of the input rows in LDS, output to HBM
            for (int k = 0; k <= K; ++k) {
                retire_lds_reads();            // (only stores of this wave are in flight: no memory wait)
                __builtin_amdgcn_s_barrier();
                if (k == 0) continue;          // (conv1's first step: no intermediate rows yet)
                const int ib = 4 * k + 2 * wp;                   // relative intermediate row of (block 0, kh 0); = relative input row of block 0
                const unsigned char* rp[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) rp[j] = smem + B64_OFF_MID + ((ib + j) & (B64_MID_ROWS - 1)) * B64_MID_ROW + lbase;
                multiply(rp);
                // epilogue: lane = output pixel (row oy, column x0 + fr; lanes 30, 31 belong to the next strip)
                u32x4 rr[2][2];
                unsigned ooff[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int oy = ys - 6 + 4 * k + 2 * wp + b, ox = x0 + fr;
                    const bool ok = oy >= ys && oy < ye && fr < BLOCK64_STRIP_W && ox < W;
                    ooff[b] = ok ? (unsigned)(((n * H + oy) * W + ox) * 128 + wc * 64 + fh * 16) : CONV_OOB;
                    const int i = ib + b;
                    const unsigned char* xr = smem + (((i >> 2) & 3) * B64_IN_GRP + (i & 3) * B64_IN_ROW) + lbase + 2 * B64_PITCH + wc * 64;
#pragma unroll
                    for (int q = 0; q < 2; ++q) rr[b][q] = *reinterpret_cast<const u32x4*>(xr + q * 32);
                }
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    half4 r4[4];
#pragma unroll
                    for (int q = 0; q < 2; ++q) epi_residual(rr[b][q], r4[2 * q], r4[2 * q + 1]);
                    half4 pk[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        floatx4 v;
                        epi_value<ACT2, 1>(v, 0, acc[b], g, lds_bias2, lds_slope2, wc * 32 + 8 * g + 4 * fh, r4[g]);
                        pk[g] = epi_half4(v);
                    }
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const u32x4 o = epi_chunk(pk[2 * q], pk[2 * q + 1]);
                        if (B64_ABL & 1) asm volatile("" ::"v"(o)); else
                        __builtin_amdgcn_raw_buffer_store_b128(o, orsrc, ooff[b] + 32 * q, 0, 0);   // couts 32 wc + 16 q + 8 fh .. + 7
                    }
                }
            }
        }
    }
    // nothing of this workgroup's DMA stream may still be in flight when its LDS is handed to the next workgroup
    wait_vmcnt<0>();
}

// ---------------------------------------------------------------------------------------------------------------- host side
// the two (activation, border bias) combinations the networks have on these blocks
int conv3x3_block64_variant(int act1, int flags1, bool slope1, int act2, int flags2) {
    if (flags2 != 0 || (flags1 & ~FRP_FLAG_BORDER_BIAS)) return 0;
    const bool border = (flags1 & FRP_FLAG_BORDER_BIAS) != 0;
    if (act1 == FRP_ACT_RELU && !border && act2 == FRP_ACT_RELU) return 1;                    // detector layer1
    if (act1 == FRP_ACT_PRELU && border && slope1 && act2 == FRP_ACT_NONE) return 2;           // IResNet block (folded pre-conv BN: 9 bias classes)
    return 0;
}

// What a launch on N maps of H x W looks like on n_cu compute units (<= 0: 256, a stand-alone call): strips of 30 columns, each cut into
// row segments (a multiple of the four rows of a step) so that the rounds of work items x the steps of an item are fewest - 32 x 272 x 480
// is 512 whole strips = two rounds of 70 steps; 320 x 56 x 56 gives 640 strips, halved: five rounds of 9 instead of three of 16.
// False: out of the kernel's reach (signed 32-bit byte offsets + slack).
bool conv3x3_block64_plan(int N, int H, int W, int n_cu, Block64Plan* g) {
    *g = Block64Plan{};
    if (N <= 0 || H <= 0 || W <= 0 || (long)N * H * W * 128 >= 0x7f000000L) return false;
    const int ncu = n_cu > 0 ? n_cu : 256;
    const int strips = (W + BLOCK64_STRIP_W - 1) / BLOCK64_STRIP_W;
    long best = -1;
    for (int want : {1, 2, 4, 8}) {
        const int rows = ((H + want - 1) / want + 3) / 4 * 4;
        if (want > 1 && rows < 8) break;
        const int segs = (H + rows - 1) / rows;
        const int steps = ((rows < H ? rows : H) + 2 + 3) / 4 + 1;
        const long items = (long)N * strips * segs, rounds = (items + ncu - 1) / ncu;
        if (items > 0x7fffffffL) continue;
        const long cost = rounds * steps;
        if (best < 0 || cost < best) {
            best = cost;
            g->strips = strips; g->segs = segs; g->seg_rows = rows; g->steps = steps; g->items = items;
            g->grid = (int)(items < ncu ? items : ncu);
            g->fill = (double)N * H * W / ((double)rounds * ncu * steps * (4.0 * BLOCK64_STRIP_W));
        }
    }
    g->lds = B64_LDS;
    return best >= 0;
}

// Where the fused launch pays: `fill` is the share of conv2's pixel slots (CUs x rounds x steps x 120) that are real output pixels - it
// falls with ragged strips (56 = 30 + 26), with the two steps an item spends filling and draining, and with a last round that does not
// occupy every CU.  The threshold is what tools/block64_probe.py measured.
bool conv3x3_block64_pays(const Block64Plan& g) {
    return g.items > 0 && g.fill >= BLOCK64_MIN_FILL;
}

template <int ACT1, bool BORDER1, int ACT2>
static hipError_t launch_block64_as(const Block64Params& p, int grid, hipStream_t stream) {
    static int attr_done[64] = {};
    int dev = 0, ncu = 0;
    hipError_t e = conv_device(&dev, &ncu);
    if (e != hipSuccess) return e;
    if (!attr_done[dev]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_block64_kernel<ACT1, BORDER1, ACT2>), hipFuncAttributeMaxDynamicSharedMemorySize, B64_LDS);
        if (e != hipSuccess) return e;
        attr_done[dev] = 1;
    }
    hipLaunchKernelGGL((conv3x3_block64_kernel<ACT1, BORDER1, ACT2>), dim3(grid), dim3(512), B64_LDS, stream, p);
    return hipGetLastError();
}

// One fused block.  p: tensors, shape, both layers' epilogues, n_cu (<= 0: the device's count is not known to the caller: 256);
// the plan fields are filled here.  hipErrorInvalidValue: no variant for these epilogues, or the shape is out of reach.
hipError_t launch_conv3x3_block64(const Block64Params& p0, hipStream_t stream) {
    Block64Params p = p0;
    Block64Plan g;
    if (!p.x || !p.w1 || !p.bias1 || !p.w2 || !p.bias2 || !p.out || p.x == p.out) return hipErrorInvalidValue;
    const int variant = conv3x3_block64_variant(p.act1, p.flags1, p.slope1 != nullptr, p.act2, 0);
    if (!variant || ((p.flags1 & FRP_FLAG_BORDER_BIAS) && (p.H < 2 || p.W < 2))) return hipErrorInvalidValue;
    if (!conv3x3_block64_plan(p.N, p.H, p.W, p.n_cu, &g)) return hipErrorInvalidValue;
    p.strips = g.strips; p.segs = g.segs; p.seg_rows = g.seg_rows;
    return variant == 1 ? launch_block64_as<FRP_ACT_RELU, false, FRP_ACT_RELU>(p, g.grid, stream)
                        : launch_block64_as<FRP_ACT_PRELU, true, FRP_ACT_NONE>(p, g.grid, stream);
}

}  // namespace frp
