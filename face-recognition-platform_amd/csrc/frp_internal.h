// Internal declarations shared by the HIP kernels and the C-ABI host code (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#define FRP_ACT_NONE 0
#define FRP_ACT_RELU 1
#define FRP_ACT_PRELU 2
#define FRP_FLAG_BORDER_BIAS 1
#define FRP_FLAG_OUT_F32 2
#define FRP_FLAG_RES_UP2 4
#define FRP_FLAG_FLATTEN 8
#define FRP_FLAG_F8 32          // conv on fp8 operands: input tensor and weights are OCP E4M3 bytes (blob: FRP_OPFLAG_FP8_MFMA)
#define FRP_FLAG_OUT_FP8 64     // the primary output is fp8 (value / out_scale); an fp8 COPY of an fp16 output goes to `out2`
#define FRP_CHIP_PIX (112 * 112)
#ifndef FRP_MAX_FACES_CAP
#define FRP_MAX_FACES_CAP 128
#endif

#include "jpeg_host.h"
#include "jpeg_selfsync.h"

namespace frp {

// The engine's environment switches (A/B runs, tests that pin a kernel family; unset: the default routing; "set": any value).  These
// comments are their record (INTEGRATION.md's table mirrors them); read_switches() / process_switches() (frp_api.cpp) their only readers.
// Per call: an entry point takes ONE snapshot and hands it down; run_net keys captured graphs by all of its bytes, so a field added here
// can never replay a graph recorded under another value.
struct Switches {
    int small_m;          // FRP_SMALL_M: tile class of the conv launches (conv_common.h: conv_small_m); unset: by each launch's tile count,
                          // "0...": never quarter tiles (-1), any other value: always (1)
    int s2;               // FRP_S2 set: the opt-in stride-2 row-patch kernel (conv3x3_s2.hip, CONV_DBG_S2)
    int no_fused_stem12;  // FRP_NO_FUSED_STEM12 set: the detector's two stems as two launches (stem1 with the u8 normalisation, stem2 generic)
    int no_fused_stem;    // FRP_NO_FUSED_STEM set: the detector input as preprocess + generic conv, not the u8 stem kernel(s)
    int no_emb_stem;      // FRP_NO_EMB_STEM set: the embedder's stem on the generic kernel, not its dedicated one
    int no_stem_fuse;     // FRP_NO_STEM_FUSE set: the embedder's stem and the 64 -> 64 conv behind it as two launches
    int wino_min_faces;   // FRP_WINO_MIN_FACES=n (default 128): the embedder's Winograd family for calls of at least n slots (run_embed)
    int host_count;       // FRP_HOST_COUNT set: threshold mode copies the face count to the host before the embedder (run_faces)
    int match_v1;         // FRP_MATCH_V1 set: the per-tile matcher only, never the persistent top-1 kernel (also a host-side count)
    int no_wino;          // FRP_NO_WINO set, read at weight load: no Winograd weight images, direct kernels only
    int no_kconcat;       // FRP_NO_KCONCAT set, read at weight load: no 1x1 shortcut conv folded into its consumer's k-loop
    int no_block_fuse;    // FRP_NO_BLOCK_FUSE set: a 64 -> 64 residual block as its two conv launches, never the fused one (conv3x3_block64.hip)
    int block_fuse_all;   // FRP_BLOCK_FUSE_ALL set: the fused block launch on every eligible shape, also where it does not pay (tests on small maps)
};
static_assert(std::has_unique_object_representations_v<Switches>, "run_net keys captured graphs by the bytes of a Switches");
Switches read_switches();

// Read once per process, at the first call that needs one of them.
struct ProcessSwitches {
    bool no_graph;             // FRP_NO_GRAPH set: every network pass launch by launch, never replayed from a captured hipGraph (run_net)
    bool c64_all;              // FRP_C64_ALL set: the 64 -> 64 kernel on every eligible shape (CONV_DBG_C64_ALL), also where it does not pay
    int jpeg_device_huffman;   // FRP_JPEG_DEVICE_HUFFMAN: entropy decode of restart-interval JPEGs on the device; unset (0): for intervals of
                               // at most 32 MCUs, "0..." (-1): never, any other value (1): always (ingest_api.cpp: candidate_route)
    bool jpeg_selfsync;        // FRP_JPEG_SELFSYNC set and not "0...": new handles decode JPEG batches without restart markers on the device
                               // (the self-synchronising decoder; frp_set_jpeg_selfsync changes it per handle)
};
const ProcessSwitches& process_switches();

struct ConvParams {
    const _Float16* x;      // [N,H,W,Cin]
    const _Float16* w;      // [Cout][KS][KS][Cin]
    const float* bias;      // [Cout] or [9][Cout] (FRP_FLAG_BORDER_BIAS)
    const float* slope;     // [Cout] (PReLU) or null
    const _Float16* res;    // [N,Ho,Wo,Cout] (or [N,Hr,Wr,Cout] with FRP_FLAG_RES_UP2) or null
    void* out;              // [N,Ho,Wo,Cout] fp16 (fp32 with FRP_FLAG_OUT_F32, fp8 with FRP_FLAG_OUT_FP8)
    void* out2;             // optional fp8 copy of an fp16 output (value / out_scale), or null
    const _Float16* x2;     // K-concat (generic kernel, 3x3, Cin % 64 == 0): a second K segment = the 1x1 conv of tensor x2 [N,H,W,Cin2]
                            // at the CENTRE tap's position (the block's stride-2 shortcut folded into its second conv);
                            // w rows are then [3][3][Cin] followed by [Cin2], bias the sum of both.  null = none
    int Cin2;               // channels of x2 (Cin2 % 64 == 0, Cin == Cin2 or 2 * Cin2)
    const float* wscale;    // FRP_FLAG_F8: per-cout scale of the fp8 weights
    float in_scale;         // FRP_FLAG_F8: the fp8 input tensor holds value / in_scale
    float out_scale;        // fp8 outputs hold value / out_scale
    int N, H, W, Cin, Cout, KS, stride;
    int act, flags;
    int Hr, Wr;             // residual spatial dims (RES_UP2)
    int ksplit;             // >1: split-K, `out` = fp32 workspace [ksplit][M][Cout] of raw partial sums;
                            // -1 (only with n_dev): the kernel picks conv_pick_ksplit(M) itself
    const _Float16* wino_w; // null, or the Winograd weight image of this layer (conv3x3_wino.hip; built by net_program.cpp:build_wino_image):
                            // launch_conv() takes the Winograd kernel when the shape is eligible
    const int32_t* n_dev;   // null, or the number of images that really exist (<= N) in device memory: the kernel derives
                            // M and its tile count from it (threshold mode: the face count never visits the host mid-pipeline)
    int n_cu;               // compute units (input of the device-side split-K choice)
    unsigned long long* stamps;   // conv_bench diagnostics: [grid][8] 100 MHz phase stamps, or null
    int dbg;                // kernel A/B bits (CONV_DBG_* below); 0 = the launcher's own choice
    int wino_wide_only;     // the Winograd kernel only in its 2-D tile form (maps wider than its flattened tiles cover) and only where the
                            // tile arithmetic says it pays (conv3x3_wino.hip: wino_2d_pays) - the detector's layers
    const void* pf_ptr;     // quarter-tile launches with CUs to spare: the NEXT launch's weights (pf_bytes of them), read once by 64 extra
    unsigned pf_bytes;      // workgroups - 8 per XCD - while this launch runs, so that the next one streams them from L2 (a call of a few
    int n_workers;          // faces reads every weight once, cold: its k-steps wait for HBM); n_workers: set by the launcher (0 = the whole grid works)
    int small_m;            // quarter tiles (128 pixels x 64 couts, two workgroups per CU): 0 = when the default tiling leaves half
                            // of the CUs idle (conv_common.h: conv_small_m), 1 = always, -1 = never (tests, A/B runs)
    // fused embedder stem (conv3x3_c64.hip, round 5): this launch is the 3x3 64 -> 64 conv that FOLLOWS the stem - the kernel computes the
    // stem (3x3, 3 real of 8 channels -> 64, + bias + PReLU) of every patch pixel itself, from the chips, and feeds its MFMAs from LDS: the
    // 64-channel map is written (for the block's shortcut) but never read back.  `x` is then only the tensor that WOULD have been read.
    const _Float16* stem_x;     // chips [N,H,W,8] fp16 (R,G,B,0..), or null = no fusion
    const _Float16* stem_w;     // folded stem weights [64][3][3][8]
    const float* stem_bias;     // [64]
    const float* stem_slope;    // [64]
    _Float16* stem_out;         // [N,H,W,64]: the stem's output, written by this launch
    int stem_even_only;         // only the pixels (even y, even x) of stem_out are written: its one reader is a 1x1 stride-2 conv (the block's
                                // shortcut, riding in a later k-loop) - a quarter of the map's bytes
    // derived by conv_derive() (conv_launch.cpp):
    int pad, Ho, Wo, M, Ktot, nk, cin_shift, n_ptiles, n_ctiles;
    unsigned x_bytes, w_bytes, x2_bytes;   // buffer-descriptor sizes (each < 2 GiB)
    int x2_shift;           // log2(Cin / Cin2)
};

// ConvParams::dbg: kernel A/B bits for parity tests, conv_bench and A/B runs.  frp_conv2d_nhwc / frp_conv_bench take them from their
// `flags` (include/frp.h; kernel_api.cpp: conv_route_from_abi_flags), the engine's passes from its switches (Switches, ProcessSwitches).
constexpr int CONV_DBG_GENERIC = 1;               // the generic kernel also for shapes a specialised one covers
constexpr int CONV_DBG_WINO_2D = 256;             // lab: the Winograd kernel's 2-D tiles whatever the shape
constexpr int CONV_DBG_NO_C64 = 512;              // not the 64 -> 64 kernel (conv3x3_c64.hip): the row-patch one, bit-identical
constexpr int CONV_DBG_C64_ALL = 1024;            // the 64 -> 64 kernel on every eligible shape, also where it does not pay
constexpr int CONV_DBG_S2 = 2048;                 // the opt-in stride-2 row-patch kernel (conv3x3_s2.hip)
constexpr int CONV_DBG_C64_SAME_ORDER = 4096;     // the 64 -> 64 kernel with all waves in the same order (A/B of its ping-pong)
// bits 1..7 mean something else to each kernel family
constexpr int CONV_DBG_LEAN_ALL_ROWS = 64;        // conv3x3_lean.hip: head outputs (Cout <= 32) on all 64 rows of the tile
constexpr int CONV_DBG_LEAN_TILE256 = 128;        // conv3x3_lean.hip: the 256-pixel tile for 64 couts (1.5 reads per MFMA)
constexpr int CONV_DBG_WINO_ABLATION = 15 << 1;   // lab, conv3x3_wino.hip: number of a timing ablation (tools/wino_ablate.py)
constexpr int CONV_DBG_WINO_ONE_WAVE = 32;        // lab, conv3x3_wino.hip: one wave per SIMD
constexpr int CONV_DBG_WINO_ROW_PATCH = 64;       // lab, conv3x3_wino.hip: the first generation's row-patch form (also wide maps)
constexpr int CONV_DBG_WINO_KLOOP_GEN1 = 128;     // lab, conv3x3_wino.hip: the first generation of the k-loop (compiler-scheduled)
constexpr int CONV_DBG_ROWS_PRE_PREFETCH = 2;     // lab, conv3x3_rows.hip: the pre-prefetch k-step (bit-identical)
constexpr int CONV_DBG_ROWS_ABLATION = 15 << 2;   // lab, conv3x3_rows.hip: number of a timing ablation of the 128-cout kernel (wrong results)
constexpr int CONV_DBG_ROWS_GEN1 = 64;            // lab, conv3x3_rows.hip: the first-generation kernel with the cross-barrier prefetch
constexpr int CONV_DBG_ROUTING = CONV_DBG_GENERIC | CONV_DBG_WINO_2D | CONV_DBG_NO_C64 | CONV_DBG_C64_ALL | CONV_DBG_S2 | CONV_DBG_C64_SAME_ORDER;
template <class... B> constexpr bool conv_dbg_disjoint(B... b) { return (b + ...) == (b | ...); }   // no bit set in two of them
static_assert(conv_dbg_disjoint(CONV_DBG_GENERIC, CONV_DBG_WINO_2D, CONV_DBG_NO_C64, CONV_DBG_C64_ALL, CONV_DBG_S2, CONV_DBG_C64_SAME_ORDER) &&
              conv_dbg_disjoint(CONV_DBG_ROUTING, CONV_DBG_LEAN_ALL_ROWS, CONV_DBG_LEAN_TILE256) &&
              conv_dbg_disjoint(CONV_DBG_ROUTING, CONV_DBG_WINO_ABLATION, CONV_DBG_WINO_ONE_WAVE, CONV_DBG_WINO_ROW_PATCH, CONV_DBG_WINO_KLOOP_GEN1) &&
              conv_dbg_disjoint(CONV_DBG_ROUTING, CONV_DBG_ROWS_PRE_PREFETCH, CONV_DBG_ROWS_ABLATION, CONV_DBG_ROWS_GEN1),
              "the dbg bits one kernel family reads must be disjoint");
constexpr int conv_dbg_field(int dbg, int field) { return (dbg & field) / (field & -field); }   // the number a multi-bit field holds

// One conv launch (conv_launch.cpp): conv_derive checks the arguments and fills the derived fields, conv_pick chooses the kernel
// family - a pure function: the routing of a layer without a GPU -, launch_conv is derive, pick, the family's launcher.
enum class ConvFamily { Wino, S2, C64, RowPatch, Generic, Invalid };
struct C64Plan {            // conv3x3_c64.hip: what a launch on a map looks like
    int variant;            // the kernel's (activation, residual, border bias) combination, 0: none of them
    int tile_w;             // 32 (x 8 rows) or 16 (x 16)
    long tiles;
    double fill;            // share of real pixels in the tiles
};
struct ConvRoute {
    ConvFamily family;
    bool few;               // Generic, RowPatch: quarter tiles (conv_common.h: conv_small_m on the family's default tile count)
    int wino_form;          // Wino: 1 flattened tiles, 2 the 2-D tiles
    C64Plan c64;            // C64
};
hipError_t conv_derive(ConvParams& p, int* ncu);
ConvRoute conv_pick(const ConvParams& p, int ncu);
hipError_t launch_conv(const ConvParams& p, hipStream_t stream);
// The families' predicates and launchers: `p` carries conv_derive()'s fields, and a launcher gets what conv_pick() found eligible.
hipError_t launch_conv_generic(const ConvParams& p, bool few, hipStream_t stream);   // conv_mfma.hip: every shape
// row-patch kernel for 3x3 stride-1 layers with Cin % 64 == 0 (conv3x3_lean.hip: static k-loop generation)
bool conv3x3_rows_eligible(const ConvParams& p);
long conv3x3_lean_default_tiles(const ConvParams& p);
#ifdef FRP_LAB
hipError_t launch_conv3x3_rows(const ConvParams& p, bool few, hipStream_t stream);   // first generation + ablations (conv3x3_rows.hip; lab build only)
#endif
hipError_t launch_conv3x3_lean(const ConvParams& p, bool few, hipStream_t stream);
// 3x3 stride-1 64 -> 64 layers on large maps (conv3x3_c64.hip): weights resident in registers, 2-D pixel tiles, one barrier per tile
bool conv3x3_c64_eligible(const ConvParams& p, C64Plan* plan);
bool conv3x3_c64_fuses_stem(int N, int H, int W, int n_cu);   // maps on which the kernel takes the embedder's stem into the launch of the conv behind it
hipError_t launch_conv3x3_c64(const ConvParams& p, const C64Plan& plan, hipStream_t stream);
// A residual block of two 3x3 stride-1 64 -> 64 convs in one launch (conv3x3_block64.hip): out = act2(conv2(act1(conv1(x))) + x), the
// intermediate tensor in LDS only.  Not a family of launch_conv: net_program.cpp's walk launches a marked pair of ops through it.
#define BLOCK64_STRIP_W 30          // output columns of a strip: the intermediate row (+ 2 halo columns) is one 32-pixel MFMA block
#define BLOCK64_IN_W 34             // input columns under a strip
#define BLOCK64_LDS_BYTES 159232    // input ring 4 x 20 KiB, intermediate ring 16 rows x 4608 B (+ 512), epilogue parameters 3 KiB
#define BLOCK64_MIN_FILL 0.70       // conv3x3_block64_pays: least share of real output pixels in the launch's pixel slots
struct Block64Params {
    const _Float16* x;      // [N,H,W,64]: conv1's input and the block's residual
    const _Float16* w1;     // [64][3][3][64]
    const float* bias1;     // [64] or [9][64] (flags1 & FRP_FLAG_BORDER_BIAS)
    const float* slope1;    // [64] (PReLU) or null
    const _Float16* w2;
    const float* bias2;     // [64]
    const float* slope2;    // [64] or null
    void* out;              // [N,H,W,64] fp16, not x
    const int32_t* n_dev;   // null, or the number of images that really exist (<= N) in device memory
    int N, H, W;
    int act1, flags1, act2;
    int n_cu;               // compute units the plan is made for (<= 0: 256)
    int strips, segs, seg_rows;   // filled by the launcher from conv3x3_block64_plan()
};
struct Block64Plan {
    int strips, segs, seg_rows;   // per image: strips of 30 columns x segments of seg_rows rows (a multiple of 4; the last may be shorter)
    int steps;                    // steps of the longest work item
    long items;                   // work items: N x strips x segs
    int grid, lds;
    double fill;                  // real output pixels / (rounds x CUs x steps x 120 pixel slots)
};
// work item `item` of a launch: image n, output rows ys .. ye - 1, output columns x0 .. x0 + 29 (clipped to the map), K conv1 steps
// (the item takes K + 1 steps).  Host and device evaluate the same function (the kernel; tests/native/block64_plan_harness.cpp).
struct Block64Item { int n, ys, ye, x0, K; };
__host__ __device__ inline Block64Item block64_item(int item, int strips, int segs, int seg_rows, int H) {
    Block64Item it;
    const int per_img = strips * segs;
    it.n = item / per_img;
    const int r = item - it.n * per_img, seg = r / strips;
    it.ys = seg * seg_rows;
    it.ye = it.ys + seg_rows < H ? it.ys + seg_rows : H;
    it.x0 = (r - seg * strips) * BLOCK64_STRIP_W;
    it.K = (it.ye - it.ys + 2 + 3) >> 2;
    return it;
}
// the input rows an item fetches (groups of four from two rows above its first output row: its groups 1 .. K + 1) and its input columns
// (34 from two columns left of its first output column): the halo the plan declares - at most BLOCK64_HALO_DOWN rows below the segment
#define BLOCK64_HALO_UP 2
#define BLOCK64_HALO_DOWN 7
__host__ __device__ inline int block64_first_in_row(const Block64Item& it) { return it.ys - 6 + 4; }
__host__ __device__ inline int block64_last_in_row(const Block64Item& it) { return it.ys - 6 + 4 * (it.K + 1) + 3; }
int conv3x3_block64_variant(int act1, int flags1, bool slope1, int act2, int flags2);   // 0: none, 1: detector (ReLU, ReLU), 2: embedder (PReLU + border classes, none)
bool conv3x3_block64_plan(int N, int H, int W, int n_cu, Block64Plan* plan);             // false: out of 32-bit reach
bool conv3x3_block64_pays(const Block64Plan& plan);
hipError_t launch_conv3x3_block64(const Block64Params& p, hipStream_t stream);
// 3x3 stride-2 layers (conv3x3_s2.hip): row patches whose left / right neighbour entries are shared by consecutive output pixels
bool conv3x3_s2_eligible(const ConvParams& p);
hipError_t launch_conv3x3_s2(const ConvParams& p, hipStream_t stream);
// Winograd F(2,3) along the image rows (conv3x3_wino.hip): the form in which it takes a launch (0: not), eligibility from the static
// layer geometry, the size of a layer's weight image, the launch (p.w = the image)
int conv3x3_wino_form(const ConvParams& p);
bool conv3x3_wino_shape_ok(int W, int Cin, int ksize, int stride);
bool conv3x3_wino_call_ok(int N, int H, int W, int Cin, int Cout, int ksize, int stride, int n_cu, bool has_res, int dbg);   // stand-alone calls: shape_ok, wide_pays or forced by dbg
bool conv3x3_wino_wide_pays(int N, int H, int W, int Cin, int Cout, int n_cu, bool has_res);   // maps wider than 30: the 2-D tile form, where its tile arithmetic pays
#ifdef FRP_LAB
bool conv3x3_wino_lab_shape_ok(int W, int Cin, int ksize, int stride);   // + the maps only the lab's row-patch form covers (CONV_DBG_WINO_ROW_PATCH)
#endif
size_t conv3x3_wino_image_bytes(int Cin, int Cout);
hipError_t launch_conv3x3_wino(const ConvParams& p, int form, hipStream_t stream);

// K1: u8 BGR frames -> normalised fp16 NHWC8 canvas (top-left letterbox, zero u8 pad)
hipError_t launch_preprocess(const uint8_t* bgr, int B, int H, int W, long row_stride, long frame_stride,
                             _Float16* out, int Hc, int Wc, int rgb_in, hipStream_t stream);

// K1+K2 fused detector stem: u8 frames -> conv3x3 s2 (3->32) + bias + ReLU, fp16 NHWC
struct StemParams {
    const uint8_t* frames;   // [B,H,W,3] u8
    int B, H, W;
    long row_stride, frame_stride;
    int Hc, Wc;              // letterbox canvas (multiples of 32)
    int Ho, Wo;              // Hc/2, Wc/2
    int rgb_in;
    const _Float16* w;       // folded [32][3][3][8] fp16 (channels R,G,B,0..)
    const float* bias;       // [32]
    _Float16* out;           // [B,Ho,Wo,32]
};
hipError_t launch_stem_u8(const StemParams& p, hipStream_t stream);

// K1+K2+K2 fused detector stems: u8 frames -> conv3x3 s2 (3->32) + ReLU -> conv3x3 s2 (32->64) + ReLU
struct Stem12Params {
    const uint8_t* frames;   // [B,H,W,3] u8
    int B, H, W;
    long row_stride, frame_stride;
    int Hc, Wc;              // letterbox canvas (multiples of 32)
    int Ho1, Wo1;            // stem1 map: Hc/2, Wc/2
    int Ho2, Wo2;            // stem2 map: Hc/4, Wc/4
    int rgb_in;
    const _Float16* w1;      // folded [32][3][3][8] fp16 (channels R,G,B,0..)
    const float* bias1;      // [32]
    const _Float16* w2;      // folded [64][3][3][32] fp16
    const float* bias2;      // [64]
    _Float16* out;           // [B,Ho2,Wo2,64]
};
hipError_t launch_stem12_u8(const Stem12Params& p, hipStream_t stream);

// embedder stem: chips fp16 NHWC8 (3 real channels) -> conv3x3 s1 (3 -> 64) + bias + PReLU, fp16 NHWC64
struct EmbStemParams {
    const _Float16* x;       // [M,H,W,8]
    int M, H, W;
    const _Float16* w;       // folded [64][3][3][8] fp16 (channels R,G,B,0..)
    const float* bias;       // [64]
    const float* slope;      // [64]
    _Float16* out;           // [M,H,W,64]
    const int32_t* n_dev;    // null, or the number of chips that really exist (<= M), read on the device
};
hipError_t launch_emb_stem(const EmbStemParams& p, hipStream_t stream);

// K3: decode + candidate select + sort + NMS, one workgroup per frame
struct DecodeParams {
    const _Float16* head[3];   // per stride [B, H_l, W_l, 32]
    int hl[3], wl[3];
    int B, max_faces;
    float logit_thresh, nms_iou;
    float* boxes;     // [B, max_faces, 4]
    float* kps;       // [B, max_faces, 10]
    float* scores;    // [B, max_faces]
    int32_t* anchor;  // [B, max_faces]
    int32_t* counts;  // [B]
    _Float16* logits; // scratch [B, anchors]: dense copy of the anchor logits
};
hipError_t launch_decode_nms(const DecodeParams& p, hipStream_t stream);

// K3b: cross-scale merge + NMS of the detection pyramid (pyramid_kernels.hip), one workgroup per frame: the detections K3 wrote per
// scale, scale-major, -> K = max_faces slots per frame in frame pixels, bit for bit pyramid.merge_scales
#define FRP_PYRAMID_MAX_SCALES 4
#define FRP_PYRAMID_MAX_CAND 512   // S * P candidates per frame at the most: one thread and one sort slot each
struct PyramidMergeParams {
    const float* boxes;       // [S][B][P][4] in the coordinates of scale s's resized image
    const float* kps;         // [S][B][P][10]
    const float* scores;      // [S][B][P] finite, >= 0
    const int32_t* counts;    // [S][B], each in [0, P]
    int S, B, P, max_faces;
    int frame_h, frame_w;
    int det_h[FRP_PYRAMID_MAX_SCALES], det_w[FRP_PYRAMID_MAX_SCALES];   // size of scale s's resized image
    float nms_iou;
    float* out_boxes;         // [B, max_faces, 4] frame pixels; slots from the count on are zero
    float* out_kps;           // [B, max_faces, 10]
    float* out_scores;        // [B, max_faces]
    int32_t* out_anchor;      // [B, max_faces] or null: -1 in every slot
    int32_t* out_counts;      // [B]
    // derived by launch_pyramid_merge():
    float rx[FRP_PYRAMID_MAX_SCALES], ry[FRP_PYRAMID_MAX_SCALES];       // (float)frame_w / (float)det_w[s], (float)frame_h / (float)det_h[s]
};
// refuses (hipErrorInvalidValue) S outside 1..4, P or max_faces outside 1..FRP_MAX_FACES_CAP, S * P > FRP_PYRAMID_MAX_CAND
hipError_t launch_pyramid_merge(PyramidMergeParams p, hipStream_t stream);

// JPEG ingest, device half (jpeg_kernels.hip): quantised coefficients -> BGR frames
struct JpegParams {
    const int16_t* coef;     // [B][blocks_per_image][64], natural order, quantised; per image the components back to back
    const uint16_t* qtab;    // [B][3][64]
    uint8_t* planes;         // scratch: per image the sample planes of the components ([by * 8][bx * 8] u8 each)
    uint8_t* frames;         // out: [B, H, W, 3] u8 BGR
    int B, W, H, components;
    int bx[3], by[3];        // blocks per row / column of each component (whole MCUs)
    int blocks_per_image;
    long plane_off[3], plane_img;   // byte offsets of the component planes inside an image's scratch, bytes per image (multiples of 8)
    int hs, vs;              // luma sampling factors (chroma 1 x 1)
    int cw, ch;              // real extent of the chroma planes: ceil(W / hs), ceil(H / vs)
};
hipError_t launch_jpeg_decode(const JpegParams& p, hipStream_t stream);

// YUV 4:2:0 ingest (yuv_kernels.hip; frp.h: frp_upload_yuv): decoder surfaces -> BGR frames.  The constants of one matrix, see the kernel file:
// y = max(0, Y - yoff) * cy, R = clamp((y + cvr * v + rnd) >> sh), G = clamp((y - cvg * v - cug * u + rnd) >> sh), B = clamp((y + cub * u + rnd) >> sh)
struct YuvCoef { int yoff, cy, cvr, cvg, cug, cub, rnd, sh; };
struct YuvParams {
    const uint8_t* const* tab;   // [B][3] device addresses per frame: Y, U (semi-planar: the interleaved plane), V (semi-planar: unused)
    uint8_t* frames;             // out: [B, H, W, 3] u8 BGR
    int B, W, H;                 // W, H even
    int64_t y_pitch, c_pitch;    // bytes per row of the Y plane / of each chroma plane
    int ush;                     // semi-planar: 0 - U is the first byte of a pair (NV12), 8 - V is (NV21)
    YuvCoef k;
};
hipError_t launch_yuv_to_bgr(const YuvParams& p, bool semi_planar, bool fast, hipStream_t stream);

// Entropy decoding ON THE DEVICE for streams with restart intervals (round 5): the DC predictors reset at every RSTn marker, so the
// intervals of a scan are independent bit streams - one thread each (jpeg_kernels.hip: jpeg_huffman_kernel).  Canonical Huffman
// tables: jpeg_entropy.h: JpegHuffTableDev.
struct JpegHuffParams {
    const uint8_t* scan;             // the entropy-coded segments of all images, back to back
    const uint32_t* int_off;         // [B][n_int + 1]: byte offset (into `scan`) of every interval's first byte; [n_int] = one past the image's data
    const JpegHuffTableDev* tables;  // [B][6]: component c's DC table at 2c, its AC table at 2c + 1
    int16_t* coef;                   // out: [B][coef_per_image], natural order (zeroed before the launch)
    int32_t* err;                    // out: [B], non-zero = the image's bit stream is corrupt / ends early
    long coef_per_image;
    int B, n_int, ri;                // intervals per image, MCUs per interval
    int mcus_y;
    JssGeom g;                       // (jpeg_selfsync.h: jss_geom; the kernel reads components, mcus_x, hs, vs, bx, comp_off)
};
hipError_t launch_jpeg_huffman(const JpegHuffParams& p, hipStream_t stream);

// Entropy decoding ON THE DEVICE for streams WITHOUT restart markers: the self-synchronising decoder (jpeg_selfsync.h has the algorithm and
// the per-thread routines, jpeg_selfsync.hip the kernels).  One thread per subsequence of S raw bytes, JSS_WG subsequences per workgroup;
// per image n_sub = ceil(scan bytes / S) subsequences, numbered from sub0 (a multiple of JSS_WG) in the state arrays.
struct JpegSelfsyncParams {
    const uint8_t* scan;             // the scans of all images, each at an offset that is a multiple of 16
    const uint32_t* img;             // [B][4]: byte offset of the scan, its bytes, n_sub, sub0
    const JpegHuffTableDev* tables;  // [B][6]: component c's DC table at 2c, its AC table at 2c + 1
    JssState* entry;                 // [N] entry state of every subsequence (N = all images' subsequences, each image rounded up to JSS_WG)
    JssState* exit_;                 // [N] ... its exit state
    JssState* wgx;                   // [2][N / JSS_WG] exit of every workgroup's last subsequence: launch k reads half k & 1, writes the other
    uint32_t* cnt;                   // [N] blocks completed
    uint32_t* base;                  // [N] blocks completed by the subsequences before it = its first block
    int32_t* rounds;                 // [B] most rounds with a change among the image's workgroups in this launch (zeroed before it)
    int32_t* stats;                  // [B][4]: subsequences, -, blocks counted (at most the total), error flag (zeroed before the first launch)
    int16_t* coef;                   // out: [B][coef_per_image], natural order (zeroed before the launch)
    long coef_per_image;
    int B, S;
    uint32_t max_sub;                // largest n_sub of the batch
    uint32_t n_wg_all;               // N / JSS_WG
    JssGeom g;
};
// launch k of the synchronisation (k = 0: speculate from the guessed states); the caller repeats it until a launch reports no round
hipError_t launch_jpeg_selfsync_round(const JpegSelfsyncParams& p, int k, hipStream_t stream);
// at the fix-point: block prefix sums, coefficients (DC differences), DC running sums
hipError_t launch_jpeg_selfsync_finish(const JpegSelfsyncParams& p, hipStream_t stream);

// diagnostic (frp_debug_det_hashes): order-independent 64-bit hash of a tensor's 16-byte words, added to *slot (aux_kernels.hip)
hipError_t launch_tensor_hash(const void* src, size_t bytes, unsigned long long* slot, hipStream_t stream);
// u8 bilinear resize for the detection pyramid (pyramid_kernels.hip; frames [B,H,W,3] tightly packed)
hipError_t launch_resize_u8(const uint8_t* src, int B, int H, int W, uint8_t* dst, int Hs, int Ws, hipStream_t stream);

// K4: 5-point similarity + bilinear warp to 112x112 -> normalised fp16 NHWC8 chips
struct AlignParams {
    const uint8_t* frames;  // [B,H,W,3] u8 BGR
    int B, H, W;
    long row_stride, frame_stride;
    const float* kps;       // [B, max_faces, 10]
    const int32_t* counts;  // [B]
    int max_faces;
    const int32_t* face_slot;  // [n_faces] -> b*max_faces + k   (compacted face list)
    int n_faces;
    int rgb_in;             // frames are RGB instead of BGR
    _Float16* chips;        // [n_faces,112,112,8]
    const int32_t* n_dev;   // null, or the real face count (<= n_faces, which then is the capacity), read on the device
};
hipError_t launch_align(const AlignParams& p, hipStream_t stream);
// raw aligned u8 chips (BGR [M,112,112,3]) -> normalised fp16 NHWC8
hipError_t launch_chips_to_blob(const uint8_t* chips, int M, _Float16* out, hipStream_t stream);
// build the compact face list from counts (device side)
hipError_t launch_compact_faces(const int32_t* counts, int B, int max_faces, int32_t* face_slot, int32_t* n_faces,
                                hipStream_t stream);

// Face tracks (track_kernels.hip; frp.h: frp_track_config): which detections of a pass belong to a face identified before, the embed
// list of the others, and the cached results of the rest.  Per stream two table halves of FRP_TRACK_SLOTS entries: a pass reads the
// half `cur` of the stream's header and writes the other one.
#define FRP_TRACK_SLOTS 128
struct alignas(16) TrackEntry {            // one row of a table half (48 bytes)
    float box[4];
    int32_t id, age, missed;
    int32_t match_idx;
    float match_cos;
    int32_t src;               // of the pass that wrote the row: where its emb / match_idx / match_cos come from (a slot's `src` below)
    int32_t pad[2];
};
static_assert(sizeof(TrackEntry) == 48, "three 16-byte words");
struct TrackHeader { int32_t next_id, n, cur, pad; };      // per stream: the next new id, rows of the current half, which half that is
struct TrackPlan { int32_t old_half, n_new; };             // per stream, written by the associate launch of a pass for its store launch
struct TrackParams {
    // configuration and state
    int max_streams;
    float iou_min;
    int refresh, max_missed, stale;
    TrackHeader* hdr;          // [max_streams]
    TrackEntry* meta;          // [max_streams][2][FRP_TRACK_SLOTS]
    float* tab_emb;            // [max_streams][2][FRP_TRACK_SLOTS][512]
    TrackPlan* plan;           // [max_streams]
    int64_t* totals;           // [2]: embedded, reused
    // the pass: B frames of K slots, stream per frame, the streams that occur (each once)
    int B, K;
    const int32_t* streams;    // [B], -1: an untracked frame
    const int32_t* present;    // [n_present]
    int n_present;
    const float* boxes;        // [B][K][4]
    const int32_t* counts;     // [B]
    // per slot [B][K].  src >= 0: the slot of this batch whose embedding it carries (its own: an embedded slot); src < 0, not
    // FRP_TRACK_DEAD: row -1 - src of the stream's old half; FRP_TRACK_DEAD: a slot at or beyond counts[b]
    int32_t *track_id, *reused, *age, *src;
    int32_t* pos;              // compact position of an embedded slot, -1 otherwise
    int32_t *face_slot, *nfaces;
    // compact results of the embedded faces (best_idx / best_cos null: the pass did not match) and the per-slot results
    const float* emb;          // [n][512]
    const int32_t* best_idx;
    const float* best_cos;
    float* slot_emb;           // [B][K][512]
    int32_t* slot_idx;
    float* slot_cos;
};
#define FRP_TRACK_DEAD INT32_MIN
hipError_t launch_track_associate(const TrackParams& p, hipStream_t stream);      // + the compact launch behind it
hipError_t launch_track_resolve(const TrackParams& p, hipStream_t stream);        // + the table store behind it

// K5 tail: row-wise L2 normalisation of [M,512] fp32 (in place) + fp16 copy for the matcher.
// With `partials` (split-K FC): emb[m][c] = sum_s partials[s][m][c] + bias[c] first.
// `n_dev` (optional): the real row count lives in device memory (M is then the capacity); with ksplit == -1 the split
// factor of the FC that wrote `partials` is re-derived from it (conv_pick_ksplit with fc_ktot, n_cu).
hipError_t launch_l2norm(float* emb, _Float16* emb16, int M, int D, hipStream_t stream,
                         const float* partials = nullptr, int ksplit = 0, const float* bias = nullptr,
                         const int32_t* n_dev = nullptr, int fc_ktot = 0, int n_cu = 0);
// Split-K factor for a skinny GEMM-shaped conv (the 25088 -> 512 FC: 8 output tiles but 392 k-steps): the largest divisor
// of nk that keeps >= 8 k-steps per slice and does not exceed the CU count in (tile, slice) pairs.  1 = no split.
// Host and device evaluate the same function (device: when the image count is only known there).
__host__ __device__ inline int conv_pick_ksplit(int M, int Cout, int Ktot, int flags, bool has_res, int n_cu) {
    if (!(flags & FRP_FLAG_OUT_F32) || has_res || (Ktot & 63) || M <= 0) return 1;
    const int nk = Ktot / 64;
    const long tiles = (long)((M + 255) / 256) * ((Cout + 127) / 128);
    if (tiles * 4 > n_cu || nk < 64) return 1;
    int best = 1;
    for (int s = 2; s <= nk / 8; ++s)
        if (nk % s == 0 && tiles * s <= n_cu) best = s;
    return best;
}
// gallery upload: fp32 rows -> unit fp16 rows
hipError_t launch_gallery_normalize(const float* in, _Float16* out, long N, int D, hipStream_t stream);
// exact compat rows (frp.h: frp_gallery_exact): unit fp16 rows widened to float64; Euclidean distances of M float64 queries to the
// N float64 rows, out[m * N + row] (face_recognition.face_distance, face_service.py:410,465,599)
hipError_t launch_gallery_widen(const _Float16* in, double* out, long N, int D, hipStream_t stream);
hipError_t launch_gallery_distances(const double* rows, long N, const double* q, int M, double* out, hipStream_t stream);

// Face quality (quality_kernels.hip; frp.h: frp_face_quality): per rectangle of the resident u8 frames the four integer sums behind
// FaceService.assess_face_quality's blur and lighting scores - S1 = sum g, S2 = sum g^2, L1 = sum lap, L2 = sum lap^2 over the crop,
// g the cv2 fixed-point grey value, lap the 5-point Laplacian of g with BORDER_REFLECT_101 at the edges of the CROP.
// One workgroup per QUALITY_TILE_H x QUALITY_TILE_W tile of a crop (mirrored in native.py: the tests size their crops from them).
#define QUALITY_TILE_H 32
#define QUALITY_TILE_W 64
struct QualityParams {
    const uint8_t* frames;        // [B,H,W,3] u8, tightly packed, 4-byte aligned base
    long long total_bytes;        // B*H*W*3: no byte at or beyond it is read
    int B, H, W;
    int rgb_in;                   // frames are RGB instead of BGR
    const int32_t* rects;         // [n][5]: frame, top, right, bottom, left (validated by the caller: inside the frame, not empty)
    const int32_t* tile_prefix;   // [n + 1]: tiles of the rectangles before r; [n] = n_tiles
    int n, n_tiles;
    long long* partials;          // [n_tiles][4]: every slot is written by its tile's workgroup (no memset, no atomics)
    long long* sums;              // out [n][4]: S1, S2, L1, L2
};
hipError_t launch_face_quality(const QualityParams& p, hipStream_t stream);

// JPEG encoder (jpeg_encode_kernels.hip; frp.h: frp_encode_jpeg): images in a u8 [.., 3] device buffer -> baseline JPEG scans with libjpeg's
// integer arithmetic.  The buffer is the resident frames (one image per rectangle: pix0 = the rectangle's first pixel, pitch = W) or the
// enhancer's tightly packed output (frp_encode_jpeg_enhanced: pix0 = the image's first pixel, pitch = its width).  Blocks, restart
// intervals and bit-stream words are numbered over ALL images of a call.
struct JpegEncImage {
    long long pix0;               // pixel index of the image's first pixel in the source buffer
    int pitch;                    // pixels from one row to the next
    int h, w;                     // (validated by the caller: every pixel of the image lies inside the buffer, none is empty)
    int mx, my;                   // MCU grid
    int n_int;                    // restart intervals of the image (1 without restart markers)
    int int0;                     // intervals of the images before it
    int pad_;
    long long blk0;               // blocks of the images before it (a block = 64 coefficients)
};
struct JpegEncTables {            // built on the host (jpeg_encode_api.cpp): Annex K's, or one set per image (FRP_FLAG_JPEG_OPTIMIZE)
    uint32_t dc[2][16];           // (length << 16) | code by magnitude category; luminance, chrominance
    uint32_t ac[2][256];          // ... by run / size symbol
    uint16_t q[2][64];            // quantisation tables, natural order
};
struct JpegEncParams {
    const uint8_t* frames;        // the source buffer: u8 pixels of 3 bytes
    long long total_bytes;        // its size: no byte at or beyond it is read
    int rgb_in;
    const JpegEncImage* img;      // [n]
    const JpegEncTables* tab;     // image i codes with tab[i * tab_stride]; the forward half quantises with tab[0].q
    int tab_stride;               // 0: one set for the call, 1: one per image
    int n;
    int hs, vs;                   // luma sampling factors: 2 x 2 (4:2:0) or 1 x 1 (4:4:4); chroma is 1 x 1
    int ri;                       // MCUs per restart interval, 0: none
    long long n_blocks;           // of all images
    long long n_int;              // intervals of all images
    int16_t* coef;                // [n_blocks][64] natural order; per image: component by component over the MCU-padded grid
    uint32_t* hist;               // [n][JE_HIST_BINS] symbol counts per image (zeroed before the histogram kernel); null without it
    // entropy stage (null for the forward half alone)
    uint32_t* blk_bits;                   // [n_blocks], in SCAN order within each image: bits of the block's codes
    unsigned long long* bit_prefix;       // [n_blocks + 1]: exclusive sums of blk_bits
    unsigned long long* group_tot;        // scratch of the prefix sums
    unsigned long long* int_word;         // [n_int + 1]: first 32-bit word of the interval's unstuffed bits in `words`; [n_int] = words used
    uint32_t* int_bytes;                  // [n_int]: unstuffed bytes, the final 1-padding included
    unsigned long long* int_ff0;          // [n_int]: 0xFF bytes of `words` before the interval's first
    uint32_t* int_outb;                   // [n_int]: bytes the interval takes in the file: stuffed, + 2 for the RSTm behind it
    unsigned long long* int_out;          // [n_int + 1]: exclusive sums of int_outb
    unsigned long long* img_off;          // [n + 1]: int_out at every image's first interval; [n] = all scan bytes
    uint32_t* words;                      // the unstuffed bit stream, most significant bit first in each word (zeroed before the pack)
    unsigned long long n_words;           // allocated words: no word at or beyond it is touched
    uint32_t* ff_chunk;                   // [n_chunks]: 0xFF bytes per JE_CHUNK_WORDS words
    unsigned long long* ff_prefix;        // [n_chunks + 1]
    long long n_chunks;
    const unsigned long long* scan_base;  // [n]: where the image's scan starts in `out`
    uint8_t* out;
    unsigned long long out_bytes;         // allocated bytes: no byte at or beyond it is written
};
#define JE_CHUNK_WORDS 256
#define JE_HIST_BINS 544          // per image: dc [2][16] by category, then ac [2][256] by run / size symbol (frp.h: FRP_JPEG_HIST_ELEMS)
size_t jpeg_enc_scan_groups(long long n);       // entries of group_tot a prefix sum over n elements needs
hipError_t launch_jpeg_enc_forward(const JpegEncParams& p, hipStream_t stream);
// the symbols every image's scan will code, counted into hist (zeroed by the caller, behind the forward half)
hipError_t launch_jpeg_enc_hist(const JpegEncParams& p, hipStream_t stream);
// block bits + their prefix sums; bit_prefix[n_blocks] is the size of everything
hipError_t launch_jpeg_enc_measure(const JpegEncParams& p, hipStream_t stream);
// (words zeroed, n_words >= (bit_prefix[n_blocks] >> 5) + n_int + 1): bit packing, 0xFF counts, the intervals' places -> img_off
hipError_t launch_jpeg_enc_pack(const JpegEncParams& p, hipStream_t stream);
// stuffed bytes and restart markers into out
hipError_t launch_jpeg_enc_emit(const JpegEncParams& p, hipStream_t stream);

// Snapshot enhancer (enhance_kernels.hip; frp.h: frp_enhance_pixels): rectangles of the resident u8 frames -> Pillow's
// resize(BICUBIC) + UnsharpMask of the crop, byte for byte, tightly packed in `out`.  All tables come from the host (enhance_api.cpp).
#define ENH_TILE_W 64
#define ENH_TILE_H 32
#define ENH_MAX_BOX_R 1           // box radius of the blur's passes the kernel's LDS tile has halo for: UnsharpMask radius <= 2.0
#define ENH_MAX_HALO (3 * (ENH_MAX_BOX_R + 1))
#define ENH_MAX_TAPS 5            // bicubic, support 2, never downscaling
struct EnhanceTap {               // one output column / row of the resample
    int32_t first;                // first source column / row of the crop (Pillow's xmin)
    int32_t count;                // taps, 1..ENH_MAX_TAPS; first + count <= the crop's width / height
    int32_t k[ENH_MAX_TAPS];      // weights scaled by 2^22; an axis that keeps its size has the one tap 2^22: the identity
    int32_t pad_;
};
struct EnhanceImage {
    int frame, top, left, h, w;   // the rectangle (validated by the caller: inside the frame, not empty)
    int ow, oh;                   // output size, >= w, h
    int tiles_x;                  // ENH_TILE_W x ENH_TILE_H tiles of the OUTPUT per row of tiles
    int tile0;                    // tiles of the images before it
    int xtap, ytap;               // first entry of its ow column taps / oh row taps in `taps`
    int pad_;
    long long out0;               // byte offset of its first pixel in `out`
};
struct EnhanceParams {
    const uint8_t* frames;        // [B,H,W,3] u8, tightly packed, 4-byte aligned base
    long long total_bytes;        // B*H*W*3: no byte at or beyond it is read
    int B, H, W;
    const EnhanceImage* img;      // [n]
    const EnhanceTap* taps;       // [n_taps]
    int n, n_tiles, n_taps;
    int sharpen;                  // 0: resample only
    int box_r;                    // ImageFilter's box radius r (0..ENH_MAX_BOX_R) and its two weights
    uint32_t ww, fw;
    int percent, threshold;
    uint8_t* out;                 // 4-byte aligned base
    long long out_bytes;          // allocated bytes: no byte at or beyond it is written
};
hipError_t launch_enhance(const EnhanceParams& p, hipStream_t stream);

#ifdef FRP_LAB
hipError_t launch_mfma_peak(const _Float16* src, float* dst, int blocks, int iters, hipStream_t stream);
// the conv k-step's MFMA + ds_read_b128 mix without memory traffic or barriers (reads per 4 MFMAs: 4, 3 or 2)
hipError_t launch_mfma_lds(const _Float16* src, float* dst, int blocks, int reads, int iters, hipStream_t stream);
// tuning lab: schedules of the conv k-step's inner loop in isolation (kstep_lab.hip)
hipError_t launch_kstep_lab(const _Float16* src, float* dst, int blocks, int variant, int iters, hipStream_t stream);
int kstep_lab_steps_per_iter(int variant);
int kstep_lab_waves(int variant);
hipError_t launch_fill_random_f16(_Float16* p, long n, unsigned seed, float scale, hipStream_t stream);
#endif

// K6: cosine match, top-1 (and optional full score matrix)
struct MatchParams {
    const _Float16* gallery;  // [N, 512] unit rows
    long N;
    const _Float16* q;        // [Mpad, 512] (rows >= M zero)
    int M, Mpad;
    float* part_cos;          // [n_wg, Mpad]
    int32_t* part_idx;        // [n_wg, Mpad]
    float* best_cos;          // [M]
    int32_t* best_idx;        // [M]
    float* all_scores;        // [M, N] or null
    int n_wg;
    const int32_t* n_dev;     // null, or the real query count (<= M) in device memory (top-1 path only)
    // "within" epilogue (hit_count null: off; not together with all_scores): every row of a real query whose cosine is >= min_cos
    float min_cos;            // >= -2 (cosines lie in [-1, 1]: -2 lists every row)
    int cap;                  // list slots per query, 1..FRP_WITHIN_MAX_CAP
    int32_t* hit_count;       // [M], zeroed on the stream before the pass: the TRUE number of such rows (may exceed cap)
    int32_t* hit_idx;         // [M, cap] ordered by (cosine desc, row asc), -1 beyond min(count, cap); a query with count > cap holds
    float* hit_cos;           // [M, cap] `cap` of its hits, which ones is a race: the caller rebuilds it (launch_topk_rows), -2.0 beyond
};
// Gallery groups of a match launch (both null: off - the kernels above, launched with MatchParams alone; both set: their GROUPS
// instantiations): row r is permitted for query q iff row_groups[r] & q_groups[q] != 0, and top-1, the hit lists and their counts are
// taken over the permitted rows only; all_scores then holds a quiet NaN where a row is not permitted.
// (A kernel argument of its own, not two more fields of MatchParams: the ungrouped kernels' register allocation depends on the size
// of their parameter block - match_top1_within_kernel goes from 2 spilled registers to 524 with 16 more bytes of it.)
struct MatchGroups {
    const uint32_t* row_groups;   // [>= round_up(N, 32)], rows >= N hold 0
    const uint32_t* q_groups;     // [>= M]
};
#define FRP_WITHIN_MAX_CAP 64    // == FRP_MAX_TOPK (frp.h): one lane per list entry in the sort, and what launch_topk_rows rebuilds
int match_num_workgroups(long N);
#define FRP_MATCH_TOP1_MAX 512   // queries per launch the persistent top-1 kernel covers (the only one that takes n_dev)
// per_tile_only: never the persistent top-1 kernel (A/B runs: Switches::match_v1); a launch with n_dev then fails
hipError_t launch_match(const MatchParams& p, bool per_tile_only, hipStream_t stream, MatchGroups groups = MatchGroups{nullptr, nullptr});
// q_groups[f] = frame_groups[face_slot[f] / K] for the n faces of a compact face list (n_dev: the count in device memory, n the capacity)
hipError_t launch_face_groups(const uint32_t* frame_groups, int B, const int32_t* face_slot, int K, int n, const int32_t* n_dev,
                              uint32_t* q_groups, hipStream_t stream);
// top-k of each row of a device score matrix [M x N] by (cosine desc, row asc); -1 / -2.0 beyond N entries
hipError_t launch_topk_rows(const float* scores, int M, long N, int k, int32_t* idx_out, float* cos_out, hipStream_t stream);

// Greedy gallery clustering (cluster_kernels.hip; frp.h: frp_gallery_cluster; host loop: cluster_api.cpp).  The sweep's state in
// device memory: seed_pos [n] (-1: unassigned) and the control words ctl [CLUSTER_CTL_WORDS] below.
#define CLUSTER_MAX_TILE 64          // == FRP_CLUSTER_MAX_TILE (frp.h): one lane per candidate, one bit per candidate in the masks
enum {
    CLUSTER_CTL_COUNT = 0,           // candidates of the current tile (0: no unassigned position is left)
    CLUSTER_CTL_CURSOR = 1,          // every position before it is assigned
    CLUSTER_CTL_NCLUSTERS = 2,       // seeds so far
    CLUSTER_CTL_SEEDS_LO = 3,        // the tile's seed mask, bit t: candidate t is a seed
    CLUSTER_CTL_SEEDS_HI = 4,
    CLUSTER_CTL_CAND = 8,            // the candidates' positions, ascending [CLUSTER_MAX_TILE]
    CLUSTER_CTL_WORDS = CLUSTER_CTL_CAND + CLUSTER_MAX_TILE
};
struct ClusterParams {
    const int32_t* order;     // [n] distinct gallery rows in [0, N): the row of every position
    int n;
    long N;                   // gallery rows = columns of a score row
    int tile;                 // candidates per tile, 1..CLUSTER_MAX_TILE
    int32_t* seed_pos;        // [n]
    int32_t* ctl;             // [CLUSTER_CTL_WORDS]
};
hipError_t launch_cluster_pick(const ClusterParams& p, hipStream_t stream);
// the candidates' rows -> out [tile][512]: fp16 rows widened to float32 (for launch_gallery_normalize), float64 rows copied
hipError_t launch_cluster_stage_f16(const ClusterParams& p, const _Float16* gallery, float* out, hipStream_t stream);
hipError_t launch_cluster_stage_f64(const ClusterParams& p, const double* rows, double* out, hipStream_t stream);
// resolve + assign over the tile's score block [count][N]: member iff score >= min_cos (float32) / dist <= max_dist (float64)
hipError_t launch_cluster_sweep_cos(const ClusterParams& p, const float* score, float min_cos, hipStream_t stream);
hipError_t launch_cluster_sweep_dist(const ClusterParams& p, const double* dist, double max_dist, hipStream_t stream);

}  // namespace frp
