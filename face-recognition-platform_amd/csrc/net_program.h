// The network program layer (host only; net_program.cpp): a blob's op table as a `Net`, the weight rewrites and the analysis done once
// at load, buffer planning, the pass walk and its cache of captured hipGraphs.  The handle it works on: frp_handle.h.
#pragma once
#include <string>
#include <vector>

#include "frp_blob.h"
#include "frp_internal.h"

struct frp_handle;

namespace frp {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct TensorDims {
    int h = 0, w = 0, c = 0;
    bool f32 = false;
    bool f8 = false;      // OCP E4M3 bytes (BASELINE config 5: fp8 matrix path of the embedder)
};

struct Net {
    std::vector<frp_conv_op> ops;
    int n_bufs = 0;
    int in_buf = 0, in_ch = 0;
    bool is_det = false;            // the detector's program (else the embedder's)
    std::vector<DevBuf> bufs;
    std::vector<TensorDims> dims;   // per physical buffer, for the last planned shape
    std::vector<int64_t> wino_off;  // per op: byte offset of its Winograd weight image in the data section, or -1
    // K-concat (conv_mfma.hip): a block's 1x1 stride-s shortcut conv folded into its 3x3 stride-s conv as a second K segment
    std::vector<int> kc_skip;       // per op: 1 = a shortcut conv that its consumer computes (not launched)
    std::vector<int> kc_src;        // per op: index of the shortcut op folded into this conv, or -1
    std::vector<int64_t> kc_w_off, kc_bias_off;   // per consumer op: concatenated weights [Cout][9 Cin + Cin2] / summed bias [Cout]
    // What the op table alone decides, derived once at load (analyse_net); a pass combines it with its per-call conditions
    bool det_stem = false;          // op 0 is the detector's 3x3 s2 3 -> 32 stem: runs as the fused u8 stem kernel (no NHWC8 blob)
    bool det_stem12 = false;        // ... and op 1 the 32 -> 64 stem reading nothing but it: both stems in one kernel
    bool emb_stem = false;          // op 0 is the embedder's 3x3 s1 3 -> 64 PReLU stem: its dedicated kernel
    int fuse_op = -1;               // the first op behind op 0 that launches: the candidate to compute the embedder's stem itself
    bool fuse_ok = false;           // that op is a plain 64 -> 64 conv reading the stem's map, no K-concat consumer, no buffer an alias
    bool fuse_even_only = false;    // the stem's map has no reader besides fuse_op but shortcut convs riding in a later k-loop
    std::vector<char> block64;      // per op: 1 = this op and the next are a residual block of two 3x3 stride-1 64 -> 64 convs that one fused
                                    // launch can compute (conv3x3_block64.hip): the intermediate tensor then never reaches its buffer
    int fc_op = -1;                 // the final op when it writes fp32 (the FC: split-K candidate), or -1
    std::vector<int> next_launch;   // per op: the next op that really launches (its weights are the prefetch target), or -1
};

// split-K of the embedder's FC: l2norm reduces the slabs.  ksplit > 0: slabs written, -1: factor chosen on the device, 0: none
struct FcSplitK {
    int ksplit = 0, ktot = 0;
    const float* bias = nullptr;
};

// What a launch of the FC shape gets (net_program.cpp: pick_fc_splitk; kernel_api.cpp: frp_debug_fc_l2norm): `ksplit` as ConvParams and
// launch_l2norm take it (0: no split, the conv's own fp32 epilogue), `ws_bytes` of slab workspace [ks][batch][cout] fp32
struct FcSplitChoice {
    int ksplit;
    size_t ws_bytes;
};
FcSplitChoice fc_splitk_choice(int batch, int out_pixels, bool device_count, int cout, int ktot, int flags, bool has_res, int n_cu);

// Everything a pass does on the host besides launching.  The walk fills one, run_net applies it - for a launched, a capturing and a
// replayed pass alike.
struct PassEffects {
    double flops = 0, f8_flops = 0;
    int64_t launches = 0, f8_launches = 0;
    FcSplitK fc;
    std::vector<TensorDims> dims;       // per physical buffer, as the pass left them
};

// A network pass as a captured hipGraph (round 5): the ~50 / ~85 launches of a detector / embedder pass replayed by ONE call when the
// same pass - same program, shapes, buffers, operands, switches - is asked for again (run_net).
struct NetGraph {
    std::string key;
    hipGraphExec_t exec = nullptr;
    uint64_t epoch = 0;                 // frp_handle::alloc_epoch at capture: any (re)allocation or weight load since makes it stale
    PassEffects fx;
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
uint16_t f32_to_f16_bits(float f);      // round to nearest even (the rounding of numpy's astype(float16))
float f16_bits_to_f32(uint16_t hbits);
void build_wino_image(const uint16_t* w16, int Cin, int Cout, uint16_t* img);

// an op's output tensor from its input tensor (as stored, or already flattened)
TensorDims conv_out_dims(const TensorDims& in, const frp_conv_op& op);

// Both programs of a blob (header `hd` already checked) into h->det / h->emb, and the device weight image: the data section followed by
// the load-time rewrites.  `sw`: the two switches read at load (no_wino, no_kconcat).
int load_program(frp_handle* h, const frp_blob_header& hd, const unsigned char* blob, size_t bytes, const Switches& sw,
                 std::vector<unsigned char>& image);
// Plan + run one conv program.  in dims: [batch, H, W, in_ch] already written to bufs[in_buf].
int plan_net(frp_handle* h, Net& net, int batch, int H, int W, bool skip_input = false);
// `n_dev`: the number of images that really exist lives in device memory (`batch` is then the capacity the buffers were
// planned for): every kernel derives its tile count from it.  The flop counters are charged for `batch` images and
// corrected by the caller once the count is known.
// `allow_wino` false: the direct kernels also where a Winograd weight image exists (calls of few faces, run_embed).
int run_net(frp_handle* h, const Switches& sw, Net& net, int batch, int H, int W, double* flops, int64_t* launches,
            const StemParams* stem = nullptr, const int32_t* n_dev = nullptr, bool allow_wino = true, FcSplitK* fc = nullptr);
void drop_graphs(frp_handle* h);

}  // namespace frp
