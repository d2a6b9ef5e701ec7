// The network program layer of libfrp.so (net_program.h): parse a blob's op tables, rewrite the weights at load (fp8 expansion, Winograd
// images, K-concat) and analyse the programs once, plan buffers, walk a pass launch by launch, cache the walk as a hipGraph.
#include "net_program.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "frp_handle.h"

namespace frp {

// OCP FP8 E4M3FN (bias 7, no infinities; S.1111.111 = NaN, decoded as 0 here: the packer never emits it)
static float fp8_e4m3_value(unsigned char c) {
    const int e = (c >> 3) & 0xF, m = c & 7;
    float v;
    if (e == 15 && m == 7) v = 0.f;
    else if (e == 0) v = std::ldexp((float)m / 8.0f, -6);
    else v = std::ldexp(1.0f + (float)m / 8.0f, e - 7);
    return (c & 0x80) ? -v : v;
}

// fp32 -> fp16 bit pattern, round to nearest even (the rounding of numpy's astype(float16))
uint16_t f32_to_f16_bits(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));     // NaN / inf
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                                    // rounds to inf (>= 65520)
    if (x < 0x33000001u) return (uint16_t)sign;                                                 // rounds to zero (<= 2^-25)
    const int exp = (int)(x >> 23) - 127;
    uint32_t mant = (x & 0x7fffffu) | 0x800000u;
    int shift;
    uint32_t base;
    if (exp < -14) { shift = 13 + (-14 - exp); base = 0; }                                      // subnormal half
    else { shift = 13; base = (uint32_t)(exp + 15) << 10; mant &= 0x7fffffu; }
    uint32_t q = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (q & 1u))) ++q;                                            // a carry walks into the exponent
    return (uint16_t)(sign | (base + q));
}

float f16_bits_to_f32(uint16_t hbits) {
    const uint32_t sign = (uint32_t)(hbits & 0x8000u) << 16;
    const int e = (hbits >> 10) & 31;
    const uint32_t m = hbits & 0x3ffu;
    float v;
    if (e == 0) v = std::ldexp((float)m, -24);
    else if (e == 31) v = m ? NAN : INFINITY;
    else v = std::ldexp((float)(m | 0x400u), e - 25);
    uint32_t bits;
    memcpy(&bits, &v, 4);
    bits |= sign;
    memcpy(&v, &bits, 4);
    return v;
}

// Weight image of the Winograd kernel (conv3x3_wino.hip) from folded fp16 weights [Cout][3][3][Cin]: per (cout tile of
// 128, 64-channel block, kernel row, 16-channel slice) one 16 KiB stage = the LDS image itself: [frequency f][32-cout block]
// [32 x 16-byte slots] (couts beyond Cout zero), the 8-channel half h of cout r of a block at slot (2 r + h) ^ ((r >> 3) & 1):
// every fragment of a stage is one per-lane base + an immediate (conv3x3_wino.hip: wino_u_slot).  U = G g: g0, (g0+g1+g2)/2,
// (g0-g1+g2)/2, g2 - exact in fp32 on fp16 inputs, rounded once.
void build_wino_image(const uint16_t* w16, int Cin, int Cout, uint16_t* img) {
    const int cpt = Cin / 64, nct = (Cout + 127) / 128;
    for (int ct = 0; ct < nct; ++ct)
        for (int cb = 0; cb < cpt; ++cb)
            for (int kh = 0; kh < 3; ++kh)
                for (int kk = 0; kk < 4; ++kk) {
                    uint16_t* st = img + ((((size_t)ct * cpt + cb) * 3 + kh) * 4 + kk) * 8192;
                    for (int row = 0; row < 128; ++row) {
                        const int co = ct * 128 + row;
                        for (int hh = 0; hh < 2; ++hh)
                            for (int e = 0; e < 8; ++e) {
                                const int ci = cb * 64 + kk * 16 + hh * 8 + e;
                                float g[3] = {0.f, 0.f, 0.f};
                                if (co < Cout)
                                    for (int kw = 0; kw < 3; ++kw) g[kw] = f16_bits_to_f32(w16[(((size_t)co * 3 + kh) * 3 + kw) * Cin + ci]);
                                const float u[4] = {g[0], (g[0] + g[1] + g[2]) * 0.5f, (g[0] - g[1] + g[2]) * 0.5f, g[2]};
                                // stage layout (conv3x3_wino.hip: wino_u_slot): [f][32-cout block][slot (2 r + h) ^ ((r >> 3) & 1)][8 channels]
                                const int r = row & 31, slot = (2 * r + hh) ^ ((r >> 3) & 1);
                                for (int f = 0; f < 4; ++f) st[f * 2048 + (row >> 5) * 512 + slot * 8 + e] = f32_to_f16_bits(u[f]);
                            }
                    }
                }
}

// ---------------------------------------------------------------- an op's tensors
namespace {

// the tensor an op reads: FLATTEN ops see their input as one pixel of all its values
TensorDims flat_input(TensorDims in, const frp_conv_op& op) {
    if (op.flags & FRP_FLAG_FLATTEN) in = {1, 1, in.h * in.w * in.c, false};
    return in;
}

// ... and the tensor(s) it writes: out_buf, and the fp8 copy of an fp16 output in out2_buf
void set_out_dims(std::vector<TensorDims>& d, const frp_conv_op& op, TensorDims out) {
    d[op.out_buf] = out;
    out.f8 = true;
    if (op.out2_buf >= 0) d[op.out2_buf] = out;
}

}  // namespace

TensorDims conv_out_dims(const TensorDims& stored, const frp_conv_op& op) {
    const TensorDims in = flat_input(stored, op);
    auto span = [&](int n) { return (n + 2 * (op.ksize / 2) - op.ksize) / op.stride + 1; };
    TensorDims out;
    out.h = span(in.h);
    out.w = span(in.w);
    out.c = op.cout;
    out.f32 = (op.flags & FRP_FLAG_OUT_F32) != 0;
    out.f8 = (op.flags & FRP_OPFLAG_OUT_FP8) != 0;
    return out;
}

// ---------------------------------------------------------------- load: parse, rewrite the weights, analyse
namespace {

int parse_net(frp_handle* h, const unsigned char* blob, size_t bytes, uint64_t off, uint32_t n_ops, uint32_t n_bufs,
              uint32_t in_buf, uint32_t in_ch, uint64_t data_bytes, Net& net) {
    if (off > bytes || n_ops > (bytes - off) / sizeof(frp_conv_op)) return fail(h, FRP_ERR_BLOB, "op table out of range");
    if (n_bufs == 0 || n_bufs > 4096 || in_buf >= n_bufs) return fail(h, FRP_ERR_BLOB, "bad buffer count");
    for (DevBuf& b : net.bufs) release(b);
    net.ops.resize(n_ops);
    if (n_ops) memcpy(net.ops.data(), blob + off, (size_t)n_ops * sizeof(frp_conv_op));
    net.n_bufs = (int)n_bufs;
    net.in_buf = (int)in_buf;
    net.in_ch = (int)in_ch;
    net.bufs.assign(n_bufs, DevBuf());
    for (const frp_conv_op& op : net.ops) {
        if (op.in_buf < 0 || op.in_buf >= (int)n_bufs || op.out_buf < 0 || op.out_buf >= (int)n_bufs ||
            op.res_buf >= (int)n_bufs || op.res_buf < -1 || op.in_buf == op.out_buf || op.res_buf == op.out_buf)
            return fail(h, FRP_ERR_BLOB, "op buffer id out of range");
        if ((op.flags & FRP_FLAG_RES_UP2) && op.res_buf < 0) return fail(h, FRP_ERR_BLOB, "upsampled residual without a residual buffer");
        if (op.out2_buf < -1 || op.out2_buf >= (int)n_bufs || op.out2_buf == op.in_buf || op.out2_buf == op.out_buf ||
            (op.out2_buf >= 0 && op.out2_buf == op.res_buf))
            return fail(h, FRP_ERR_BLOB, "op second-output buffer id out of range");
        if ((op.flags & FRP_OPFLAG_FP8_MFMA) && !(op.flags & FRP_OPFLAG_W_FP8)) return fail(h, FRP_ERR_BLOB, "fp8 op without fp8 weights");
        if ((op.flags & (FRP_OPFLAG_FP8_MFMA | FRP_OPFLAG_OUT_FP8)) || op.out2_buf >= 0) {
            if (!(op.in_scale > 0.f) || !(op.out_scale > 0.f) || !std::isfinite(op.in_scale) || !std::isfinite(op.out_scale))
                return fail(h, FRP_ERR_BLOB, "fp8 tensor scale must be positive and finite");
        }
        if (!(op.ksize == 1 || op.ksize == 3) || !(op.stride == 1 || op.stride == 2) || op.cin < 8 || (op.cin & 7) ||
            op.cout < 4 || (op.cout & 3) || op.act < 0 || op.act > 2)
            return fail(h, FRP_ERR_BLOB, "op shape not supported");
        const uint64_t welems = (uint64_t)op.cout * op.ksize * op.ksize * op.cin;
        // fp8 storage: one byte per element, then (16-byte aligned) cout fp32 scales
        const uint64_t wbytes = (op.flags & FRP_OPFLAG_W_FP8) ? ((welems + 15) / 16 * 16 + (uint64_t)op.cout * 4) : welems * 2;
        const uint64_t bbytes = (uint64_t)op.cout * 4 * ((op.flags & FRP_FLAG_BORDER_BIAS) ? 9 : 1);
        if (op.w_off < 0 || (uint64_t)op.w_off + wbytes > data_bytes || (op.w_off & 15) || op.bias_off < 0 ||
            (uint64_t)op.bias_off + bbytes > data_bytes || (op.bias_off & 15))
            return fail(h, FRP_ERR_BLOB, "op tensor offset out of range");
        if (op.act == FRP_ACT_PRELU &&
            (op.slope_off < 0 || (uint64_t)op.slope_off + (uint64_t)op.cout * 4 > data_bytes || (op.slope_off & 15)))
            return fail(h, FRP_ERR_BLOB, "op slope offset out of range");
    }
    return FRP_OK;
}

// `n` more bytes at the next 256-byte boundary of the weight image; their offset.  (The image may move: no pointer into it survives.)
size_t append_aligned(std::vector<unsigned char>& image, size_t n) {
    const size_t off = (image.size() + 255) / 256 * 256;
    image.resize(off + n);
    return off;
}

// fp8-stored weights of fp16 ops are expanded to fp16 behind the blob's data section (the kernels are the fp16 ones)
void expand_fp8_weights(Net& net, std::vector<unsigned char>& image) {
    for (frp_conv_op& op : net.ops) {
        if (!(op.flags & FRP_OPFLAG_W_FP8) || (op.flags & FRP_OPFLAG_FP8_MFMA)) continue;   // fp8 ops use the bytes as stored
        const size_t per_row = (size_t)op.ksize * op.ksize * op.cin, n = per_row * op.cout;
        const size_t src = (size_t)op.w_off, sc = src + (n + 15) / 16 * 16;
        const size_t dst = append_aligned(image, n * 2);
        const unsigned char* data = image.data();
        uint16_t* out16 = reinterpret_cast<uint16_t*>(image.data() + dst);
        for (int r = 0; r < op.cout; ++r) {
            float scale;
            memcpy(&scale, data + sc + (size_t)r * 4, 4);
            for (size_t i = 0; i < per_row; ++i)
                out16[(size_t)r * per_row + i] = f32_to_f16_bits(fp8_e4m3_value(data[src + (size_t)r * per_row + i]) * scale);
        }
        op.w_off = (int64_t)dst;
        op.flags &= ~FRP_OPFLAG_W_FP8;
    }
}

// Winograd weight images (conv3x3_wino.hip) for the 3x3 stride-1 layers `shape_ok` admits, appended behind the data section.  `width`:
// the network's static input width (the embedder's 112 x 112 chips: the map width of every op is known here), or 0.
void add_wino_images(Net& net, int width, bool (*shape_ok)(const frp_conv_op& op, int win), std::vector<unsigned char>& image) {
    std::vector<TensorDims> d(net.n_bufs);
    d[net.in_buf] = {width, width, net.in_ch, false};
    for (size_t i = 0; i < net.ops.size(); ++i) {
        const frp_conv_op& op = net.ops[i];
        const int win = flat_input(d[op.in_buf], op).w;
        set_out_dims(d, op, conv_out_dims(d[op.in_buf], op));
        if (!shape_ok(op, win) || op.cout < 64 || op.out2_buf >= 0 ||
            (op.flags & (FRP_FLAG_OUT_F32 | FRP_FLAG_FLATTEN | FRP_FLAG_RES_UP2 | FRP_OPFLAG_W_FP8 | FRP_OPFLAG_FP8_MFMA | FRP_OPFLAG_OUT_FP8)))
            continue;
        const size_t dst = append_aligned(image, conv3x3_wino_image_bytes(op.cin, op.cout));
        build_wino_image(reinterpret_cast<const uint16_t*>(image.data() + op.w_off), op.cin, op.cout, reinterpret_cast<uint16_t*>(image.data() + dst));
        net.wino_off[i] = (int64_t)dst;
    }
}

// K-concat plan of one network: which 1x1 shortcut convs ride in their consumer's k-loop, the concatenated weights and summed biases.
// `read_outside`: the buffers something behind the program reads (the decode kernel, the l2norm).
void plan_kconcat(Net& net, const std::vector<int>& read_outside, std::vector<unsigned char>& image) {
    const size_t n_ops = net.ops.size();
    for (size_t j = 0; j < n_ops; ++j) {
        const frp_conv_op& c = net.ops[j];
        // consumer: 3x3 conv over whole channel blocks with a plain residual, fp16 operands, one bias class
        if (c.ksize != 3 || c.res_buf < 0 || (c.cin & 63) || c.flags != 0) continue;
        // producer of the residual: the last writer of res_buf before j
        int i = -1;
        for (int q = (int)j - 1; q >= 0; --q)
            if (net.ops[q].out_buf == c.res_buf || net.ops[q].out2_buf == c.res_buf) { i = q; break; }
        if (i < 0) continue;
        const frp_conv_op& d = net.ops[i];
        if (d.out_buf != c.res_buf || d.ksize != 1 || d.stride != c.stride || d.act != FRP_ACT_NONE || d.res_buf >= 0 || d.flags != 0 ||
            d.out2_buf >= 0 || d.cout != c.cout || (d.cin & 63) || !(c.cin == d.cin || c.cin == 2 * d.cin) || net.kc_skip[i])
            continue;
        // the shortcut map has no other reader while it holds this tensor; its input and the consumer's input stay
        // untouched from the shortcut op to the consumer, and the consumer does not write over the shortcut's input
        bool ok = c.out_buf != d.in_buf && c.in_buf != d.in_buf;
        for (size_t q = (size_t)i + 1; q < n_ops && ok; ++q) {
            const frp_conv_op& o = net.ops[q];
            if (q != j && (o.in_buf == c.res_buf || o.res_buf == c.res_buf)) ok = false;     // another reader
            if (q < j && (o.out_buf == d.in_buf || o.out2_buf == d.in_buf)) ok = false;       // shortcut input rewritten early
            if (o.out_buf == c.res_buf || o.out2_buf == c.res_buf) break;                     // the buffer moves on to another tensor
        }
        for (int b : read_outside) ok &= b != c.res_buf;
        if (!ok) continue;
        const size_t k1 = (size_t)9 * c.cin, k2 = (size_t)d.cin, kt = k1 + k2;
        const size_t wdst = append_aligned(image, (size_t)c.cout * kt * 2);
        const size_t bdst = append_aligned(image, (size_t)c.cout * 4);
        unsigned char* im = image.data();
        for (int r = 0; r < c.cout; ++r) {
            memcpy(im + wdst + ((size_t)r * kt) * 2, im + c.w_off + (size_t)r * k1 * 2, k1 * 2);
            memcpy(im + wdst + ((size_t)r * kt + k1) * 2, im + d.w_off + (size_t)r * k2 * 2, k2 * 2);
            float b1, b2;
            memcpy(&b1, im + c.bias_off + (size_t)r * 4, 4);
            memcpy(&b2, im + d.bias_off + (size_t)r * 4, 4);
            const float bs = b1 + b2;
            memcpy(im + bdst + (size_t)r * 4, &bs, 4);
        }
        net.kc_skip[i] = 1;
        net.kc_src[j] = i;
        net.kc_w_off[j] = (int64_t)wdst;
        net.kc_bias_off[j] = (int64_t)bdst;
    }
}

// first detector op as the fused u8 stem (no NHWC8 blob)?
bool stem_fusable(const Net& net) {
    if (net.ops.empty()) return false;
    const frp_conv_op& op = net.ops[0];
    return op.in_buf == net.in_buf && op.cin == 8 && op.cout == 32 && op.ksize == 3 && op.stride == 2 &&
           op.act == FRP_ACT_RELU && op.res_buf < 0 && op.flags == 0 && (op.real_ch & 0xffff) == 3;
}

// ... and the second one (3x3 s2 32->64 + ReLU) reading nothing but the first: both stems in one kernel
bool stem12_fusable(const Net& net) {
    if (!stem_fusable(net) || net.ops.size() < 2) return false;
    const frp_conv_op& a = net.ops[0];
    const frp_conv_op& b = net.ops[1];
    if (!(b.in_buf == a.out_buf && b.cin == 32 && b.cout == 64 && b.ksize == 3 && b.stride == 2 && b.act == FRP_ACT_RELU &&
          b.res_buf < 0 && b.flags == 0))
        return false;
    for (size_t i = 2; i < net.ops.size(); ++i)          // the stem1 map must have no other reader
        if (net.ops[i].in_buf == a.out_buf || net.ops[i].res_buf == a.out_buf) {
            // (physical buffers are recycled: a later tensor may live in the same buffer - only a read
            // before the next write of that buffer would be the stem1 map)
            bool rewritten = false;
            for (size_t j = 2; j < i; ++j) rewritten |= net.ops[j].out_buf == a.out_buf;
            if (!rewritten) return false;
        }
    return true;
}

// The embedder's stem (chips NHWC8 -> 3x3 s1 3->64 + PReLU) and the conv behind it.  Where that conv runs on the 64 -> 64 kernel
// (conv3x3_c64.hip), its launch computes the stem of its own input patch from the chips: the 64-channel map is written once (the block's
// shortcut reads it) and never read back by the conv; one launch fewer.
void analyse_emb_stem(Net& net) {
    const frp_conv_op& a = net.ops[0];
    net.emb_stem = a.in_buf == net.in_buf && a.cin == 8 && (a.real_ch & 0xffff) == 3 && a.cout == 64 && a.ksize == 3 && a.stride == 1 &&
                   a.act == FRP_ACT_PRELU && a.res_buf < 0 && a.flags == 0 && a.slope_off >= 0;
    // (the next op that launches: the block's shortcut conv in between rides in a later k-loop - kc_skip - and reads the map then)
    const int nb = net.next_launch[0];
    net.fuse_op = nb;
    if (nb < 0) return;
    const frp_conv_op& b = net.ops[nb];
    const bool plain = !(b.flags & ~FRP_FLAG_BORDER_BIAS) && (b.flags & FRP_FLAG_BORDER_BIAS) && b.out2_buf < 0 && b.res_buf < 0;
    const bool chained = net.kc_src[nb] < 0;
    // (the fused launch reads the chips while it writes both maps: none of the three buffers may be another's alias - this
    // packer pins network inputs, a foreign blob's plan might not)
    net.fuse_ok = plain && chained && b.in_buf == a.out_buf && b.out_buf != a.out_buf && b.out_buf != a.in_buf && a.out_buf != a.in_buf &&
                  b.cin == 64 && b.cout == 64 && b.ksize == 3 && b.stride == 1 && b.act == FRP_ACT_PRELU && b.slope_off >= 0;
    // who else reads the stem's map?  Only shortcut convs (1x1, stride 2) that ride in a later k-loop: then a quarter of its
    // pixels is all that has to reach HBM
    net.fuse_even_only = true;
    for (int j = 1; j < (int)net.ops.size(); ++j) {
        const frp_conv_op& o = net.ops[j];
        if (j == nb || (o.in_buf != a.out_buf && o.res_buf != a.out_buf)) continue;
        const bool shortcut = net.kc_skip[j] && o.in_buf == a.out_buf && o.res_buf != a.out_buf && o.ksize == 1 && o.stride == 2;
        if (!shortcut) net.fuse_even_only = false;
    }
}

// Residual blocks of two 3x3 stride-1 64 -> 64 convs that the fused block kernel can take (conv3x3_block64.hip): ops (i, i + 1) where the
// intermediate tensor has no reader but op i + 1, the residual is op i's input and the output lands in a third buffer.  A blob that
// fails a precondition runs the two launches, as with K-concat.  `read_outside`: the buffers something behind the program reads.
void analyse_block64(Net& net, const std::vector<int>& read_outside) {
    const int n = (int)net.ops.size();
    net.block64.assign(n, 0);
    for (int i = 0; i + 1 < n; ++i) {
        const frp_conv_op &a = net.ops[i], &b = net.ops[i + 1];
        auto c64 = [](const frp_conv_op& o) { return o.ksize == 3 && o.stride == 1 && o.cin == 64 && o.cout == 64 && o.out2_buf < 0; };
        if (!c64(a) || !c64(b) || net.kc_skip[i] || net.kc_skip[i + 1] || net.kc_src[i] >= 0 || net.kc_src[i + 1] >= 0) continue;
        if (a.res_buf >= 0 || b.in_buf != a.out_buf || b.res_buf != a.in_buf || b.out_buf == a.in_buf || b.out_buf == a.out_buf) continue;
        if (a.in_buf == net.in_buf && net.in_ch != 64) continue;
        if (!conv3x3_block64_variant(a.act, a.flags, a.slope_off >= 0, b.act, b.flags)) continue;       // (also: no fp8 / OUT_F32 / RES_UP2 flag)
        if (net.fuse_ok && i == net.fuse_op) continue;                                                   // the launch that computes the embedder's stem
        bool ok = true;
        for (int q = i + 2; q < n && ok; ++q) {                  // the intermediate tensor has no other reader while the buffer holds it
            const frp_conv_op& o = net.ops[q];
            if (o.in_buf == a.out_buf || o.res_buf == a.out_buf) ok = false;
            if (o.out_buf == a.out_buf || o.out2_buf == a.out_buf) break;
        }
        for (int r : read_outside) ok &= r != a.out_buf;
        if (!ok) continue;
        net.block64[i] = 1;
        ++i;                                                     // (op i + 1 belongs to this pair)
    }
}

// every fact of the finished op table (K-concat plan included) that a pass would otherwise re-derive
void analyse_net(Net& net, const std::vector<int>& read_outside) {
    const int n = (int)net.ops.size();
    net.det_stem = stem_fusable(net);
    net.det_stem12 = stem12_fusable(net);
    net.fc_op = n && (net.ops[n - 1].flags & FRP_FLAG_OUT_F32) ? n - 1 : -1;
    net.next_launch.assign(n, -1);
    for (int i = n - 1, nx = -1; i >= 0; --i) {
        net.next_launch[i] = nx;
        if (!net.kc_skip[i]) nx = i;
    }
    net.emb_stem = net.fuse_ok = net.fuse_even_only = false;
    net.fuse_op = -1;
    if (n) analyse_emb_stem(net);
    analyse_block64(net, read_outside);
}

}  // namespace

int load_program(frp_handle* h, const frp_blob_header& hd, const unsigned char* blob, size_t bytes, const Switches& sw,
                 std::vector<unsigned char>& image) {
    Net &det = h->det, &emb = h->emb;
    det.is_det = true;
    FRPCHK(parse_net(h, blob, bytes, hd.det_ops_offset, hd.n_det_ops, hd.n_det_bufs, hd.det_in_buf, hd.det_in_ch, hd.data_bytes, det));
    FRPCHK(parse_net(h, blob, bytes, hd.emb_ops_offset, hd.n_emb_ops, hd.n_emb_bufs, hd.emb_in_buf, hd.emb_in_ch, hd.data_bytes, emb));
    for (int l = 0; l < 3; ++l)
        if (hd.det_head_buf[l] >= hd.n_det_bufs) return fail(h, FRP_ERR_BLOB, "head buffer id out of range");
    if (hd.emb_out_buf >= hd.n_emb_bufs) return fail(h, FRP_ERR_BLOB, "embedding buffer id out of range");
    image.assign(blob + hd.data_offset, blob + hd.data_offset + hd.data_bytes);
    for (Net* net : {&det, &emb}) {
        const size_t n_ops = net->ops.size();
        net->wino_off.assign(n_ops, -1);
        net->kc_skip.assign(n_ops, 0);
        net->kc_src.assign(n_ops, -1);
        net->kc_w_off.assign(n_ops, -1);
        net->kc_bias_off.assign(n_ops, -1);
        expand_fp8_weights(*net, image);
    }
    if (!sw.no_wino) {                // FRP_NO_WINO: direct kernels only
        add_wino_images(emb, FRP_CHIP, [](const frp_conv_op& op, int win) { return conv3x3_wino_shape_ok(win, op.cin, op.ksize, op.stride); }, image);
        // The detector's maps depend on the frame size, so which of its layers take the kernel (in its 2-D tile form: maps wider than
        // 30 pixels) is decided per launch (conv3x3_wino.hip: wino_2d_pays); every 3x3 stride-1 layer of 128 channels and more that
        // could gets an image here (a third more weight bytes for those layers).
        add_wino_images(det, 0, [](const frp_conv_op& op, int) { return op.ksize == 3 && op.stride == 1 && !(op.cin & 63) && op.cin >= 128; }, image);
    }
    if (!sw.no_kconcat) {             // FRP_NO_KCONCAT: every op as written in the blob
        plan_kconcat(det, {(int)hd.det_head_buf[0], (int)hd.det_head_buf[1], (int)hd.det_head_buf[2]}, image);
        plan_kconcat(emb, {(int)hd.emb_out_buf}, image);
    }
    analyse_net(det, {(int)hd.det_head_buf[0], (int)hd.det_head_buf[1], (int)hd.det_head_buf[2]});
    analyse_net(emb, {(int)hd.emb_out_buf});
    return FRP_OK;
}

// ---------------------------------------------------------------- plan
int plan_net(frp_handle* h, Net& net, int batch, int H, int W, bool skip_input) {
    net.dims.assign(net.n_bufs, TensorDims());
    std::vector<size_t> need(net.n_bufs, 0);
    net.dims[net.in_buf] = {H, W, net.in_ch, false};
    need[net.in_buf] = skip_input ? 0 : (size_t)batch * H * W * net.in_ch * 2;
    for (const frp_conv_op& op : net.ops) {
        if (net.dims[op.in_buf].c == 0) return fail(h, FRP_ERR_BLOB, "program reads an unwritten buffer");
        const TensorDims in = flat_input(net.dims[op.in_buf], op), out = conv_out_dims(in, op);
        if (in.c != op.cin) return fail(h, FRP_ERR_BLOB, "program channel mismatch");
        if (out.h <= 0 || out.w <= 0) return fail(h, FRP_ERR_INVALID, "input too small for the network");
        if (in.f32) return fail(h, FRP_ERR_BLOB, "program reads an fp32 tensor as a conv input");
        const bool op_f8 = (op.flags & FRP_OPFLAG_FP8_MFMA) != 0;
        if (in.f8 != op_f8) return fail(h, FRP_ERR_BLOB, "program operand precision mismatch (fp8 op <-> fp8 tensor)");
        if (op_f8 && !(op.ksize == 3 && op.stride == 1 && (op.cin & 127) == 0 && !(op.flags & (FRP_FLAG_OUT_F32 | FRP_FLAG_FLATTEN | FRP_FLAG_RES_UP2))))
            return fail(h, FRP_ERR_BLOB, "op shape not covered by the fp8 matrix path");
        if (out.f8 && (out.f32 || !op_f8)) return fail(h, FRP_ERR_BLOB, "fp8 primary output needs an fp8 op");
        if (op.res_buf >= 0) {                     // the epilogue reads the residual unchecked: validate it here
            const TensorDims& r = net.dims[op.res_buf];
            const bool up2 = (op.flags & FRP_FLAG_RES_UP2) != 0;
            if (r.c != op.cout || r.f32 || r.f8 || (up2 ? (r.h * 2 != out.h || r.w * 2 != out.w) : (r.h != out.h || r.w != out.w)))
                return fail(h, FRP_ERR_BLOB, "program residual shape mismatch");
        }
        if (op.out2_buf >= 0 && (out.f32 || out.f8)) return fail(h, FRP_ERR_BLOB, "fp8 copy of a non-fp16 output");
        set_out_dims(net.dims, op, out);
        const size_t elems = (size_t)batch * out.h * out.w * out.c;
        need[op.out_buf] = std::max(need[op.out_buf], elems * (out.f32 ? 4 : out.f8 ? 1 : 2));
        if (op.out2_buf >= 0) need[op.out2_buf] = std::max(need[op.out2_buf], elems);
    }
    for (int i = 0; i < net.n_bufs; ++i)
        if (need[i]) FRPCHK(ensure(h, net.bufs[i], need[i]));
    return FRP_OK;
}

// ---------------------------------------------------------------- the pass
namespace {

struct NetPass {       // what run_net was asked for
    frp_handle* h;
    const Switches& sw;
    Net& net;
    int batch, H, W;
    const StemParams* stem;
    const int32_t* n_dev;
    bool allow_wino;
    const char* weights() const { return (const char*)h->wdata.p; }
};

struct FusedStem {  // the embedder's stem, handed to the launch of the 64 -> 64 conv behind it (Net::fuse_op)
    bool on = false;
    EmbStemParams p{};
};

int launched(frp_handle* h, hipError_t e, const char* what) {
    return e == hipSuccess ? FRP_OK : fail(h, FRP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// The detector's stem(s) straight from the u8 frames.  Both in one kernel (the stem1 map never reaches HBM); FRP_NO_FUSED_STEM12 keeps
// stem1 (fused with the u8 normalisation) and stem2 (generic conv) apart for A/B runs.  `next`: the first op left to the walk.
int run_det_stems(const NetPass& ps, PassEffects& fx, size_t& next) {
    frp_handle* h = ps.h;
    const Net& net = ps.net;
    const StemParams& st = *ps.stem;
    const char* wbase = ps.weights();
    if (net.ops.empty()) return FRP_OK;
    const frp_conv_op& a = net.ops[0];
    if (net.det_stem12 && (st.Hc % 4) == 0 && (st.Wc % 4) == 0 && !ps.sw.no_fused_stem12) {
        const frp_conv_op& b = net.ops[1];
        Stem12Params sp{};
        sp.frames = st.frames; sp.B = st.B; sp.H = st.H; sp.W = st.W;
        sp.row_stride = st.row_stride; sp.frame_stride = st.frame_stride;
        sp.Hc = st.Hc; sp.Wc = st.Wc; sp.Ho1 = st.Hc / 2; sp.Wo1 = st.Wc / 2; sp.Ho2 = st.Hc / 4; sp.Wo2 = st.Wc / 4;
        sp.rgb_in = st.rgb_in;
        sp.w1 = (const _Float16*)(wbase + a.w_off); sp.bias1 = (const float*)(wbase + a.bias_off);
        sp.w2 = (const _Float16*)(wbase + b.w_off); sp.bias2 = (const float*)(wbase + b.bias_off);
        sp.out = (_Float16*)net.bufs[b.out_buf].p;
        FRPCHK(launched(h, launch_stem12_u8(sp, h->stream), "launch_stem12_u8"));
        fx.dims[a.out_buf] = {sp.Ho1, sp.Wo1, 32, false};
        fx.dims[b.out_buf] = {sp.Ho2, sp.Wo2, 64, false};
        fx.flops += 2.0 * ps.batch * sp.Ho1 * sp.Wo1 * 9.0 * 3 * 32 + 2.0 * ps.batch * sp.Ho2 * sp.Wo2 * 9.0 * 32 * 64;
        fx.launches += 1;
        next = 2;
        if (!h->det_hash_on) return FRP_OK;
        return launched(h, launch_tensor_hash(sp.out, (size_t)ps.batch * sp.Ho2 * sp.Wo2 * 64 * 2, (unsigned long long*)h->det_hashes.p + 1, h->stream),
                        "tensor_hash");
    }
    StemParams sp = st;
    sp.w = (const _Float16*)(wbase + a.w_off);
    sp.bias = (const float*)(wbase + a.bias_off);
    sp.out = (_Float16*)net.bufs[a.out_buf].p;
    FRPCHK(launched(h, launch_stem_u8(sp, h->stream), "launch_stem_u8"));
    fx.dims[a.out_buf] = {sp.Ho, sp.Wo, 32, false};
    fx.flops += 2.0 * ps.batch * sp.Ho * sp.Wo * 9.0 * 3 * 32;
    fx.launches += 1;
    next = 1;
    return FRP_OK;
}

// The embedder's stem on its dedicated kernel (FRP_NO_EMB_STEM keeps the generic one) - or, where the conv behind it takes it into its
// own launch, its parameters for that launch (`fused`; FRP_NO_STEM_FUSE: the two launches, for A/B runs; the results are the same bits)
int run_emb_stem(const NetPass& ps, PassEffects& fx, size_t& next, FusedStem& fused) {
    const Net& net = ps.net;
    if (!net.emb_stem || ps.sw.no_emb_stem) return FRP_OK;
    const frp_conv_op& a = net.ops[0];
    const char* wbase = ps.weights();
    EmbStemParams ep{};
    ep.x = (const _Float16*)net.bufs[a.in_buf].p;
    ep.M = ps.batch; ep.H = ps.H; ep.W = ps.W;
    ep.w = (const _Float16*)(wbase + a.w_off);
    ep.bias = (const float*)(wbase + a.bias_off);
    ep.slope = (const float*)(wbase + a.slope_off);
    ep.out = (_Float16*)net.bufs[a.out_buf].p;
    ep.n_dev = ps.n_dev;
    fused.on = net.fuse_ok && !ps.sw.no_stem_fuse && ps.sw.small_m <= 0 && conv3x3_c64_fuses_stem(ps.batch, ps.H, ps.W, ps.h->n_cu);
    if (fused.on) {
        fused.p = ep;
    } else {
        FRPCHK(launched(ps.h, launch_emb_stem(ep, ps.h->stream), "launch_emb_stem"));
        fx.launches += 1;
    }
    fx.dims[a.out_buf] = {ps.H, ps.W, 64, false};
    fx.flops += 2.0 * ps.batch * ps.H * ps.W * 9.0 * 3 * 64;
    next = 1;
    return FRP_OK;
}

// the launch parameters of op `i` reading a tensor of dims `in` (`d`: the pass's dims table, for the residual)
ConvParams conv_params_for(const NetPass& ps, size_t i, const TensorDims& in, const std::vector<TensorDims>& d, const FusedStem& fused) {
    const Net& net = ps.net;
    const frp_conv_op& op = net.ops[i];
    const char* wbase = ps.weights();
    ConvParams p{};
    p.x = (const _Float16*)net.bufs[op.in_buf].p;
    p.w = (const _Float16*)(wbase + op.w_off);
    p.bias = (const float*)(wbase + op.bias_off);
    p.slope = op.slope_off >= 0 ? (const float*)(wbase + op.slope_off) : nullptr;
    p.res = op.res_buf >= 0 ? (const _Float16*)net.bufs[op.res_buf].p : nullptr;
    p.out = net.bufs[op.out_buf].p;
    p.N = ps.batch; p.H = in.h; p.W = in.w; p.Cin = op.cin; p.Cout = op.cout;
    p.KS = op.ksize; p.stride = op.stride; p.act = op.act;
    p.n_dev = ps.n_dev;
    p.n_cu = ps.h->n_cu;
    p.small_m = ps.sw.small_m;
    // the kernel A/B bits of every conv launch of the pass (frp_internal.h: CONV_DBG_*)
    p.dbg = (ps.sw.s2 ? CONV_DBG_S2 : 0) | (process_switches().c64_all ? CONV_DBG_C64_ALL : 0);
    if (fused.on && (int)i == net.fuse_op) {
        p.stem_x = fused.p.x; p.stem_w = fused.p.w; p.stem_bias = fused.p.bias; p.stem_slope = fused.p.slope; p.stem_out = fused.p.out;
        p.stem_even_only = net.fuse_even_only ? 1 : 0;
    }
    p.wino_wide_only = net.is_det ? 1 : 0;
    if (ps.allow_wino && net.wino_off[i] >= 0) p.wino_w = (const _Float16*)(wbase + net.wino_off[i]);
    p.flags = op.flags & (FRP_FLAG_BORDER_BIAS | FRP_FLAG_OUT_F32 | FRP_FLAG_RES_UP2);
    if (op.flags & FRP_FLAG_RES_UP2) { p.Hr = d[op.res_buf].h; p.Wr = d[op.res_buf].w; }
    p.in_scale = p.out_scale = 1.0f;
    if (op.flags & FRP_OPFLAG_FP8_MFMA) {      // fp8 operands: E4M3 weights as stored, per-cout scales behind them
        const size_t welems = (size_t)op.cout * op.ksize * op.ksize * op.cin;
        p.flags |= FRP_FLAG_F8;
        p.wscale = (const float*)(wbase + op.w_off + (welems + 15) / 16 * 16);
        p.in_scale = op.in_scale;
    }
    if (net.kc_src[i] >= 0) {                  // K-concat: the block's shortcut conv rides in this conv's k-loop
        const frp_conv_op& sc = net.ops[net.kc_src[i]];
        p.x2 = (const _Float16*)net.bufs[sc.in_buf].p;
        p.Cin2 = sc.cin;
        p.w = (const _Float16*)(wbase + net.kc_w_off[i]);
        p.bias = (const float*)(wbase + net.kc_bias_off[i]);
        p.res = nullptr;
    }
    if (op.flags & FRP_OPFLAG_OUT_FP8) p.flags |= FRP_FLAG_OUT_FP8;
    if (op.out2_buf >= 0) p.out2 = net.bufs[op.out2_buf].p;
    if ((op.flags & FRP_OPFLAG_OUT_FP8) || op.out2_buf >= 0) p.out_scale = op.out_scale;
    // the weights the NEXT launch will stream (a quarter-tile launch with CUs to spare warms the L2s with them: conv_common.h)
    const int nx = net.next_launch[i];
    if (nx < 0) return p;
    const frp_conv_op& no = net.ops[nx];
    if (net.kc_src[nx] >= 0) {
        p.pf_ptr = wbase + net.kc_w_off[nx];
        p.pf_bytes = (unsigned)((size_t)no.cout * (9 * (size_t)no.cin + net.ops[net.kc_src[nx]].cin) * 2);
    } else if (ps.allow_wino && net.wino_off[nx] >= 0) {
        p.pf_ptr = wbase + net.wino_off[nx];
        p.pf_bytes = (unsigned)std::min<size_t>(conv3x3_wino_image_bytes(no.cin, no.cout), 0x7fffffffu);
    } else {
        const size_t es = (no.flags & FRP_OPFLAG_FP8_MFMA) ? 1 : 2;
        p.pf_ptr = wbase + no.w_off;
        p.pf_bytes = (unsigned)std::min<size_t>((size_t)no.cout * no.ksize * no.ksize * no.cin * es, 0x7fffffffu);
    }
    return p;
}

}  // namespace

// The split-K choice of a skinny fp32-output GEMM launch (the FC) of `batch` images with `out_pixels` outputs each: the value of
// ConvParams::ksplit and the bytes of the slab workspace.  Device-side count: the kernel picks the factor of the real batch itself (the
// same function), the slabs are sized for the largest one - that of a single image - times the capacity.
FcSplitChoice fc_splitk_choice(int batch, int out_pixels, bool device_count, int cout, int ktot, int flags, bool has_res, int n_cu) {
    const int ks = conv_pick_ksplit((device_count ? 1 : batch) * out_pixels, cout, ktot, flags, has_res, n_cu);
    if (ks <= 1) return {0, 0};
    return {device_count ? -1 : ks, (size_t)ks * batch * cout * 4};   // 1x1 output per image for the FC shape
}

namespace {

// skinny fp32-output GEMM (the FC): split K over the CUs; the slabs are reduced (+bias) by the l2norm kernel that follows
void pick_fc_splitk(const NetPass& ps, const frp_conv_op& op, const TensorDims& in, const TensorDims& out, ConvParams& p, FcSplitK& fc) {
    frp_handle* h = ps.h;
    const int ktot = op.ksize * op.ksize * op.cin;
    const FcSplitChoice c = fc_splitk_choice(ps.batch, out.h * out.w, ps.n_dev != nullptr, op.cout, ktot, op.flags, op.res_buf >= 0, h->n_cu);
    if (c.ksplit == 0 || in.h != 1 || in.w != 1) return;
    if (ensure(h, h->splitk_ws, c.ws_bytes) != FRP_OK) return;
    p.ksplit = c.ksplit;
    p.out = h->splitk_ws.p;
    fc.ksplit = p.ksplit;
    fc.bias = p.bias;
    fc.ktot = ktot;
}

// what a launched op is charged for: algorithmic FLOPs on the unpadded channels
void charge(const frp_conv_op& op, const TensorDims& out, int batch, PassEffects& fx) {
    const int cin_r = op.real_ch & 0xffff, cout_r = (op.real_ch >> 16) & 0xffff;
    const double fl = 2.0 * batch * out.h * out.w * (double)op.ksize * op.ksize * (cin_r ? cin_r : op.cin) * (cout_r ? cout_r : op.cout);
    fx.flops += fl;
    fx.launches += 1;
    if (op.flags & FRP_OPFLAG_FP8_MFMA) { fx.f8_flops += fl; fx.f8_launches += 1; }
}

// Does this pass run a marked residual block (Net::block64) on maps of dims `in` as the fused launch?  Where its plan pays
// (conv3x3_block64.hip: conv3x3_block64_pays; FRP_BLOCK_FUSE_ALL: wherever the kernel reaches); never with FRP_NO_BLOCK_FUSE or forced
// quarter tiles.  (The walk adds: not with the per-op hashes, not when the diagnostic op limit cuts the pair.)
bool block64_fuses(const NetPass& ps, const TensorDims& in) {
    if (ps.sw.no_block_fuse || ps.sw.small_m > 0) return false;
    Block64Plan plan;
    if (!conv3x3_block64_plan(ps.batch, in.h, in.w, ps.h->n_cu, &plan)) return false;
    if ((in.h < 2 || in.w < 2)) return false;
    return ps.sw.block_fuse_all || conv3x3_block64_pays(plan);
}

// One pass, launch by launch, into `fx` (nothing else on the handle or the net is written, but for the split-K workspace).
int walk(const NetPass& ps, PassEffects& fx) {
    frp_handle* h = ps.h;
    const Net& net = ps.net;
    fx = PassEffects();
    std::vector<TensorDims>& d = fx.dims;      // re-derived while walking (physical buffers are reused by several tensors)
    d.assign(net.n_bufs, TensorDims());
    d[net.in_buf] = {ps.H, ps.W, net.in_ch, false};
    const bool hashing = net.is_det && h->det_hash_on;       // (diagnostic: a hash of every op's output, in stream order)
    if (hashing) HIPCHK(h, hipMemsetAsync(h->det_hashes.p, 0, 64 * 8, h->stream));
    size_t i = 0;
    FusedStem fused;
    if (ps.stem) FRPCHK(run_det_stems(ps, fx, i));
    else FRPCHK(run_emb_stem(ps, fx, i, fused));
    size_t end = net.ops.size();
    if (net.is_det && h->det_op_limit >= 0) end = std::min(end, (size_t)h->det_op_limit);      // (diagnostic prefix run)
    for (; i < end; ++i) {
        const frp_conv_op& op = net.ops[i];
        const TensorDims in = flat_input(d[op.in_buf], op), out = conv_out_dims(in, op);
        if (net.kc_skip[i]) {                  // a shortcut conv its consumer computes (K-concat): FLOPs charged here
            set_out_dims(d, op, out);
            fx.flops += 2.0 * ps.batch * out.h * out.w * (double)op.cin * op.cout;
            continue;
        }
        if (net.block64[i] && i + 1 < end && !hashing && block64_fuses(ps, in)) {
            // the residual block (i, i + 1) as ONE launch: both ops' dims and FLOPs, one launch; op i's output buffer is not written
            const frp_conv_op& op2 = net.ops[i + 1];
            const char* wbase = ps.weights();
            Block64Params bp{};
            bp.x = (const _Float16*)net.bufs[op.in_buf].p;
            bp.out = net.bufs[op2.out_buf].p;
            bp.w1 = (const _Float16*)(wbase + op.w_off); bp.bias1 = (const float*)(wbase + op.bias_off);
            bp.slope1 = op.slope_off >= 0 ? (const float*)(wbase + op.slope_off) : nullptr;
            bp.w2 = (const _Float16*)(wbase + op2.w_off); bp.bias2 = (const float*)(wbase + op2.bias_off);
            bp.slope2 = op2.slope_off >= 0 ? (const float*)(wbase + op2.slope_off) : nullptr;
            bp.n_dev = ps.n_dev;
            bp.N = ps.batch; bp.H = in.h; bp.W = in.w;
            bp.act1 = op.act; bp.flags1 = op.flags & FRP_FLAG_BORDER_BIAS; bp.act2 = op2.act;
            bp.n_cu = h->n_cu;
            FRPCHK(launched(h, launch_conv3x3_block64(bp, h->stream), "launch_conv3x3_block64"));
            set_out_dims(d, op, out);
            set_out_dims(d, op2, out);
            charge(op, out, ps.batch, fx);
            charge(op2, out, ps.batch, fx);
            fx.launches -= 1;
            ++i;
            continue;
        }
        ConvParams p = conv_params_for(ps, i, in, d, fused);
        if ((int)i == net.fc_op) pick_fc_splitk(ps, op, in, out, p, fx.fc);
        FRPCHK(launched(h, launch_conv(p, h->stream), "launch_conv"));
        set_out_dims(d, op, out);
        if (hashing && i < 64 && !ps.n_dev)
            FRPCHK(launched(h, launch_tensor_hash(net.bufs[op.out_buf].p, (size_t)ps.batch * out.h * out.w * out.c * (out.f32 ? 4 : 2),
                                                  (unsigned long long*)h->det_hashes.p + i, h->stream), "tensor_hash"));
        charge(op, out, ps.batch, fx);
    }
    return FRP_OK;
}

// The key of a pass in the graph cache: everything the launches depend on that is not fixed by the loaded weights - program, shapes,
// family, operand pointers, the bytes of the switch snapshot; device buffers and weights are covered by the allocation epoch.  Empty: none
std::string graph_key(const NetPass& ps) {
    char kb[512];
    int len = snprintf(kb, sizeof kb, "%c|%d|%d|%d|%d|%p|%p|", ps.net.is_det ? 'd' : 'e', ps.batch, ps.H, ps.W, (int)ps.allow_wino, (const void*)ps.n_dev,
                       (const void*)ps.h->wdata.p);
    if (const StemParams* stem = ps.stem; stem && len > 0 && len < (int)sizeof kb)
        len += snprintf(kb + len, sizeof kb - len, "%p|%d|%d|%d|%ld|%ld|%d|%d|%d", (const void*)stem->frames, stem->B, stem->H, stem->W, stem->row_stride,
                        stem->frame_stride, stem->Hc, stem->Wc, stem->rgb_in);
    if (len <= 0 || len >= (int)sizeof kb) return std::string();
    return std::string(kb, len) + std::string(reinterpret_cast<const char*>(&ps.sw), sizeof ps.sw);
}

// The pass, replayed from its captured graph when it has been asked for before (FRP_NO_GRAPH: always launch by launch).  Not with the
// detector diagnostics (they are not captured).  Either way `fx` holds the effects of exactly one pass.
int launch_or_replay(const NetPass& ps, PassEffects& fx) {
    frp_handle* h = ps.h;
    if (process_switches().no_graph || h->det_hash_on || h->det_op_limit >= 0) return walk(ps, fx);
    const std::string key = graph_key(ps);
    if (key.empty()) return walk(ps, fx);
    for (size_t i = 0; i < h->graphs.size(); ++i) {
        NetGraph& g = h->graphs[i];
        if (g.key != key) continue;
        if (g.epoch != h->alloc_epoch) {            // its buffers may have moved
            (void)hipGraphExecDestroy(g.exec);
            h->graphs.erase(h->graphs.begin() + i);
            break;
        }
        if (hipGraphLaunch(g.exec, h->stream) != hipSuccess) {      // (never seen; if the runtime refuses a replay, the pass is launched instead)
            (void)hipGetLastError();
            (void)hipGraphExecDestroy(g.exec);
            h->graphs.erase(h->graphs.begin() + i);
            h->graph_bad.push_back(key);
            break;
        }
        fx = g.fx;
        h->graph_replays += 1;
        return FRP_OK;
    }
    auto has = [](const std::vector<std::string>& v, const std::string& k) { for (const std::string& x : v) if (x == k) return true; return false; };
    if (has(h->graph_bad, key) || !has(h->graph_seen, key)) {
        if (h->graph_seen.size() > 256) h->graph_seen.clear();
        if (!has(h->graph_seen, key)) h->graph_seen.push_back(key);
        return walk(ps, fx);
    }
    // second request for this pass: capture it (thread-local mode: the other lanes' threads keep allocating and synchronising as they like)
    const uint64_t epoch0 = h->alloc_epoch;
    if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        h->graph_bad.push_back(key);
        return walk(ps, fx);
    }
    const int rc = walk(ps, fx);
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(h->stream, &graph);
    NetGraph g;
    bool ok = rc == FRP_OK && ce == hipSuccess && graph && h->alloc_epoch == epoch0;
    if (ok) ok = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (graph) (void)hipGraphDestroy(graph);
    if (!ok) {
        // nothing of the captured pass has run: say so once, then do it launch by launch (the walk starts `fx` afresh)
        (void)hipGetLastError();
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        h->graph_bad.push_back(key);
        return rc != FRP_OK ? rc : walk(ps, fx);
    }
    g.key = key;
    g.epoch = epoch0;
    g.fx = fx;
    if (h->graphs.size() >= 16) {                  // (two frame buffers x two networks x a few call shapes; the oldest goes)
        (void)hipGraphExecDestroy(h->graphs.front().exec);
        h->graphs.erase(h->graphs.begin());
    }
    const hipError_t le = hipGraphLaunch(g.exec, h->stream);
    h->graphs.push_back(g);
    return launched(h, le, "hipGraphLaunch");
}

}  // namespace

int run_net(frp_handle* h, const Switches& sw, Net& net, int batch, int H, int W, double* flops, int64_t* launches, const StemParams* stem,
            const int32_t* n_dev, bool allow_wino, FcSplitK* fc) {
    const NetPass ps{h, sw, net, batch, H, W, stem, n_dev, allow_wino};
    PassEffects fx;
    FRPCHK(launch_or_replay(ps, fx));
    // the one place where a pass - launched, captured or replayed - leaves its mark on the host side
    *flops += fx.flops;
    *launches += fx.launches;
    h->ctr.f8_conv_flops += fx.f8_flops;
    h->ctr.f8_conv_launches += fx.f8_launches;
    net.dims = std::move(fx.dims);
    if (fc) *fc = fx.fc;
    return FRP_OK;
}

void drop_graphs(frp_handle* h) {
    for (NetGraph& g : h->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    h->graphs.clear();
    h->graph_seen.clear();
    h->graph_bad.clear();
}

}  // namespace frp
