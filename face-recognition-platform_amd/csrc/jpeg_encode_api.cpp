// frp_jpeg_encode_headers, frp_jpeg_optimal_table, frp_encode_jpeg, frp_encode_jpeg_coefficients, frp_encode_jpeg_histograms
// (include/frp.h): baseline JPEG files of rectangles of the resident frames.  The header segments are written here, in PIL's order,
// and so are the optimal Huffman tables of FRP_FLAG_JPEG_OPTIMIZE, from the counts of jpeg_enc_hist_kernel; the scans come from
// jpeg_encode_kernels.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <functional>
#include <queue>

#include "frp.h"
#include "frp_handle.h"

using namespace frp;

namespace {

const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// ITU-T T.81 Annex K.1 / K.2, natural order
const uint8_t kBaseQ[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K.3: BITS and HUFFVAL of the DC / AC tables, luminance then chrominance
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (baseline: 1..255)
void quant_tables(int quality, uint16_t q[2][64]) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) q[t][i] = (uint16_t)std::min(255, std::max(1, (kBaseQ[t][i] * s + 50) / 100));
}

// Annex C: (length << 16) | code per symbol
void huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = ((uint32_t)len << 16) | code++;
        code <<= 1;
    }
}

// BITS / HUFFVAL of one table, as a DHT segment carries them
struct HuffSpec {
    uint8_t bits[16];
    uint8_t vals[256];
    int n;             // symbols
};
// DC0, AC0, DC1, AC1 - the order of the DHT segments
struct HuffSet { HuffSpec t[4]; };

HuffSet annex_k() {
    HuffSet s{};
    for (int i = 0; i < 2; ++i) {
        std::memcpy(s.t[2 * i].bits, kDcBits[i], 16);
        std::memcpy(s.t[2 * i].vals, kDcVals, 12);
        s.t[2 * i].n = 12;
        std::memcpy(s.t[2 * i + 1].bits, kAcBits[i], 16);
        std::memcpy(s.t[2 * i + 1].vals, kAcVals[i], 162);
        s.t[2 * i + 1].n = 162;
    }
    return s;
}

void build_tables(int quality, const HuffSet& s, JpegEncTables& t) {
    std::memset(&t, 0, sizeof(t));
    for (int i = 0; i < 2; ++i) {
        huff_codes(s.t[2 * i].bits, s.t[2 * i].vals, t.dc[i]);
        huff_codes(s.t[2 * i + 1].bits, s.t[2 * i + 1].vals, t.ac[i]);
    }
    quant_tables(quality, t.q);
}

// libjpeg's jpeg_gen_optimal_table, from its definition (T.81 K.2; frp.h: frp_jpeg_optimal_table).  false: all counts zero, or a code
// deeper than 32 bits.  (libjpeg's searches start from a bound of 10^9 and so never pick a larger count; here every count can be
// picked - the two agree below that bound, which no file Pillow can write comes near.)
bool optimal_table(const uint32_t* counts, HuffSpec& out) {
    long long freq[257];
    int codesize[257], others[257], bits[33];
    bool any = false;
    for (int i = 0; i < 256; ++i) {
        freq[i] = counts[i];
        any = any || counts[i];
    }
    if (!any) return false;
    freq[256] = 1;                                            // the pseudo-symbol: no real symbol gets the all-ones code
    for (int i = 0; i < 257; ++i) { codesize[i] = 0; others[i] = -1; }
    // libjpeg finds the two least frequent entries by two linear searches with `<=` (ties go to the larger index, the second search
    // skips the first's pick): the same two entries leave a heap ordered by (count, larger index first) - a call with hundreds of
    // crops makes over a thousand tables, and the searches were most of its time
    typedef std::pair<long long, int> Entry;                  // (count, -index): the smallest pair is the next pick
    std::vector<Entry> entries;
    entries.reserve(257);
    for (int i = 0; i <= 256; ++i)
        if (freq[i]) entries.push_back(Entry(freq[i], -i));
    std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> live(std::greater<Entry>(), std::move(entries));
    while (live.size() > 1) {
        int c1 = -live.top().second;
        live.pop();
        int c2 = -live.top().second;
        live.pop();
        freq[c1] += freq[c2];
        freq[c2] = 0;
        live.push(Entry(freq[c1], -c1));
        for (++codesize[c1]; others[c1] >= 0;) { c1 = others[c1]; ++codesize[c1]; }
        others[c1] = c2;                                      // chain c2's tree behind c1's
        for (++codesize[c2]; others[c2] >= 0;) { c2 = others[c2]; ++codesize[c2]; }
    }
    std::memset(bits, 0, sizeof(bits));
    int first[34] = {0};                                      // HUFFVAL is the symbols by (unlimited) code length, then by value:
    for (int i = 0; i <= 256; ++i) {                          // first[len] = symbols with shorter codes (a counting sort)
        if (codesize[i] > 32) return false;
        if (codesize[i]) ++bits[codesize[i]];
        if (codesize[i] && i < 256) ++first[codesize[i] + 1];
    }
    for (int len = 1; len <= 33; ++len) first[len] += first[len - 1];
    for (int i = 32; i > 16; --i)                             // Figure K.3: no code longer than 16
        while (bits[i] > 0) {
            int j = i - 2;
            while (bits[j] == 0) --j;
            bits[i] -= 2; ++bits[i - 1];
            bits[j + 1] += 2; --bits[j];
        }
    int last = 16;
    while (bits[last] == 0) --last;
    --bits[last];                                             // the pseudo-symbol leaves: it had the longest code
    out = HuffSpec{};
    for (int i = 1; i <= 16; ++i) out.bits[i - 1] = (uint8_t)bits[i];
    for (int j = 0; j < 256; ++j)
        if (codesize[j]) {
            out.vals[first[codesize[j]]++] = (uint8_t)j;
            ++out.n;
        }
    return true;
}

// the four tables of one image from its symbol counts (JE_HIST_BINS: dc [2][16], ac [2][256])
bool optimal_set(const uint32_t* hist, HuffSet& s) {
    for (int i = 0; i < 2; ++i) {
        uint32_t dc[256] = {0};
        std::memcpy(dc, hist + 16 * i, 16 * sizeof(uint32_t));
        if (!optimal_table(dc, s.t[2 * i]) || !optimal_table(hist + 32 + 256 * i, s.t[2 * i + 1])) return false;
    }
    return true;
}

bool sampling_ok(int subsampling, int& hs, int& vs) {
    if (subsampling == FRP_JPEG_420) { hs = vs = 2; return true; }
    if (subsampling == FRP_JPEG_444) { hs = vs = 1; return true; }
    return false;
}

struct Seg {           // appends big-endian segments
    std::vector<uint8_t> b;
    void u8(int v) { b.push_back((uint8_t)v); }
    void u16(int v) { u8(v >> 8); u8(v & 255); }
    void marker(int m, int payload) { u8(0xFF); u8(m); u16(payload + 2); }
};

// SOI, APP0 (JFIF 1.01, no density), DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1, DRI when restart_mcus > 0, SOS; the DHT segments carry
// the tables of `huff`: their length is the image's own
std::vector<uint8_t> headers(int width, int height, int quality, int hs, int vs, int restart_mcus, const HuffSet& huff) {
    Seg s;
    s.u8(0xFF); s.u8(0xD8);
    s.marker(0xE0, 14);
    for (char c : {'J', 'F', 'I', 'F'}) s.u8(c);
    s.u8(0); s.u8(1); s.u8(1); s.u8(0); s.u16(1); s.u16(1); s.u8(0); s.u8(0);
    uint16_t q[2][64];
    quant_tables(quality, q);
    for (int t = 0; t < 2; ++t) {
        s.marker(0xDB, 65);
        s.u8(t);
        for (int i = 0; i < 64; ++i) s.u8(q[t][kZigzag[i]]);
    }
    s.marker(0xC0, 15);
    s.u8(8); s.u16(height); s.u16(width); s.u8(3);
    s.u8(1); s.u8((hs << 4) | vs); s.u8(0);
    s.u8(2); s.u8(0x11); s.u8(1);
    s.u8(3); s.u8(0x11); s.u8(1);
    for (int t = 0; t < 4; ++t) {
        const HuffSpec& hf = huff.t[t];
        s.marker(0xC4, 1 + 16 + hf.n);
        s.u8(((t & 1) << 4) | (t >> 1));                     // class (0: DC, 1: AC), table
        for (int i = 0; i < 16; ++i) s.u8(hf.bits[i]);
        for (int i = 0; i < hf.n; ++i) s.u8(hf.vals[i]);
    }
    if (restart_mcus > 0) {
        s.marker(0xDD, 2);
        s.u16(restart_mcus);
    }
    s.marker(0xDA, 10);
    s.u8(3); s.u8(1); s.u8(0x00); s.u8(2); s.u8(0x11); s.u8(3); s.u8(0x11); s.u8(0); s.u8(63); s.u8(0);
    return s.b;
}

// ... with the Annex K tables
std::vector<uint8_t> headers(int width, int height, int quality, int hs, int vs, int restart_mcus) {
    return headers(width, height, quality, hs, vs, restart_mcus, annex_k());
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// the checks of the encoder's own arguments, shared by every entry point
int check_args(frp_handle* h, const std::string& w, int quality, int subsampling, int restart_mcus, int& hs, int& vs) {
    if (quality < 1 || quality > 100) return fail(h, FRP_ERR_INVALID, w + ": quality outside 1..100");
    if (!sampling_ok(subsampling, hs, vs)) return fail(h, FRP_ERR_INVALID, w + ": subsampling is neither FRP_JPEG_420 nor FRP_JPEG_444");
    if (restart_mcus < 0 || restart_mcus > 65535) return fail(h, FRP_ERR_INVALID, w + ": restart_mcus outside 0..65535");
    return FRP_OK;
}

// the images' MCU grids and their places among the blocks and intervals of the call
int layout(frp_handle* h, const std::string& w, const JpegEncSource* src, int32_t n, int hs, int vs, int restart_mcus, uint32_t flags,
           std::vector<JpegEncImage>& img, JpegEncParams& p) {
    img.resize((size_t)n);
    long long blocks = 0, ints = 0;
    for (int32_t i = 0; i < n; ++i) {
        JpegEncImage& I = img[(size_t)i];
        I = JpegEncImage{};
        I.pix0 = src[i].pix0; I.pitch = src[i].pitch; I.h = src[i].h; I.w = src[i].w;
        I.mx = (I.w + 8 * hs - 1) / (8 * hs);
        I.my = (I.h + 8 * vs - 1) / (8 * vs);
        const long long mcus = (long long)I.mx * I.my;
        I.n_int = restart_mcus ? (int)((mcus + restart_mcus - 1) / restart_mcus) : 1;
        I.int0 = (int)ints;
        I.blk0 = blocks;
        blocks += mcus * (hs * vs + 2);
        ints += I.n_int;
        if (blocks >= (1LL << 26) || ints >= (1LL << 26)) return fail(h, FRP_ERR_INVALID, w + ": more than 2^26 blocks or restart intervals in one call");
    }
    p = JpegEncParams{};
    p.rgb_in = (flags & FRP_FLAG_RGB) ? 1 : 0;
    p.n = n;
    p.hs = hs; p.vs = vs;
    p.ri = restart_mcus;
    p.n_blocks = blocks;
    p.n_int = ints;
    return FRP_OK;
}

// validation + geometry of rectangles of the resident frames; FRP_OK with n == 0 means: nothing to do
int plan(frp_handle* h, const char* who, const int32_t* rects, int32_t n, int quality, int subsampling, int restart_mcus, uint32_t flags,
         uint32_t allowed, std::vector<JpegEncImage>& img, JpegEncParams& p) {
    const std::string w(who);
    if (h->rB <= 0 || !h->frames.p) return fail(h, FRP_ERR_INVALID, w + ": no resident frames");
    if (n < 0) return fail(h, FRP_ERR_INVALID, w + ": n < 0");
    if (flags & ~allowed)
        return fail(h, FRP_ERR_INVALID, w + ": flags other than FRP_FLAG_RGB" + ((allowed & FRP_FLAG_JPEG_OPTIMIZE) ? " and FRP_FLAG_JPEG_OPTIMIZE" : ""));
    int hs = 0, vs = 0;
    FRPCHK(check_args(h, w, quality, subsampling, restart_mcus, hs, vs));
    if (n == 0) return FRP_OK;
    if (!rects) return fail(h, FRP_ERR_INVALID, w + ": null rects");
    std::vector<JpegEncSource> src((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        FRPCHK(jpeg_enc_check_rect(h, w, rects, i));
        const int32_t *r = rects + (size_t)i * 5;
        src[(size_t)i] = JpegEncSource{((long long)r[0] * h->rH + r[1]) * h->rW + r[4], h->rW, r[2] - r[4], r[3] - r[1]};
    }
    FRPCHK(layout(h, w, src.data(), n, hs, vs, restart_mcus, flags, img, p));
    p.frames = (const uint8_t*)h->frames.p;
    p.total_bytes = (long long)h->rB * h->rH * h->rW * 3;
    return FRP_OK;
}

// rectangles + tables (+ room for the scans' places; `hist`: and for every image's symbol counts and its own tables, p.hist) to the
// device, the coefficient buffer; queues the forward half
int forward(frp_handle* h, const std::vector<JpegEncImage>& img, int quality, JpegEncParams& p, std::vector<uint8_t>& up, bool hist = false) {
    const size_t img_bytes = align16(img.size() * sizeof(JpegEncImage)), tab_bytes = align16(sizeof(JpegEncTables));
    const size_t base_bytes = img_bytes + tab_bytes + align16(img.size() * sizeof(unsigned long long));
    const size_t hist_bytes = hist ? align16(img.size() * JE_HIST_BINS * sizeof(uint32_t)) : 0;
    up.assign(img_bytes + tab_bytes, 0);
    std::memcpy(up.data(), img.data(), img.size() * sizeof(JpegEncImage));
    JpegEncTables t;
    build_tables(quality, annex_k(), t);
    std::memcpy(up.data() + img_bytes, &t, sizeof(t));
    FRPCHK(ensure(h, h->jenc_in, base_bytes + hist_bytes + (hist ? img.size() * sizeof(JpegEncTables) : 0)));
    FRPCHK(ensure(h, h->jenc_coef, (size_t)p.n_blocks * 64 * sizeof(int16_t)));
    uint8_t* in = (uint8_t*)h->jenc_in.p;
    p.img = (const JpegEncImage*)in;
    p.tab = (const JpegEncTables*)(in + img_bytes);
    p.tab_stride = 0;
    p.hist = hist ? (uint32_t*)(in + base_bytes) : nullptr;
    p.scan_base = (const unsigned long long*)(in + img_bytes + tab_bytes);
    p.coef = (int16_t*)h->jenc_coef.p;
    HIPCHK(h, hipMemcpyAsync(h->jenc_in.p, up.data(), up.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_jpeg_enc_forward(p, h->stream));
    return FRP_OK;
}

// after a failed step: nothing of this call stays queued behind the caller's buffers
int drain(frp_handle* h, int rc) {
    (void)hipStreamSynchronize(h->stream);
    settle_events(h, true);
    return rc;
}

// behind the forward half (queued with room for them: forward(..., hist = true)): the images' symbol counts -> counts [n][JE_HIST_BINS]; waits
int histograms(frp_handle* h, const std::string& w, JpegEncParams& p, std::vector<uint32_t>& counts) {
    counts.assign((size_t)p.n * JE_HIST_BINS, 0);
    hipError_t e = hipMemsetAsync(p.hist, 0, counts.size() * sizeof(uint32_t), h->stream);
    if (e == hipSuccess) e = launch_jpeg_enc_hist(p, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(counts.data(), p.hist, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
    const hipError_t e2 = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, w + " histograms: " + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(h, FRP_ERR_HIP, w + " histograms sync: " + hipGetErrorString(e2));
    return FRP_OK;
}

// a count is at most 63 per block (ZRL and the AC symbols of a block together): it has to fit uint32
int check_hist_range(frp_handle* h, const std::string& w, const std::vector<JpegEncImage>& img, const JpegEncParams& p) {
    for (size_t i = 0; i < img.size(); ++i)
        if ((unsigned long long)img[i].mx * img[i].my * (p.hs * p.vs + 2) * 63ull > 0xFFFFFFFFull)
            return fail(h, FRP_ERR_INVALID, w + ": image " + std::to_string(i) + " has too many blocks for 32-bit symbol counts");
    return FRP_OK;
}

// the planned images (p.frames / p.total_bytes: their buffer) -> the files in out; waits.  optimize: every image with Huffman tables
// of its own - histogram kernel, one more copy and wait, the tables made here and uploaded, then the same entropy stage
int files(frp_handle* h, const std::string& w, const std::vector<JpegEncImage>& img, JpegEncParams& p, int quality, bool optimize, uint8_t* out,
          int64_t out_cap, int64_t* offsets) {
    std::vector<uint8_t> up;
    const int32_t n = p.n;
    const int restart_mcus = p.ri;
    if (optimize) FRPCHK(check_hist_range(h, w, img, p));
    FRPCHK(forward(h, img, quality, p, up, optimize));
    std::vector<HuffSet> huff;                              // per image (optimize); empty: Annex K's for all
    std::vector<JpegEncTables> tabs;                        // (read by the upload until the next wait)
    if (optimize) {
        std::vector<uint32_t> counts;
        const int hrc = histograms(h, w, p, counts);
        if (hrc != FRP_OK) return drain(h, hrc);
        huff.resize((size_t)n);
        tabs.resize((size_t)n);
        for (int32_t i = 0; i < n; ++i) {
            if (!optimal_set(counts.data() + (size_t)i * JE_HIST_BINS, huff[(size_t)i]))
                return drain(h, fail(h, FRP_ERR_HIP, w + ": implausible symbol counts for image " + std::to_string(i)));
            build_tables(quality, huff[(size_t)i], tabs[(size_t)i]);
        }
        JpegEncTables* dev = (JpegEncTables*)(p.hist + align16((size_t)n * JE_HIST_BINS * sizeof(uint32_t)) / sizeof(uint32_t));
        hipError_t e = hipMemcpyAsync(dev, tabs.data(), tabs.size() * sizeof(JpegEncTables), hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) return drain(h, fail(h, FRP_ERR_HIP, w + " tables: " + hipGetErrorString(e)));
        p.tab = dev;
        p.tab_stride = 1;
    }
    // the work arrays of the entropy half, carved out of one allocation
    const size_t nb = (size_t)p.n_blocks, ni = (size_t)p.n_int;
    const size_t groups = jpeg_enc_scan_groups((long long)std::max(nb, ni)) + 64;      // (the 0xFF chunks are fewer than the blocks: see n_words)
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off += align16(bytes); return at; };
    const size_t o_bits = carve(nb * 4), o_pre = carve((nb + 1) * 8), o_grp = carve(groups * 8), o_iw = carve((ni + 1) * 8), o_ib = carve(ni * 4),
                 o_if = carve(ni * 8), o_io = carve(ni * 4), o_ip = carve((ni + 1) * 8), o_img = carve(((size_t)n + 1) * 8);
    int rc = ensure(h, h->jenc_work, off);
    if (rc != FRP_OK) return drain(h, rc);                  // (the uploads above read this frame's vectors)
    uint8_t* wk = (uint8_t*)h->jenc_work.p;
    p.blk_bits = (uint32_t*)(wk + o_bits);
    p.bit_prefix = (unsigned long long*)(wk + o_pre);
    p.group_tot = (unsigned long long*)(wk + o_grp);
    p.int_word = (unsigned long long*)(wk + o_iw);
    p.int_bytes = (uint32_t*)(wk + o_ib);
    p.int_ff0 = (unsigned long long*)(wk + o_if);
    p.int_outb = (uint32_t*)(wk + o_io);
    p.int_out = (unsigned long long*)(wk + o_ip);
    p.img_off = (unsigned long long*)(wk + o_img);
    // 1. bits per block and their prefix sums: the size of the unstuffed stream
    unsigned long long total_bits = 0;
    hipError_t e = launch_jpeg_enc_measure(p, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&total_bits, p.bit_prefix + nb, sizeof(total_bits), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return drain(h, fail(h, FRP_ERR_HIP, w + " measure: " + hipGetErrorString(e)));
    // a block codes at most 20 + 63 * 26 bits with Annex K's tables (a DC code of 9 bits + 11 magnitude bits; per AC coefficient a
    // code of 16 + 10 - a ZRL covers 16 coefficients with at most 16 bits), 27 + 63 * 26 with tables whose DC codes may take 16 bits:
    // anything beyond that is not a size
    if (total_bits > (unsigned long long)nb * (optimize ? 1665ull : 1658ull)) return drain(h, fail(h, FRP_ERR_HIP, w + ": implausible bit count"));
    // 2. the stream in words (every interval starts on a word of its own), 0xFF counts per chunk, the intervals' places
    p.n_words = (total_bits >> 5) + ni + 1;
    p.n_chunks = (long long)((p.n_words + JE_CHUNK_WORDS - 1) / JE_CHUNK_WORDS);
    if (jpeg_enc_scan_groups(p.n_chunks) > groups) return drain(h, fail(h, FRP_ERR_INVALID, w + ": stream too long"));
    const size_t words_bytes = align16((size_t)p.n_words * 4), chunk_bytes = align16((size_t)p.n_chunks * 4);
    rc = ensure(h, h->jenc_bits, words_bytes + chunk_bytes + align16(((size_t)p.n_chunks + 1) * 8));
    if (rc != FRP_OK) return drain(h, rc);
    uint8_t* bw = (uint8_t*)h->jenc_bits.p;
    p.words = (uint32_t*)bw;
    p.ff_chunk = (uint32_t*)(bw + words_bytes);
    p.ff_prefix = (unsigned long long*)(bw + words_bytes + chunk_bytes);
    std::vector<unsigned long long> scan_off((size_t)n + 1);
    e = hipMemsetAsync(p.words, 0, words_bytes, h->stream);
    if (e == hipSuccess) e = launch_jpeg_enc_pack(p, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(scan_off.data(), p.img_off, scan_off.size() * 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return drain(h, fail(h, FRP_ERR_HIP, w + " pack: " + hipGetErrorString(e)));
    // 3. the files' places: headers + scan + EOI each
    std::vector<std::vector<uint8_t>> hdr((size_t)n);
    std::vector<unsigned long long> scan_base((size_t)n);
    int64_t at = 0;
    for (int32_t i = 0; i < n; ++i) {
        hdr[(size_t)i] = optimize ? headers(img[(size_t)i].w, img[(size_t)i].h, quality, p.hs, p.vs, restart_mcus, huff[(size_t)i])
                                  : headers(img[(size_t)i].w, img[(size_t)i].h, quality, p.hs, p.vs, restart_mcus);
        const unsigned long long scan = scan_off[(size_t)i + 1] - scan_off[(size_t)i];
        // stuffing at most doubles a stream, and every interval adds a marker: anything beyond that is not a size
        if (scan_off[(size_t)i + 1] < scan_off[(size_t)i] || scan > 2ull * ((total_bits >> 3) + 4ull * ni) + 16)
            return drain(h, fail(h, FRP_ERR_HIP, w + ": implausible scan size"));
        offsets[i] = at;
        scan_base[(size_t)i] = (unsigned long long)at + hdr[(size_t)i].size();
        at += (int64_t)(hdr[(size_t)i].size() + scan + 2);
    }
    offsets[n] = at;
    if (at > out_cap) return drain(h, fail(h, FRP_ERR_INVALID, w + ": the files take " + std::to_string(at) + " bytes, out_cap is " + std::to_string(out_cap)));
    if (!out) return drain(h, fail(h, FRP_ERR_INVALID, w + ": null out"));
    rc = ensure(h, h->jenc_out, (size_t)at);
    if (rc != FRP_OK) return drain(h, rc);
    p.out = (uint8_t*)h->jenc_out.p;
    p.out_bytes = (unsigned long long)at;
    e = hipMemcpyAsync((void*)p.scan_base, scan_base.data(), scan_base.size() * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = launch_jpeg_enc_emit(p, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, p.out, (size_t)at, hipMemcpyDeviceToHost, h->stream);
    hipError_t e2 = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return drain(h, fail(h, FRP_ERR_HIP, w + " emit: " + hipGetErrorString(e)));
    if (e2 != hipSuccess) return drain(h, fail(h, FRP_ERR_HIP, w + " sync: " + hipGetErrorString(e2)));
    for (int32_t i = 0; i < n; ++i) {                        // the host's part of every file: what precedes the scan, and EOI
        std::memcpy(out + offsets[i], hdr[(size_t)i].data(), hdr[(size_t)i].size());
        out[offsets[i + 1] - 2] = 0xFF;
        out[offsets[i + 1] - 1] = 0xD9;
    }
    settle_events(h, true);
    return FRP_OK;
}

int encode(frp_handle* h, const int32_t* rects, int32_t n, int quality, int subsampling, int restart_mcus, uint32_t flags, uint8_t* out,
           int64_t out_cap, int64_t* offsets) {
    std::vector<JpegEncImage> img;
    JpegEncParams p;
    FRPCHK(plan(h, "encode_jpeg", rects, n, quality, subsampling, restart_mcus, flags, FRP_FLAG_RGB | FRP_FLAG_JPEG_OPTIMIZE, img, p));
    if (out_cap < 0) return fail(h, FRP_ERR_INVALID, "encode_jpeg: out_cap < 0");
    if (!offsets) return fail(h, FRP_ERR_INVALID, "encode_jpeg: null offsets");
    if (n == 0) {
        offsets[0] = 0;
        return FRP_OK;
    }
    return files(h, "encode_jpeg", img, p, quality, (flags & FRP_FLAG_JPEG_OPTIMIZE) != 0, out, out_cap, offsets);
}

}  // namespace

namespace frp {

int jpeg_enc_check_rect(frp_handle* h, const std::string& w, const int32_t* rects, int32_t i) {
    const int32_t *r = rects + (size_t)i * 5, f = r[0], top = r[1], right = r[2], bottom = r[3], left = r[4];
    if (!(f >= 0 && f < h->rB && top >= 0 && top < bottom && bottom <= h->rH && left >= 0 && left < right && right <= h->rW) ||
        bottom - top > 65535 || right - left > 65535)
        return fail(h, FRP_ERR_INVALID, w + ": rectangle " + std::to_string(i) + " (frame " + std::to_string(f) + ", top " +
                    std::to_string(top) + ", right " + std::to_string(right) + ", bottom " + std::to_string(bottom) + ", left " +
                    std::to_string(left) + ") is empty or outside the " + std::to_string(h->rB) + " resident frames of " +
                    std::to_string(h->rH) + " x " + std::to_string(h->rW));
    return FRP_OK;
}

int jpeg_enc_plan_buffer(frp_handle* h, const std::string& who, const JpegEncSource* src, int32_t n, int quality, int subsampling, int restart_mcus,
                         uint32_t flags, std::vector<JpegEncImage>& img, JpegEncParams& p) {
    int hs = 0, vs = 0;
    FRPCHK(check_args(h, who, quality, subsampling, restart_mcus, hs, vs));
    return layout(h, who, src, n, hs, vs, restart_mcus, flags, img, p);
}

int jpeg_enc_files(frp_handle* h, const std::string& who, const std::vector<JpegEncImage>& img, JpegEncParams& p, int quality, bool optimize,
                   uint8_t* out, int64_t out_cap, int64_t* offsets) {
    return files(h, who, img, p, quality, optimize, out, out_cap, offsets);
}

}  // namespace frp

extern "C" {

int64_t frp_jpeg_encode_headers(int32_t width, int32_t height, int32_t quality, int32_t subsampling, int32_t restart_mcus, uint8_t* out, int64_t cap) {
    int hs = 0, vs = 0;
    if (width < 1 || width > 65535 || height < 1 || height > 65535 || quality < 1 || quality > 100 || !sampling_ok(subsampling, hs, vs) ||
        restart_mcus < 0 || restart_mcus > 65535 || !out || cap < 0)
        return FRP_ERR_INVALID;
    const std::vector<uint8_t> b = headers(width, height, quality, hs, vs, restart_mcus);
    if ((int64_t)b.size() > cap) return FRP_ERR_INVALID;
    std::memcpy(out, b.data(), b.size());
    return (int64_t)b.size();
}

int frp_jpeg_optimal_table(const uint32_t freq[256], uint8_t bits[16], uint8_t vals[256]) {
    if (!freq || !bits || !vals) return FRP_ERR_INVALID;
    HuffSpec s;
    if (!optimal_table(freq, s)) return FRP_ERR_INVALID;
    std::memcpy(bits, s.bits, 16);
    std::memcpy(vals, s.vals, (size_t)s.n);
    return s.n;
}

int frp_encode_jpeg(frp_handle* h, const int32_t* rects, int32_t n, int32_t quality, int32_t subsampling, int32_t restart_mcus, uint32_t flags,
                    uint8_t* out, int64_t out_cap, int64_t* offsets) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);      // queued behind whatever pass is pending; its stage events are read after this call's own wait
    return encode(h, rects, n, quality, subsampling, restart_mcus, flags, out, out_cap, offsets);
}

int frp_encode_jpeg_coefficients(frp_handle* h, const int32_t* rects, int32_t n, int32_t quality, int32_t subsampling, uint32_t flags,
                                 int16_t* coef, int64_t coef_elems) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    std::vector<JpegEncImage> img;
    std::vector<uint8_t> up;
    JpegEncParams p;
    FRPCHK(plan(h, "encode_jpeg_coefficients", rects, n, quality, subsampling, 0, flags, FRP_FLAG_RGB, img, p));
    if (n == 0) return FRP_OK;
    if (!coef || coef_elems != p.n_blocks * 64)
        return fail(h, FRP_ERR_INVALID, "encode_jpeg_coefficients: the rectangles have " + std::to_string(p.n_blocks * 64) + " coefficients, coef_elems is " +
                    std::to_string(coef_elems));
    FRPCHK(forward(h, img, quality, p, up));
    hipError_t e = hipMemcpyAsync(coef, p.coef, (size_t)coef_elems * sizeof(int16_t), hipMemcpyDeviceToHost, h->stream);
    hipError_t e2 = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("encode_jpeg_coefficients: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(h, FRP_ERR_HIP, std::string("encode_jpeg_coefficients sync: ") + hipGetErrorString(e2));
    settle_events(h, true);
    return FRP_OK;
}

int frp_encode_jpeg_histograms(frp_handle* h, const int32_t* rects, int32_t n, int32_t quality, int32_t subsampling, int32_t restart_mcus,
                               uint32_t flags, uint32_t* hist, int64_t hist_elems) {
    if (!h) return FRP_ERR_INVALID;
    Guard g(h, false);
    const std::string w("encode_jpeg_histograms");
    std::vector<JpegEncImage> img;
    std::vector<uint8_t> up;
    JpegEncParams p;
    FRPCHK(plan(h, w.c_str(), rects, n, quality, subsampling, restart_mcus, flags, FRP_FLAG_RGB | FRP_FLAG_JPEG_OPTIMIZE, img, p));
    if (n == 0) return FRP_OK;
    if (!hist || hist_elems != (int64_t)n * JE_HIST_BINS)
        return fail(h, FRP_ERR_INVALID, w + ": " + std::to_string(n) + " images have " + std::to_string((int64_t)n * JE_HIST_BINS) + " counts, hist_elems is " +
                    std::to_string(hist_elems));
    FRPCHK(check_hist_range(h, w, img, p));
    FRPCHK(forward(h, img, quality, p, up, true));
    std::vector<uint32_t> counts;
    const int rc = histograms(h, w, p, counts);           // (waits on its error paths too: `up` lives long enough)
    settle_events(h, true);
    if (rc != FRP_OK) return rc;
    std::memcpy(hist, counts.data(), counts.size() * sizeof(uint32_t));
    return FRP_OK;
}

}  // extern "C"
