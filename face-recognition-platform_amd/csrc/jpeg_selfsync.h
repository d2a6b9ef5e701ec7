// Self-synchronising parallel Huffman decode of a baseline JPEG scan WITHOUT restart markers: the per-thread
// routines, compiled for the device (jpeg_selfsync.hip) and for the host (tests/native/jpeg_selfsync_harness.cpp runs the same code,
// the grid emulated serially, under the address and undefined-behaviour sanitizers).
//
// The scan of an image is cut into subsequences of S raw bytes.  The decoder's state at a symbol boundary is (p, n, z): p = the bit
// position of the symbol in the RAW scan (8 * byte offset + bit; a position never lies in a stuffed 0x00), n = the block inside
// the MCU (component, hence tables), z = 0 before a DC symbol, else the zig-zag index the next AC symbol continues from.  The DC
// predictor is not part of it: blocks carry DC differences until jss_dc_addr's pass sums them.  jss_decode<false> walks the symbols that
// START inside a subsequence from an entry state and returns the exit state and the blocks it completed: a pure function of
// (entry, bytes), so the chain entry(i + 1) = exit(i) iterated to its fix-point IS the serial decode.  jss_decode<true> is the same walk
// from the final entry state, writing coefficients and reporting what the serial decoder reports (jpeg_host.cpp).
//
// Reads: the bytes [0, n_bytes) of the scan in aligned 8-byte words, so never beyond round_up(n_bytes, 8) - inside the 16-byte slot
// the staging layout gives every scan (jpeg_device_stage_layout).  Bytes at and behind n_bytes count as zeros ("padding").
// The bit window, the symbol decode and the zig-zag order are the ones every entropy decoder here uses: jpeg_entropy.h.
#pragma once
#include <stdint.h>

#include "jpeg_entropy.h"
#include "jpeg_host.h"

namespace frp {

#define JSS_WG 256                       // subsequences (threads) per workgroup
#define JSS_MAX_SCAN (1u << 28)          // scans of this many bytes or more are refused (bit positions stay below 2^31)

// geometry of the images of a batch (they share it): where block j of the scan lies in the coefficient buffer of JpegBatchLayout (both
// device decoders: JpegHuffParams and JpegSelfsyncParams carry one)
struct JssGeom {
    int components, bpm;                 // blocks per MCU (1 .. 6)
    int mcus_x;
    uint32_t total;                      // blocks of an image = mcus_x * mcus_y * bpm
    int hs[3], vs[3], bx[3];             // sampling factors and blocks per row of each component
    long comp_off[3];                    // first coefficient of each component inside an image
    uint8_t comp[8], bv[8], bh[8];       // block n of an MCU: its component, its row and column inside the component's part of the MCU
};

JPEG_HD void jss_geom_blocks(JssGeom& g) {     // comp / bv / bh / bpm from components, hs, vs
    int n = 0;
    for (int c = 0; c < g.components; ++c)
        for (int v = 0; v < g.vs[c]; ++v)
            for (int h = 0; h < g.hs[c]; ++h) {
                if (n < 8) { g.comp[n] = (uint8_t)c; g.bv[n] = (uint8_t)v; g.bh[n] = (uint8_t)h; }
                ++n;
            }
    g.bpm = n;
}

inline JssGeom jss_geom(const frp_jpeg_info& I, const JpegBatchLayout& L) {
    JssGeom g{};
    g.components = I.components;
    g.mcus_x = I.mcus_x;
    for (int c = 0; c < 3; ++c) { g.hs[c] = I.h_samp[c]; g.vs[c] = I.v_samp[c]; g.bx[c] = L.bx[c]; g.comp_off[c] = L.plane_off[c]; }
    jss_geom_blocks(g);
    g.total = (uint32_t)L.blocks_per_image;
    return g;
}

// block j of the scan (MCU j / bpm, block j % bpm of it) -> its first coefficient
JPEG_HD long jss_block_addr(const JssGeom& g, uint32_t j) {
    const uint32_t m = j / (uint32_t)g.bpm;
    const int n = (int)(j - m * (uint32_t)g.bpm), c = g.comp[n];
    const int my = (int)(m / (uint32_t)g.mcus_x), mx = (int)(m - (uint32_t)my * (uint32_t)g.mcus_x);
    return g.comp_off[c] + ((long)(my * g.vs[c] + g.bv[n]) * g.bx[c] + (mx * g.hs[c] + g.bh[n])) * 64;
}
// the k-th block of component c in SCAN order (4:2:0 luma: MCU by MCU, not row by row): the order the DC differences are summed in
JPEG_HD long jss_dc_addr(const JssGeom& g, int c, uint32_t k) {
    const uint32_t per = (uint32_t)(g.hs[c] * g.vs[c]);
    const uint32_t m = k / per;
    const int r = (int)(k - m * per), v = r / g.hs[c], h = r - v * g.hs[c];
    const int my = (int)(m / (uint32_t)g.mcus_x), mx = (int)(m - (uint32_t)my * (uint32_t)g.mcus_x);
    return g.comp_off[c] + ((long)(my * g.vs[c] + v) * g.bx[c] + (mx * g.hs[c] + h)) * 64;
}

// state (p, n, z) in one word: equal words = equal continuations
typedef unsigned long long JssState;
JPEG_HD JssState jss_pack(uint32_t p, int n, int z) { return (JssState)p | ((JssState)(unsigned)n << 32) | ((JssState)(unsigned)z << 40); }
JPEG_HD uint32_t jss_p(JssState s) { return (uint32_t)s; }
JPEG_HD int jss_n(JssState s) { return (int)((s >> 32) & 0xff); }
JPEG_HD int jss_z(JssState s) { return (int)((s >> 40) & 0xff); }

// first byte of subsequence i: i * S, or the byte behind it when that one is the stuffed 0x00 of a 0xFF (inside entropy-coded data
// a 0x00 behind a 0xFF is nothing else).  i == n_sub gives the end of the scan.
JPEG_HD uint32_t jss_start(const uint8_t* scan, uint32_t n_bytes, uint32_t i, uint32_t n_sub, uint32_t S) {
    if (i >= n_sub) return n_bytes;
    const uint32_t o = i * S;
    return (o > 0 && scan[o] == 0x00 && scan[o - 1] == 0xFF) ? o + 1 : o;
}
JPEG_HD uint32_t jss_subsequences(uint32_t n_bytes, uint32_t S) { return n_bytes == 0 ? 1u : (n_bytes + S - 1) / S; }

// Bit reader over the raw scan from an arbitrary bit position.  The 64-bit window and the symbol decode of jpeg_entropy.h (as DevBits of
// jpeg_kernels.hip); `ffm` moves with the window and marks the last bit of every 0xFF data byte, so that the RAW position of the next bit
// can be told at any time: every byte with bits in the window stands for one raw byte, two if it is a 0xFF (its stuffed zero).
struct JssBits : JpegBitWindow<JssBits> {
    const unsigned long long* words;      // the scan, 8-byte aligned
    uint32_t n_bytes;
    uint32_t next;                        // raw offset of the next byte to feed (behind n_bytes: zeros)
    unsigned long long raw;               // bytes fetched but not yet fed (next byte = bits 0..7)
    int rawn;
    unsigned long long ffm;

    JPEG_HD unsigned next_byte() {
        unsigned b = 0;
        if (next < n_bytes) {
            if (rawn == 0) { raw = words[next >> 3]; rawn = 8; }       // (next is a multiple of 8 here: word next / 8 starts inside the scan)
            b = (unsigned)(raw & 0xffu);
            raw >>= 8;
            --rawn;
        }
        ++next;
        return b;
    }
    JPEG_HD void fill() {
        while (nbits <= 56) {
            const unsigned b = next_byte();
            if (b == 0xFF) { (void)next_byte(); ffm |= 1ull << (56 - nbits); }     // its stuffed zero goes with it
            acc |= (unsigned long long)b << (56 - nbits);
            nbits += 8;
        }
    }
    JPEG_HD void init(const uint8_t* scan, uint32_t n, uint32_t p) {
        words = (const unsigned long long*)__builtin_assume_aligned(scan, 8);
        n_bytes = n;
        next = p >> 3;
        raw = 0;
        rawn = 0;
        if (next < n_bytes && (next & 7u)) { raw = words[next >> 3] >> (8 * (next & 7u)); rawn = 8 - (int)(next & 7u); }
        acc = ffm = 0;
        nbits = 0;
        fill();
        skip((int)(p & 7u));
    }
    JPEG_HD void skip(int n) { acc <<= n; ffm <<= n; nbits -= n; }                    // (replaces the window's: ffm moves with acc)
    JPEG_HD uint32_t pos() const {
        const uint32_t bytes = (uint32_t)((nbits + 7) >> 3) + (uint32_t)__builtin_popcountll(ffm);
        return (next - bytes) * 8u + (uint32_t)((8 - (nbits & 7)) & 7);
    }
};

// The symbols that start in [p(entry), end_bit), from `entry`.  WRITE == false (speculation and synchronisation): nothing is stored
// and nothing is an error - an invalid code consumes one bit, a DC size above 11 its code, a run beyond index 63 ends the block -;
// -> exit state, blocks completed.  WRITE == true: the same walk for the blocks from blk0 on that lie below g.total; coefficients
// (natural order, the DC DIFFERENCE at index 0) go to `coef`, which was zeroed; returns non-zero where the serial decoder refuses
// the image: an invalid code, a DC size above 11, an index above 63, or bits consumed behind the end of the scan.
// Every iteration consumes at least one bit, so the loop ends within its budget of end_bit - p(entry) iterations.
template <bool WRITE>
JPEG_HD int jss_decode(const uint8_t* scan, uint32_t n_bytes, const JpegHuffTableDev* tab, const uint8_t* zz, const JssGeom& g, JssState entry,
                       uint32_t end_bit, int16_t* coef, uint32_t blk0, JssState* exit_state, uint32_t* completed) {
    uint32_t p = jss_p(entry), blk = blk0, done = 0;
    int n = jss_n(entry), z = jss_z(entry), bad = 0;
    if (p < end_bit && !(WRITE && blk >= g.total)) {
        JssBits br;
        br.init(scan, n_bytes, p);
        int16_t* dst = WRITE ? coef + jss_block_addr(g, blk) : nullptr;
        const uint32_t scan_bits = n_bytes * 8u;
        for (uint32_t budget = end_bit - p; budget > 0 && p < end_bit; --budget) {
            br.fill();
            const int c = g.comp[n];
            bool block_done = false;
            if (z == 0) {
                const int s = br.decode(tab[2 * c]);
                if (s < 0) { br.skip(1); bad = 1; }
                else if (s > 11) bad = 1;
                else {
                    const int diff = br.extend(s);
                    if (WRITE && diff) dst[0] = (int16_t)diff;
                    z = 1;
                }
            } else {
                const int rs = br.decode(tab[2 * c + 1]);
                if (rs < 0) { br.skip(1); bad = 1; }
                else {
                    const int r = rs >> 4, sz = rs & 15;
                    if (sz == 0) {
                        if (r == 15) { z += 16; block_done = z > 63; }       // (a run of zeros across the block's end ends it: as the serial decoders)
                        else block_done = true;
                    } else if (z + r > 63) { bad = 1; block_done = true; }
                    else {
                        const int v = br.extend(sz);
                        if (WRITE) dst[zz[z + r]] = (int16_t)v;
                        z += r + 1;
                        block_done = z > 63;
                    }
                }
            }
            p = br.pos();
            if (WRITE && (bad || p > scan_bits)) { bad = 1; break; }
            if (block_done) {
                z = 0;
                n = n + 1 == g.bpm ? 0 : n + 1;
                ++done;
                ++blk;
                if (WRITE) {
                    if (blk >= g.total) break;
                    dst = coef + jss_block_addr(g, blk);
                }
            }
        }
    }
    if (exit_state) *exit_state = jss_pack(p, n, z);
    if (completed) *completed = done;
    return WRITE ? bad : 0;
}

}  // namespace frp
