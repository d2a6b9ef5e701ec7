// What the entropy decoders of the JPEG ingest share: the zig-zag order, the flattened canonical Huffman table, and the 64-bit bit window
// with the symbol decode over such a table.  Plain C++ for the host (jpeg_host.cpp, the harnesses under tests/native/) and for the device
// (jpeg_kernels.hip: DevBits, jpeg_selfsync.h: JssBits - they differ in how they REFILL the window).  The host decoder's own reader
// (jpeg_host.cpp: BitReader / HuffTable, 10-bit look-ahead with magnitudes) takes the zig-zag order from here and nothing else.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define JPEG_HD inline
#endif

namespace frp {

// index k of the zig-zag sequence -> position in the 8 x 8 block (T.81 figure A.6)
static constexpr uint8_t kJpegZigZag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Canonical Huffman table in the form the device decoders walk (T.81 F.2.2.3) + a 9-bit look-ahead: (code length << 8) | value, 0 = a
// longer code.  Plain data: built on the host (jpeg_host.cpp: flatten_table), copied to the device as it is.
struct JpegHuffTableDev {
    uint16_t fast[512];
    int32_t mincode[17], maxcode[18], valptr[17];
    uint8_t vals[256];
};

// 64-bit window on a bit stream, left-aligned: the next bit of the stream is bit 63, and the symbol decode over it.  A Reader derives from
// JpegBitWindow<Reader>, feeds bytes in at bit 56 - nbits and keeps at least 32 bits in the window before a symbol (a code is at most 16
// bits, a magnitude at most 15).  Bits are consumed through the READER's skip, so one that tracks more than the window (JssBits: ffm)
// replaces skip and nothing else.
template <class Reader>
struct JpegBitWindow {
    unsigned long long acc;
    int nbits;

    JPEG_HD unsigned peek(int n) const { return (unsigned)(acc >> (64 - n)); }       // 1 <= n <= 32
    JPEG_HD void skip(int n) { acc <<= n; nbits -= n; }
    JPEG_HD int extend(int s) {                                                      // T.81 F.2.2.1, s <= 15
        if (s == 0) return 0;
        const int v = (int)peek(s);
        static_cast<Reader*>(this)->skip(s);
        return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    }
    JPEG_HD int decode(const JpegHuffTableDev& t) {                                  // -> the value, -1 = no such code
        const unsigned f = t.fast[peek(9)];
        if (f) { static_cast<Reader*>(this)->skip((int)(f >> 8)); return (int)(f & 0xff); }
        for (int len = 10; len <= 16; ++len) {
            const int code = (int)peek(len);
            if (t.maxcode[len] >= 0 && code <= t.maxcode[len] && code >= t.mincode[len]) {
                static_cast<Reader*>(this)->skip(len);
                return t.vals[t.valptr[len] + code - t.mincode[len]];
            }
        }
        return -1;
    }
};

}  // namespace frp
