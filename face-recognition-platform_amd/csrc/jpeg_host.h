// Host half of the JPEG ingest (jpeg_host.cpp): header parsing + Huffman decoding of baseline JPEG stills, the buffer layouts of a batch.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "frp.h"

namespace frp {

size_t jpeg_coef_elems(const frp_jpeg_info& info);
int jpeg_info(const uint8_t* data, size_t size, frp_jpeg_info* out, std::string* err);
// coef: per component [blocks_y][blocks_x][64] int16 (natural order, quantised), components back to back; qtab: [3][64] uint16
int jpeg_decode_coefficients(const uint8_t* data, size_t size, int16_t* coef, size_t coef_elems, uint16_t* qtab, frp_jpeg_info* info,
                             std::string* err);

// What the device entropy decoder needs of one image (frp_upload_jpeg_async's device path): headers parsed as above, the scan
// located, the restart markers found and checked (count and RST0..7 sequence).  Fails (FRP_ERR_INVALID) for files without
// restart intervals and for anything the host decoder refuses.
// Canonical Huffman table in the form both decoders walk (T.81 F.2.2.3) + a 9-bit look-ahead: (code length << 8) | value, 0 = a
// longer code.  (Plain data: shared with the device code through frp_internal.h.)
struct JpegHuffTableDev {
    uint16_t fast[512];
    int32_t mincode[17], maxcode[18], valptr[17];
    uint8_t vals[256];
};
struct JpegDevicePlan {
    frp_jpeg_info info;
    uint16_t qtab[192];                 // [3][64] natural order
    const uint8_t* scan = nullptr;      // first entropy-coded byte
    size_t scan_bytes = 0;              // up to the end of the last interval (the marker behind it, or the end of the file)
    std::vector<uint32_t> int_off;      // [n_int + 1] offsets from `scan`
};
int jpeg_plan_device_decode(const uint8_t* data, size_t size, JpegDevicePlan& plan, JpegHuffTableDev* tables6, std::string* err);

// What the self-synchronising device decoder needs of one image WITHOUT restart intervals (frp_upload_jpeg_async's second device path,
// jpeg_selfsync.h): headers, the six tables and the quantisation tables as above; the scan ends where the host decoder's bit reader stops
// taking bytes - at the first 0xFF that is not followed by a stuffed 0x00, or at the end of the file -, so both decoders see the same
// bytes.  Fails (FRP_ERR_INVALID) for files with restart intervals, for scans of 2^28 bytes or more and for what the host decoder refuses.
struct JpegSelfsyncPlan {
    frp_jpeg_info info;
    uint16_t qtab[192];                 // [3][64] natural order
    const uint8_t* scan = nullptr;      // first entropy-coded byte
    size_t scan_bytes = 0;
};
int jpeg_plan_selfsync_decode(const uint8_t* data, size_t size, JpegSelfsyncPlan& plan, JpegHuffTableDev* tables6, std::string* err);

#define FRP_JPEG_LOCAL __attribute__((visibility("hidden")))   // for ingest_api.cpp and the test harness: not among the library's exports

// Where a batch of B images of one geometry lies (frp_upload_jpeg_async; plain arithmetic on header fields, so the sanitizer harness
// reaches it).  Coefficient staging, the same on the host and on the device: [B][coef_elems] int16, then at q_off (256-byte aligned)
// [B][3][64] uint16 quantisation tables; `total` bytes in all.  Sample planes of the pixel kernels: per image the components back to
// back (plane_off, plane_img bytes per image), bx x by blocks each (whole MCUs); cw x ch = real extent of the chroma planes.
struct JpegBatchLayout {
    size_t coef_elems, coef_bytes, q_off, total;
    int bx[3], by[3];
    long plane_off[3], plane_img;
    int blocks_per_image, cw, ch;
};
FRP_JPEG_LOCAL JpegBatchLayout jpeg_batch_layout(const frp_jpeg_info& info, int B);

// Page-locked staging of the device entropy decode: scans (16-byte aligned each, soff[B + 1]) | interval offsets [B][n_int + 1] u32 |
// Huffman tables [B][6] | quantisation tables, 384 bytes per image | error flags [B] i32 (read back) - every part 256-byte aligned.
// The first o_err bytes go to the device.  too_large: the scans do not fit 32-bit offsets (the batch takes the host decoder).
struct JpegDeviceStageLayout {
    std::vector<size_t> soff;
    size_t o_int, o_tab, o_q, o_err, stage_total;
    bool too_large;
};
FRP_JPEG_LOCAL JpegDeviceStageLayout jpeg_device_stage_layout(int B, long n_int, const size_t* scan_bytes);

}  // namespace frp
