// Host half of the JPEG ingest (jpeg_host.cpp): header parsing + Huffman decoding of baseline JPEG stills, the scan plan of the device
// entropy decoders, the buffer layouts of a batch.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "frp.h"
#include "jpeg_entropy.h"

namespace frp {

size_t jpeg_coef_elems(const frp_jpeg_info& info);
int jpeg_info(const uint8_t* data, size_t size, frp_jpeg_info* out, std::string* err);
// coef: per component [blocks_y][blocks_x][64] int16 (natural order, quantised), components back to back; qtab: [3][64] uint16
int jpeg_decode_coefficients(const uint8_t* data, size_t size, int16_t* coef, size_t coef_elems, uint16_t* qtab, frp_jpeg_info* info,
                             std::string* err);

// What the device entropy decoders need of one image (ingest_api.cpp: plan_entropy_batch): headers parsed as above, the quantisation tables,
// the six Huffman tables flattened (tables6: component c's DC table at 2c, its AC table at 2c + 1) and the scan located by ONE pass over its
// 0xFF bytes.  Which pass, info.restart_interval decides - a caller that takes one kind of scan checks it:
//   with restart intervals   every RSTn marker starts an interval: int_off[n_int + 1], count and RST0..7 sequence checked, FF FF fill
//                            bytes skipped; the scan ends at the first other marker or at the end of the file.  Refused from 0xfffffff0
//                            bytes or 0x7fffff intervals on.
//   without                  int_off stays empty; the scan ends where the host decoder's bit reader stops taking bytes - at the first
//                            0xFF that is not followed by a stuffed 0x00, or at the end of the file -, so both decoders see the same
//                            bytes.  Refused from 2^28 bytes on.
// Fails (FRP_ERR_INVALID) for these and for anything the host decoder's header parser refuses.
struct JpegScanPlan {
    frp_jpeg_info info;
    uint16_t qtab[192];                 // [3][64] natural order
    const uint8_t* scan = nullptr;      // first entropy-coded byte
    size_t scan_bytes = 0;              // up to the marker that ends the scan, or the end of the file
    std::vector<uint32_t> int_off;      // [n_int + 1] offsets from `scan`; empty for a scan without restart intervals
};
int jpeg_plan_scan(const uint8_t* data, size_t size, JpegScanPlan& plan, JpegHuffTableDev* tables6, std::string* err);

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

// Page-locked staging of the device entropy decode: scans (16-byte aligned each, soff[B + 1]) | offsets [B][n_int + 1] u32 |
// Huffman tables [B][6] | quantisation tables, 384 bytes per image | error flags [B] i32 (read back) - every part 256-byte aligned.
// The first o_err bytes go to the device.  too_large: the scans do not fit 32-bit offsets (the batch takes the host decoder).
struct JpegDeviceStageLayout {
    std::vector<size_t> soff;
    size_t o_int, o_tab, o_q, o_err, stage_total;
    bool too_large;
};
FRP_JPEG_LOCAL JpegDeviceStageLayout jpeg_device_stage_layout(int B, long n_int, const size_t* scan_bytes);

}  // namespace frp
