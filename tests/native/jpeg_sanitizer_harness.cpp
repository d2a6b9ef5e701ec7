// Sanitizer harness of the JPEG host decoder (csrc/jpeg_host.cpp, plain C++: no HIP): built by tests/test_jpeg.py with
// g++ -fsanitize=address,undefined and run over a corpus of damaged files.  Every input is copied into a heap block of EXACTLY its
// size (so a read one byte past the file is a heap-buffer-overflow report, not a lucky zero), parsed, and - if the headers pass -
// entropy-decoded into an exactly sized coefficient buffer; for every file that decodes, the buffer layouts of a batch of such images
// are checked too.  Prints one summary line; exits non-zero only through a sanitizer report or a layout violation.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "frp.h"
#include "jpeg_host.h"

// The buffer layouts of a batch of B such images (jpeg_batch_layout, jpeg_device_stage_layout): the parts in order, none overlapping
// the next, each at its alignment, the last one ending at the total, and no product wrapping.  A violation ends the run non-zero.
#define LAYOUT_CHECK(cond)                                                                            \
    do {                                                                                              \
        if (!(cond)) { fprintf(stderr, "%s: B %d: layout check failed: %s\n", path, B, #cond); exit(3); } \
    } while (0)

static void check_layouts(const char* path, const frp_jpeg_info& info, const frp::JpegScanPlan* plan, size_t file_bytes) {
    for (int B : {1, 3, 32}) {
        const frp::JpegBatchLayout L = frp::jpeg_batch_layout(info, B);
        const unsigned __int128 b = (unsigned)B;
        LAYOUT_CHECK(L.coef_elems == frp::jpeg_coef_elems(info));
        LAYOUT_CHECK(b * L.coef_elems * 2 == L.coef_bytes);                              // (no wrap)
        LAYOUT_CHECK(L.q_off >= L.coef_bytes && L.q_off - L.coef_bytes < 256 && L.q_off % 256 == 0);
        LAYOUT_CHECK(L.total == L.q_off + (size_t)B * 384 && L.total > L.q_off);
        long end = 0;
        int blocks = 0;
        for (int c = 0; c < info.components; ++c) {
            LAYOUT_CHECK(L.bx[c] > 0 && L.by[c] > 0 && L.plane_off[c] == end && L.plane_off[c] % 8 == 0);
            LAYOUT_CHECK((__int128)L.bx[c] * L.by[c] * 64 <= (__int128)0x7fffffffffffffffLL - end);
            end += (long)L.bx[c] * L.by[c] * 64;
            blocks += L.bx[c] * L.by[c];
        }
        LAYOUT_CHECK(L.plane_img == end && L.blocks_per_image == blocks && (size_t)blocks * 64 == L.coef_elems);
        LAYOUT_CHECK(b * (unsigned __int128)L.plane_img == (size_t)B * L.plane_img);     // B * plane_img does not wrap
        LAYOUT_CHECK(L.cw > 0 && L.ch > 0 && L.cw <= L.bx[0] * 8 && L.ch <= L.by[0] * 8);
        // scan sizes: the file's own where it has restart intervals, else made up from the file size
        const long n_int = plan ? (long)plan->int_off.size() - 1 : 1 + (long)(file_bytes % 7);
        std::vector<size_t> scans((size_t)B);
        for (int i = 0; i < B; ++i) scans[i] = plan ? plan->scan_bytes : (file_bytes + 13 * (size_t)i) % 100003;
        const frp::JpegDeviceStageLayout S = frp::jpeg_device_stage_layout(B, n_int, scans.data());
        LAYOUT_CHECK(S.soff.size() == (size_t)B + 1 && S.soff[0] == 0 && !S.too_large);
        for (int i = 0; i < B; ++i) LAYOUT_CHECK(S.soff[i] % 16 == 0 && S.soff[i + 1] >= S.soff[i] + scans[i]);
        LAYOUT_CHECK(S.o_int >= S.soff[B] && S.o_tab >= S.o_int + (size_t)B * (n_int + 1) * 4);
        LAYOUT_CHECK(S.o_q >= S.o_tab + (size_t)B * 6 * sizeof(frp::JpegHuffTableDev) && S.o_err >= S.o_q + (size_t)B * 384);
        LAYOUT_CHECK(S.o_int % 256 == 0 && S.o_tab % 256 == 0 && S.o_q % 256 == 0 && S.o_err % 256 == 0);
        LAYOUT_CHECK(S.stage_total == S.o_err + (size_t)B * 4);
    }
}

// The one answer of jpeg_device_stage_layout that no file of the corpus reaches: scans that end at or beyond 0xfffffff0 bytes do not
// fit the kernel's 32-bit offsets (pure arithmetic: nothing of that size is allocated).
static void check_too_large() {
    const char* path = "(made-up scan sizes)";
    const int B = 2;
    const size_t fits[B] = {0x7ffffff0u, 0x7fffffe1u}, over[B] = {0x7ffffff0u, 0x7ffffff1u};
    const frp::JpegDeviceStageLayout F = frp::jpeg_device_stage_layout(B, 1, fits), O = frp::jpeg_device_stage_layout(B, 1, over);
    LAYOUT_CHECK(F.soff[B] == 0xffffffe0u && !F.too_large && F.o_int == 0x100000000ull);
    LAYOUT_CHECK(O.soff[B] == 0xfffffff0u && O.too_large);
}

int main(int argc, char** argv) {
    int decoded = 0, refused = 0;
    check_too_large();
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) continue;
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        unsigned char* buf = (unsigned char*)malloc(n > 0 ? (size_t)n : 1);
        if (n > 0 && fread(buf, 1, (size_t)n, f) != (size_t)n) { fclose(f); free(buf); continue; }
        fclose(f);
        frp_jpeg_info info{};
        std::string err;
        int rc = frp::jpeg_info(buf, (size_t)n, &info, &err);
        if (rc == FRP_OK) {
            const size_t ce = frp::jpeg_coef_elems(info);
            if (ce > (size_t)64 << 20) { rc = FRP_ERR_INVALID; }          // (the pixel limit keeps real inputs far below this)
            else {
                int16_t* coef = (int16_t*)malloc(ce * 2 ? ce * 2 : 2);
                uint16_t q[192];
                rc = frp::jpeg_decode_coefficients(buf, (size_t)n, coef, ce, q, &info, &err);
                free(coef);
            }
        }
        {   // the plan of the device entropy decode (headers + the pass over the scan's 0xFF bytes) over the same bytes
            frp::JpegScanPlan plan;
            frp::JpegHuffTableDev tabs[6];
            std::string e2;
            const int rc2 = frp::jpeg_plan_scan(buf, (size_t)n, plan, tabs, &e2);
            if (rc2 == FRP_OK) {
                volatile unsigned sum = 0;
                for (size_t k = 0; k + 1 < plan.int_off.size(); ++k) sum += plan.scan[plan.int_off[k] < plan.scan_bytes ? plan.int_off[k] : 0];
                if (plan.scan_bytes) sum += plan.scan[plan.scan_bytes - 1];
            }
            if (rc == FRP_OK) check_layouts(argv[i], info, rc2 == FRP_OK && plan.info.restart_interval > 0 ? &plan : nullptr, (size_t)n);
        }
        if (rc == FRP_OK) ++decoded; else ++refused;
        free(buf);
    }
    printf("decoded %d refused %d\n", decoded, refused);
    return 0;
}
