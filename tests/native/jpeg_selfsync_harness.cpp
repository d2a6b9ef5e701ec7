// CPU harness of the self-synchronising JPEG entropy decoder (csrc/jpeg_selfsync.h over csrc/jpeg_entropy.h: the per-thread routines the kernels of
// csrc/jpeg_selfsync.hip run), built by tests/test_jpeg_selfsync_host.py with g++ -fsanitize=address,undefined.  The grid is emulated
// serially, launch by launch and workgroup by workgroup as the kernels run it: speculate, rounds to the fix-point (inside a workgroup, then
// across workgroups with the boundary states double-buffered between launches), count, write, DC sums.  Every input is copied into a heap
// block of exactly its size, its scan into one of exactly the scan's size rounded up to the staging layout's 16 bytes, and the coefficients
// go to an exactly sized buffer: a read or write outside is a sanitizer report.
//
// For every file and S in {16, 32, 128, 1024}: the verdict (accepted / refused) equals jpeg_decode_coefficients', the coefficients are
// equal where both accept, synchronisation rounds <= subsequences, launches <= workgroups.  One line per file on stdout:
//   <path> host=<0|1> [S=<S>:<subsequences>:<rounds>:<launches>:<blocks>]...        (host=1: accepted; files with restart intervals: "skipped")
// Exit code 3 with a message on stderr when one of these does not hold.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "frp.h"
#include "jpeg_host.h"
#include "jpeg_selfsync.h"

using namespace frp;

#define REQUIRE(cond, ...)                                                     \
    do {                                                                       \
        if (!(cond)) { fprintf(stderr, "%s: ", path); fprintf(stderr, __VA_ARGS__); fprintf(stderr, " [%s]\n", #cond); exit(3); } \
    } while (0)

struct Emu {
    const char* path;
    const uint8_t* scan;
    uint32_t n_bytes, S, n_sub, n_wg;
    const JpegHuffTableDev* tab;
    JssGeom g;
    std::vector<JssState> entry, exit_, wgx[2];
    std::vector<uint32_t> cnt, base;
    int launches = 0;
    uint32_t rounds = 0;                  // over the launches: the most rounds a workgroup of that launch ran with a change

    uint32_t start_bit(uint32_t i) const { return jss_start(scan, n_bytes, i, n_sub, S) * 8u; }
    void decode(uint32_t i) { jss_decode<false>(scan, n_bytes, tab, kJpegZigZag, g, entry[i], start_bit(i + 1), nullptr, 0, &exit_[i], &cnt[i]); }

    // one launch of the synchronisation kernel; -> the rounds of the launch (0: nothing changed)
    uint32_t launch(int k) {
        uint32_t lr = 0;
        for (uint32_t w = 0; w < n_wg; ++w) {
            const uint32_t first = w * JSS_WG, m = (n_sub - first < JSS_WG) ? n_sub - first : JSS_WG;
            if (k > 0 && w == 0) { wgx[(k & 1) ^ 1][0] = exit_[m - 1]; continue; }
            JssState ex[JSS_WG + 1];
            if (k == 0) {
                for (uint32_t t = 0; t < m; ++t) { entry[first + t] = jss_pack(start_bit(first + t), 0, 0); decode(first + t); }
                ex[0] = entry[first];
            } else {
                ex[0] = wgx[k & 1][w - 1];
            }
            for (uint32_t t = 0; t < m; ++t) ex[t + 1] = exit_[first + t];
            uint32_t with_change = 0;
            for (int r = 0; r < JSS_WG; ++r) {
                JssState ne[JSS_WG];
                for (uint32_t t = 0; t < m; ++t) ne[t] = ex[t];                   // (barrier: every thread has read its predecessor's exit)
                bool any = false;
                for (uint32_t t = 0; t < m; ++t)
                    if (ne[t] != entry[first + t]) {
                        entry[first + t] = ne[t];
                        decode(first + t);
                        ex[t + 1] = exit_[first + t];
                        any = true;
                    }
                if (!any) break;
                ++with_change;
            }
            wgx[(k & 1) ^ 1][w] = exit_[first + m - 1];
            lr = with_change > lr ? with_change : lr;
        }
        return lr;
    }

    // -> error flag; stats = subsequences, rounds, blocks, flag
    int run(int16_t* coef, int32_t* stats) {
        n_sub = jss_subsequences(n_bytes, S);
        n_wg = (n_sub + JSS_WG - 1) / JSS_WG;
        entry.assign(n_sub, 0); exit_.assign(n_sub, 0); cnt.assign(n_sub, 0); base.assign(n_sub, 0);
        wgx[0].assign(n_wg, 0); wgx[1].assign(n_wg, 0);
        rounds = 0;
        for (launches = 0;;) {                                                    // the host's relaunch loop: launch k leaves workgroups 0 .. k final
            REQUIRE((uint32_t)launches <= n_wg, "S %u: no fix-point after %d launches", S, launches);
            const uint32_t lr = launch(launches);
            rounds += lr;
            ++launches;
            if (launches == 1 ? n_wg == 1 : lr == 0) break;                       // (one workgroup: launch 0 ran to its fix-point)
        }
        for (uint32_t i = 0; i + 1 < n_sub; ++i) REQUIRE(entry[i + 1] == exit_[i], "S %u: not a fix-point at subsequence %u", S, i);
        // count
        uint32_t running = 0;
        for (uint32_t i = 0; i < n_sub; ++i) { base[i] = running; running += cnt[i]; }
        int err = running < g.total;
        // write
        for (uint32_t i = 0; i < n_sub; ++i)
            err |= jss_decode<true>(scan, n_bytes, tab, kJpegZigZag, g, entry[i], start_bit(i + 1), coef, base[i], nullptr, nullptr);
        // DC: running sums per component in scan order
        for (int c = 0; c < g.components; ++c) {
            const uint32_t nb = g.total / (uint32_t)g.bpm * (uint32_t)(g.hs[c] * g.vs[c]);
            uint32_t pred = 0;
            for (uint32_t k = 0; k < nb; ++k) {
                int16_t* d = coef + jss_dc_addr(g, c, k);
                pred += (uint32_t)(int32_t)*d;
                *d = (int16_t)(int32_t)pred;
            }
        }
        stats[0] = (int32_t)n_sub; stats[1] = (int32_t)rounds; stats[2] = (int32_t)(running < g.total ? running : g.total); stats[3] = err;
        REQUIRE(rounds <= n_sub, "S %u: %u rounds for %u subsequences", S, rounds, n_sub);
        return err;
    }
};

int main(int argc, char** argv) {
    int accepted = 0, refused = 0, skipped = 0;
    for (int a = 1; a < argc; ++a) {
        const char* path = argv[a];
        FILE* f = fopen(path, "rb");
        if (!f) continue;
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        unsigned char* buf = (unsigned char*)malloc(n > 0 ? (size_t)n : 1);
        if (n > 0 && fread(buf, 1, (size_t)n, f) != (size_t)n) { fclose(f); free(buf); continue; }
        fclose(f);
        frp_jpeg_info info{};
        std::string err;
        int rc = jpeg_info(buf, (size_t)n, &info, &err);
        std::vector<int16_t> ref;
        uint16_t q[192];
        if (rc == FRP_OK) {
            const size_t ce = jpeg_coef_elems(info);
            if (ce > (size_t)64 << 20) { free(buf); ++skipped; printf("%s skipped\n", path); continue; }      // (a damaged header claiming a huge image)
            ref.assign(ce, 0);
            rc = jpeg_decode_coefficients(buf, (size_t)n, ref.data(), ce, q, &info, &err);
        }
        JpegScanPlan plan;
        JpegHuffTableDev tabs[6];
        std::string e2;
        const int rc2 = jpeg_plan_scan(buf, (size_t)n, plan, tabs, &e2);
        if (plan.info.restart_interval != 0 && plan.info.width > 0) { ++skipped; printf("%s skipped\n", path); free(buf); continue; }
        if (rc2 != FRP_OK) {
            REQUIRE(rc != FRP_OK, "the plan refuses (%s) what the host decoder accepts", e2.c_str());
            ++refused;
            printf("%s host=0\n", path);
            free(buf);
            continue;
        }
        REQUIRE(memcmp(plan.qtab, q, sizeof(q)) == 0 || rc != FRP_OK, "quantisation tables differ");
        // the scan as it is staged: its bytes, then zeros up to the next multiple of 16 (jpeg_device_stage_layout: 16-byte slots)
        const size_t one[1] = {plan.scan_bytes};
        const JpegDeviceStageLayout SL = jpeg_device_stage_layout(1, 3, one);
        REQUIRE(!SL.too_large && SL.soff[0] == 0 && SL.soff[1] >= plan.scan_bytes && SL.soff[1] % 16 == 0, "stage layout");
        const size_t slot = SL.soff[1] ? SL.soff[1] : 16;
        uint8_t* scan = (uint8_t*)aligned_alloc(16, slot);
        memset(scan, 0, slot);
        memcpy(scan, plan.scan, plan.scan_bytes);
        const JpegBatchLayout L = jpeg_batch_layout(plan.info, 1);
        Emu E;
        E.path = path;
        E.scan = scan;
        E.n_bytes = (uint32_t)plan.scan_bytes;
        E.tab = tabs;
        E.g = jss_geom(plan.info, L);
        const JssGeom& g = E.g;
        REQUIRE(g.bpm >= 1 && g.bpm <= 6 && (size_t)g.total * 64 == L.coef_elems && (uint32_t)(plan.info.mcus_x * plan.info.mcus_y * g.bpm) == g.total, "geometry");
        printf("%s host=%d", path, rc == FRP_OK ? 1 : 0);
        for (uint32_t S : {16u, 32u, 128u, 1024u}) {
            int16_t* coef = (int16_t*)calloc(L.coef_elems ? L.coef_elems : 1, 2);
            int32_t stats[4];
            E.S = S;
            const int bad = E.run(coef, stats);
            REQUIRE((bad == 0) == (rc == FRP_OK), "S %u: verdict %d, the host decoder's %d (%s)", S, bad, rc, err.c_str());
            if (!bad) {
                REQUIRE(memcmp(coef, ref.data(), L.coef_elems * 2) == 0, "S %u: coefficients differ", S);
                REQUIRE((uint32_t)stats[2] == g.total, "S %u: %d blocks counted of %u", S, stats[2], g.total);
            }
            printf(" S=%u:%d:%d:%d:%d", S, stats[0], stats[1], E.launches, stats[2]);
            free(coef);
        }
        printf("\n");
        if (rc == FRP_OK) ++accepted; else ++refused;
        free(scan);
        free(buf);
    }
    printf("accepted %d refused %d skipped %d\n", accepted, refused, skipped);
    return 0;
}
