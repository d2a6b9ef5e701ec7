// Host-side check of the fused block kernel's work decomposition (csrc/conv3x3_block64.hip): links the launcher source compiled host-only
// and walks conv3x3_block64_plan() + block64_item() - the functions the launcher and the kernel evaluate - over a list of maps:
//   every output pixel belongs to exactly one work item; every item's input rows and columns stay within the declared halo; the steps
//   of every item fit the plan's; the grid and the LDS bytes are in range; shapes beyond signed 32-bit byte offsets are refused.
// usage: block64_plan_harness <n_cu>      (prints one line per map, exits non-zero at the first violation)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "frp_internal.h"

using namespace frp;

static int fail(const char* what, int N, int H, int W) {
    printf("FAIL %s at N=%d H=%d W=%d\n", what, N, H, W);
    return 1;
}

static int check_map(int N, int H, int W, int ncu) {
    Block64Plan g;
    if (!conv3x3_block64_plan(N, H, W, ncu, &g)) return fail("plan refused", N, H, W);
    if (g.lds > 160 * 1024 || g.lds != BLOCK64_LDS_BYTES) return fail("LDS bytes", N, H, W);
    if (g.grid < 1 || g.grid > (ncu > 0 ? ncu : 256) || g.grid > g.items) return fail("grid", N, H, W);
    if (g.items != (long)N * g.strips * g.segs || (g.seg_rows & 3) || g.seg_rows < 4) return fail("items", N, H, W);
    if (!(g.fill > 0.0 && g.fill <= 1.0)) return fail("fill", N, H, W);
    std::vector<unsigned char> owner((size_t)N * H * W, 0);
    for (long item = 0; item < g.items; ++item) {
        const Block64Item it = block64_item((int)item, g.strips, g.segs, g.seg_rows, H);
        if (it.n < 0 || it.n >= N || it.ys < 0 || it.ys >= it.ye || it.ye > H || it.x0 < 0 || it.x0 >= W) return fail("item geometry", N, H, W);
        if (it.K + 1 > g.steps) return fail("steps", N, H, W);
        // conv2's last step reaches the segment's last row, conv1's the intermediate row below it
        if (it.ys - 6 + 4 * it.K + 3 < it.ye - 1 || it.ys - 1 + 4 * (it.K - 1) + 3 < it.ye) return fail("rows not reached", N, H, W);
        // input rows fetched: [first, last] within [ys - HALO_UP, ye - 1 + HALO_DOWN]; every row conv1 reads is fetched
        const int r0 = block64_first_in_row(it), r1 = block64_last_in_row(it);
        if (r0 < it.ys - BLOCK64_HALO_UP || r1 > it.ye - 1 + BLOCK64_HALO_DOWN) return fail("row halo", N, H, W);
        if (r0 > it.ys - 2 || r1 < it.ys - 1 + 4 * (it.K - 1) + 3 + 1) return fail("rows not fetched", N, H, W);
        // input columns x0 - 2 .. x0 + 31 cover the output columns' receptive field of two convs
        const int xe = it.x0 + BLOCK64_STRIP_W < W ? it.x0 + BLOCK64_STRIP_W : W;
        if (it.x0 - 2 + BLOCK64_IN_W - 1 < xe - 1 + 2) return fail("column halo", N, H, W);
        for (int y = it.ys; y < it.ye; ++y)
            for (int x = it.x0; x < xe; ++x) {
                unsigned char& o = owner[((size_t)it.n * H + y) * W + x];
                if (o) return fail("pixel owned twice", N, H, W);
                o = 1;
            }
    }
    for (unsigned char o : owner)
        if (!o) return fail("pixel without an owner", N, H, W);
    printf("ok N=%d H=%d W=%d strips=%d segs=%d seg_rows=%d steps=%d items=%ld grid=%d fill=%.3f pays=%d\n", N, H, W, g.strips, g.segs, g.seg_rows,
           g.steps, g.items, g.grid, g.fill, (int)conv3x3_block64_pays(g));
    return 0;
}

int main(int argc, char** argv) {
    const int ncu = argc > 1 ? atoi(argv[1]) : 256;
    static const int maps[][3] = {{1, 2, 2}, {2, 3, 29}, {1, 5, 30}, {1, 4, 31}, {3, 9, 61}, {2, 8, 60}, {1, 33, 90}, {5, 56, 56}, {1, 16, 480},
                                  {32, 272, 480}, {320, 56, 56}, {4, 272, 480}, {1, 1, 1}, {7, 13, 1}, {1, 1000, 31}, {37, 56, 56}, {2, 64, 96}};
    for (const auto& m : maps)
        if (check_map(m[0], m[1], m[2], ncu)) return 1;
    // out of signed 32-bit reach, and nonsense: refused
    Block64Plan g;
    static const int far[][3] = {{1024, 128, 128}, {64, 512, 512}, {0, 8, 8}, {1, 0, 8}, {1, 8, -1}, {130, 272, 480}};
    for (const auto& m : far)
        if (conv3x3_block64_plan(m[0], m[1], m[2], ncu, &g)) return fail("shape out of reach accepted", m[0], m[1], m[2]);
    if (!conv3x3_block64_plan(126, 272, 480, ncu, &g)) return fail("shape within reach refused", 126, 272, 480);
    // the launcher refuses them too, before anything is launched (no device is touched on this path)
    Block64Params p{};
    p.x = (const _Float16*)&g; p.w1 = p.w2 = (const _Float16*)&g; p.bias1 = p.bias2 = (const float*)&g; p.out = &p;
    p.N = 1024; p.H = 128; p.W = 128; p.act1 = p.act2 = FRP_ACT_RELU;
    if (launch_conv3x3_block64(p, nullptr) != hipErrorInvalidValue) return fail("launcher accepted a shape out of reach", p.N, p.H, p.W);
    p.N = 1; p.act2 = FRP_ACT_PRELU;
    if (launch_conv3x3_block64(p, nullptr) != hipErrorInvalidValue) return fail("launcher accepted an uncovered epilogue", p.N, p.H, p.W);
    printf("all ok\n");
    return 0;
}
