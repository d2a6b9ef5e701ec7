// Prints the host-callable pieces of the conv kernels' frame (csrc/conv_common.h) for
// tests/test_conv_frame_host.py to hold against its own restatement:
//   walk G n_tiles b t0 t1 tstep           conv_tile_walk, every workgroup b of G
//   tap KS stride H W oy ox mask [mask_s1] conv_tap_mask (pad = KS / 2) and, for 3x3 stride 1, conv_tap_mask_s1
//   count n_dev N n                        conv_image_count
// No device is touched.
#include <climits>
#include <cstdio>

#include "conv_common.h"

int main() {
    static const int Gs[] = {8, 64, 256, 512, 1, 5, 9, 36, 250, 255};
    long lines = 0;
    for (int G : Gs) {
        const int ns[] = {0, 1, 7, 8, 9, G - 1, G, G + 1, 2 * G + 3, 8 * G, 100003};
        for (int n : ns)
            for (int b = 0; b < G; ++b) {
                const frp::TileWalk w = frp::conv_tile_walk(n, G, (unsigned)b);
                printf("walk %d %d %d %d %d %d\n", G, n, b, w.t0, w.t1, w.tstep);
                ++lines;
            }
    }
    static const int maps[][2] = {{1, 1}, {1, 5}, {2, 2}, {3, 7}, {8, 8}};
    static const int kinds[][2] = {{3, 1}, {3, 2}, {1, 1}, {1, 2}};   // (KS, stride)
    for (const auto& hw : maps)
        for (const auto& ks : kinds)
            for (int oy = 0; oy < hw[0]; ++oy)
                for (int ox = 0; ox < hw[1]; ++ox) {
                    const unsigned m = frp::conv_tap_mask(oy, ox, hw[0], hw[1], ks[1], ks[0] / 2, ks[0]);
                    if (ks[0] == 3 && ks[1] == 1)
                        printf("tap %d %d %d %d %d %d %u %u\n", ks[0], ks[1], hw[0], hw[1], oy, ox, m, frp::conv_tap_mask_s1(oy, ox, hw[0], hw[1]));
                    else
                        printf("tap %d %d %d %d %d %d %u\n", ks[0], ks[1], hw[0], hw[1], oy, ox, m);
                    ++lines;
                }
    static const int Ns[] = {1, 4, 32};
    for (int N : Ns) {
        const int vals[] = {-3, 0, 1, N, N + 1, INT_MAX};
        for (int v : vals) {
            printf("count %d %d %d\n", v, N, frp::conv_image_count(v, N));
            ++lines;
        }
    }
    printf("lines %ld\n", lines);
    return 0;
}
