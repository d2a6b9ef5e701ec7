// Prints conv_pick_ksplit (csrc/frp_internal.h) - the function the host, the conv kernel and the l2norm kernel all evaluate - over a grid
// of (M, Cout, Ktot, n_cu), one "M Cout Ktot n_cu flags has_res factor" line each, for tests/test_embed_tail_inputs.py to hold
// embed_tail_model.pick_ksplit against.  No device is touched.
#include <cstdio>

#include "frp_internal.h"

int main() {
    static const int Ms[] = {-1, 0, 1, 2, 3, 64, 255, 256, 257, 320, 511, 512, 513, 768, 769, 1024, 1025, 1280, 2048, 2049, 4096, 100000};
    static const int Couts[] = {8, 64, 96, 128, 136, 512, 1024};
    static const int Ktots[] = {64, 576, 4032, 4096, 4160, 6400, 8192, 25088, 25080, 32768};
    static const int ncus[] = {1, 8, 64, 104, 228, 256, 304};
    long lines = 0;
    for (int M : Ms)
        for (int Cout : Couts)
            for (int Ktot : Ktots)
                for (int ncu : ncus)
                    for (int variant = 0; variant < 3; ++variant) {
                        const int flags = variant == 1 ? 0 : FRP_FLAG_OUT_F32;
                        const bool has_res = variant == 2;
                        printf("%d %d %d %d %d %d %d\n", M, Cout, Ktot, ncu, flags, (int)has_res, frp::conv_pick_ksplit(M, Cout, Ktot, flags, has_res, ncu));
                        ++lines;
                    }
    printf("lines %ld\n", lines);
    return 0;
}
