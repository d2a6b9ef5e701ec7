// Runs the host side of the detection tail's box arithmetic (csrc/box_nms.h: box_area1, box_iou1) for
// tests/test_box_nms_host.py to hold against tracks.iou:
//   stdin   one box pair per line, eight fp32 bit patterns in hex: ax1 ay1 ax2 ay2 bx1 by1 bx2 by2
//   stdout  per pair the bit patterns of box_area1(a), box_area1(b) and box_iou1(a, b), then "lines N"
// Bit patterns, so that a NaN or an infinity travels unchanged.  No device is touched.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "box_nms.h"

static float as_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t as_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

int main() {
    long lines = 0;
    uint32_t u[8];
    while (scanf("%x %x %x %x %x %x %x %x", &u[0], &u[1], &u[2], &u[3], &u[4], &u[5], &u[6], &u[7]) == 8) {
        float v[8];
        for (int i = 0; i < 8; ++i) v[i] = as_float(u[i]);
        const float aa = frp::box_area1(v[0], v[1], v[2], v[3]), ba = frp::box_area1(v[4], v[5], v[6], v[7]);
        const float iou = frp::box_iou1(v[0], v[1], v[2], v[3], aa, v[4], v[5], v[6], v[7], ba);
        printf("%08x %08x %08x\n", as_bits(aa), as_bits(ba), as_bits(iou));
        ++lines;
    }
    printf("lines %ld\n", lines);
    return 0;
}
