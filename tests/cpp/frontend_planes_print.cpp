// tests/cpp/frontend_planes_print.cpp — host-only: the planes csrc/s3_format.h gives for a list of fp32 values (tests/test_frontend_planes_cpu.py holds the numpy
// restatement tests/frontend_planes.py against this output).  argv[1]: a text file of fp32 bit patterns in hex, one per line.  Per value one line:
//   value  split2h.A0 split2h.A1  join2h  split3.a split3.b split3.c  join_np(.., 3)        (all as hex bit patterns)
#include <cstdio>
#include <cstring>
#include "cuahn_vio_amd/csrc/s3_format.h"
using namespace hnet;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned u;
    while (fscanf(f, "%x", &u) == 1) {
        float v;
        const uint32_t uu = u;
        memcpy(&v, &uu, 4);
        uint16_t a0, a1, b0, b1, b2;
        split2h(v, a0, a1);
        split3(v, b0, b1, b2);
        printf("%08x %04x %04x %08x %04x %04x %04x %08x\n", uu, a0, a1, bits(join2h(a0, a1)), b0, b1, b2, bits(join_np(b0, b1, b2, 3)));
    }
    fclose(f);
    return 0;
}
