// hnet::split2h (csrc/s3_format.h, host side) over a file of fp32 values: argv[1] = n float32 in, argv[2] = n pairs (A0, A1) of uint16 out.
// tests/test_f16x2_range_cases_cpu.py compares the pairs with the numpy restatement the range cases are built with (tests/f16x2_range_cases.py).
#include "cuahn_vio_amd/csrc/s3_format.h"
#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const size_t n = (size_t)ftell(f) / sizeof(float);
    fseek(f, 0, SEEK_SET);
    std::vector<float> v(n);
    if (fread(v.data(), sizeof(float), n, f) != n) return 2;
    fclose(f);
    std::vector<uint16_t> out(2 * n);
    for (size_t i = 0; i < n; i++) hnet::split2h(v[i], out[2 * i], out[2 * i + 1]);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), sizeof(uint16_t), 2 * n, f) != 2 * n) return 2;
    fclose(f);
    return 0;
}
