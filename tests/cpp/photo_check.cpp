// photo_check.cpp — the core of the photometric residual reference (tests/cpp/photo_ref.cpp) on fixed inputs, meant for AddressSanitizer + UBSan on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I <rocm>/include
//       -I cuahn_vio_amd/csrc tests/cpp/photo_check.cpp -o photo_check && ./photo_check
// Cases: identity, a shift that leaves the image, a perspective quadrilateral, a degenerate quadrilateral (det = 0) and NaN offsets; then the hostile pool of
// tests/photo_hostile.py (NaN, inf, 1e30 and 3e38 offsets, folded and collapsed quads, candidates on the inside bound): positions far outside every integer
// type reach floorf and the float-to-int conversions of the sampler, which is what UBSan is here for.  Exit status 0 = all hold.
#include "photo_ref.cpp"

#include <cstdlib>

namespace {
int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

// a fixed textured pair (an LCG; no library generator, so every platform sees the same bytes)
void make_pair(std::vector<uint8_t>& a, std::vector<uint8_t>& b) {
    a.resize(photo_ref::NPIX);
    b.resize(photo_ref::NPIX);
    uint32_t s = 12345u;
    for (int i = 0; i < photo_ref::NPIX; i++) {
        s = s * 1664525u + 1013904223u;
        a[i] = (uint8_t)(s >> 24);
        s = s * 1664525u + 1013904223u;
        b[i] = (uint8_t)(s >> 24);
    }
}
}  // namespace

int main() {
    using photo_ref::IMG_H;
    using photo_ref::IMG_W;
    using photo_ref::NPIX;
    std::vector<uint8_t> i1, i2;
    make_pair(i1, i2);
    std::vector<float> map(NPIX);
    int32_t edge = -1;

    // identity: every pixel inside, e = |img2 - img1| exactly (integers below 2^24 in a double)
    {
        const float off[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const photo_ref::Record r = photo_ref::record(i1.data(), i2.data(), off, &edge, map.data());
        double want = 0;
        for (int i = 0; i < NPIX; i++) want += std::abs((int)i2[i] - (int)i1[i]);
        CHECK(r.flags == 0 && r.n_inside == NPIX && edge == 0);
        CHECK(std::fabs(r.sum - want) <= 1e-4 * want && r.sum == r.sum_inside);
    }
    // +100.25 px in u: columns 0 .. 219 sample inside (ix <= 319.25), the others see zeros only
    {
        float off[8];
        for (int k = 0; k < 8; k++) off[k] = (k & 1) ? 0.0f : 100.25f;
        const photo_ref::Record r = photo_ref::record(i1.data(), i2.data(), off, &edge, map.data());
        double outside = 0;
        for (int v = 0; v < IMG_H; v++)
            for (int u = 220; u < IMG_W; u++) outside += i1[v * IMG_W + u];
        CHECK(r.flags == 0 && r.n_inside == IMG_H * 220);
        CHECK(std::fabs((r.sum - r.sum_inside) - outside) <= 1e-6 * outside);
    }
    // a perspective quadrilateral reaching outside on two sides
    {
        const float off[8] = {-14.5f, 9.25f, 6.0f, 21.75f, 30.5f, -12.0f, -8.25f, -17.5f};
        const photo_ref::Record r = photo_ref::record(i1.data(), i2.data(), off, &edge, map.data());
        CHECK(r.flags == 0 && r.n_inside > 0 && r.n_inside < NPIX && std::isfinite(r.sum) && r.sum_inside <= r.sum && edge >= 0);
        for (int i = 0; i < NPIX; i++) CHECK(map[i] >= 0.0f && map[i] <= 255.0f);
    }
    // degenerate: all four corners on one line (det = 0) -> flag, every sample 0, nothing inside
    {
        float off[8];
        for (int c = 0; c < 4; c++) {
            off[2 * c] = (float)(10.0 * c - hnet::p4(2 * c));
            off[2 * c + 1] = (float)(5.0 * c - hnet::p4(2 * c + 1));
        }
        const photo_ref::Record r = photo_ref::record(i1.data(), i2.data(), off, &edge, nullptr);
        double all = 0;
        for (int i = 0; i < NPIX; i++) all += i1[i];
        CHECK(r.flags == photo_ref::DEGENERATE && r.n_inside == 0 && r.sum_inside == 0.0 && std::isfinite(r.sum));
        CHECK(std::fabs(r.sum - all) <= 1e-6 * all);
    }
    // NaN offsets
    {
        float off[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        off[3] = NAN;
        const photo_ref::Record r = photo_ref::record(i1.data(), i2.data(), off, &edge, map.data());
        CHECK(r.flags == photo_ref::DEGENERATE && r.n_inside == 0 && std::isfinite(r.sum) && r.sum_inside == 0.0 && edge == 0);
    }
    // the batched entry point: the same records, in order
    {
        std::vector<uint8_t> a2(2 * (size_t)NPIX), b2(a2.size());
        memcpy(a2.data(), i1.data(), NPIX); memcpy(a2.data() + NPIX, i2.data(), NPIX);
        memcpy(b2.data(), i2.data(), NPIX); memcpy(b2.data() + NPIX, i1.data(), NPIX);
        std::vector<float> off(2 * 3 * 8, 0.0f);
        off[8] = -3.5f;
        off[16 + 24 + 1] = -2.0f;
        std::vector<photo_ref::Record> rec(6);
        std::vector<int32_t> edges(6);
        photo_ref_records(a2.data(), b2.data(), 2, off.data(), 3, rec.data(), edges.data(), nullptr);
        const photo_ref::Record one = photo_ref::record(i2.data(), i1.data(), off.data() + 40, nullptr, nullptr);
        CHECK(rec[5].sum == one.sum && rec[5].sum_inside == one.sum_inside && rec[5].n_inside == one.n_inside);
        CHECK(rec[0].n_inside == NPIX && rec[3].n_inside == NPIX && rec[1].n_inside < NPIX);
    }
    // the hostile pool (tests/photo_hostile.py pool(), the same order): flags, n_inside and n_edge depend on the offsets alone, so the table of
    // test_photo_hostile_cpu.py holds on this pair too; without a homography or a pixel inside every sample is 0 and the sum is that of img1
    {
        const float big = 1e30f, huge = 3e38f, inf = INFINITY;
        struct Cand { const char* name; float off[8]; int flags, n_inside, n_edge; };
        const Cand pool[] = {
            {"zero", {0, 0, 0, 0, 0, 0, 0, 0}, 0, 71680, 0},
            {"line", {0, 0, 10, 5 - 223, 20 - 319, 10 - 223, 30 - 319, 15}, 1, 0, 0},
            {"nan", {NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN}, 1, 0, 0},
            {"nan1", {0, 0, 0, NAN, 0, 0, 0, 0}, 1, 0, 0},
            {"inf", {0, 0, 0, inf, 0, 0, 0, 0}, 1, 0, 0},
            {"1e30all", {big, big, big, big, big, big, big, big}, 1, 0, 0},
            {"1e30one", {big, 0, 0, 0, 0, 0, 0, 0}, 0, 35896, 0},
            {"3e38", {huge, huge, 0, 0, 0, 0, 0, 0}, 0, 24146, 0},
            {"bowtie", {319, 0, 0, 0, 0, 0, -319, 0}, 0, 640, 0},
            {"concave", {0, 0, 0, 0, -250, -170, 0, 0}, 0, 41986, 1},
            {"far", {400, 0, 400, 0, 400, 0, 400, 0}, 0, 0, 0},
            {"farneg", {-5000, -5000, -5000, -5000, -5000, -5000, -5000, -5000}, 0, 0, 0},
            {"shift+1", {1, 0, 1, 0, 1, 0, 1, 0}, 0, 71456, 0},
            {"half-", {-0.5f, -0.5f, -0.5f, -0.5f, -0.5f, -0.5f, -0.5f, -0.5f}, 0, 71456, 543},
            {"half+", {0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f}, 0, 71137, 543},
            {"collapse", {100, 100, 100, 100 - 223, 100 - 319, 100 - 223, 100 - 319, 100}, 1, 0, 0},
            {"shrink", {100, 100, 100, 111.1494140625f - 223, 115.9501953125f - 319, 111.1494140625f - 223, 115.9501953125f - 319, 100}, 0, 71680, 0},
            {"zoom3", {-300, -300, -300, 369 - 223, 657 - 319, 369 - 223, 657 - 319, -300}, 0, 8025, 0},
            {"flip", {319, 223, 319, -223, -319, -223, -319, 223}, 0, 71680, 0},
        };
        constexpr int M = sizeof pool / sizeof pool[0];
        static_assert(M == 19, "the pool of tests/photo_hostile.py");
        double all = 0;
        for (int i = 0; i < NPIX; i++) all += i1[i];
        std::vector<float> offs(M * 8), hs(M * 9);
        std::vector<int32_t> oks(M);
        for (int c = 0; c < M; c++) memcpy(&offs[c * 8], pool[c].off, sizeof pool[c].off);
        photo_ref_homography(M, offs.data(), hs.data(), oks.data());
        for (int c = 0; c < M; c++) {
            const photo_ref::Record r = photo_ref::record(i1.data(), i2.data(), pool[c].off, &edge, map.data());
            if (!(r.flags == pool[c].flags && r.n_inside == pool[c].n_inside && edge == pool[c].n_edge))
                printf("%s: flags %d, n_inside %d, n_edge %d\n", pool[c].name, r.flags, r.n_inside, edge);
            CHECK(r.flags == pool[c].flags && r.n_inside == pool[c].n_inside && edge == pool[c].n_edge);
            CHECK(std::isfinite(r.sum) && std::isfinite(r.sum_inside) && r.sum_inside >= 0.0 && r.sum_inside <= r.sum);
            CHECK(oks[c] == (pool[c].flags == 0));
            for (int k = 0; k < 9; k++) CHECK(oks[c] ? std::isfinite(hs[c * 9 + k]) : std::isnan(hs[c * 9 + k]));
            if (r.flags || r.n_inside == 0) CHECK(r.sum == all && r.sum_inside == 0.0);
            for (int i = 0; i < NPIX; i += 97) CHECK(map[i] >= 0.0f && map[i] <= 255.0f);
        }
    }
    if (failures) { printf("photo_check: %d failure(s)\n", failures); return 1; }
    printf("photo_check: ok\n");
    return 0;
}
