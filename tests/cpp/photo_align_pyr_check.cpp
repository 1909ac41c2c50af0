// photo_align_pyr_check.cpp — the core of the coarse-to-fine alignment reference (tests/cpp/photo_align_pyr_ref.cpp) and the shared level functions
// (include/hnet_photo_pyramid.h) on fixed inputs, meant for AddressSanitizer + UBSan on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I <rocm>/include
//       -I cuahn_vio_amd/csrc -I include tests/cpp/photo_align_pyr_check.cpp -o photo_align_pyr_check && ./photo_align_pyr_check [cases.bin]
// Without an argument: the pyramid of a fixed scene, of a 0 / 255 checker and of an all-255 frame (the rounding must not overflow a byte), a scene moved
// by (18, -10) pixels found from zero offsets with 4 levels (levels = 1 being the single-level reference byte for byte), and the hostile starts at 4 levels: a constant img2 (SINGULAR at every
// level, the offsets bit for bit), stripes, a start without a homography, one 400 px away, NaN (its payload comes back), inf, 1e30 and 3e38 offsets and
// the bowtie (the float-to-int conversions of far-out positions at every level are the point).
// With cases.bin = {int32 n, int32 levels, int32 max_iterations, float gate_px, img1 u8 [n][224][320], img2 u8 [n][224][320], truth f64 [n][8]} (the basin
// cases of tests/test_photo_align_pyr_cpu.py) it also aligns each pair from zero offsets and holds the end against the truth.
// Exit status 0 = all hold.
#include "photo_align_pyr_ref.cpp"

#include <cstdlib>

namespace {
int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

constexpr int CELL = 16, LW = 26, LH = 20, MARGIN = 40;      // lattice of 16-pixel cells covering 400 x 304

// a fixed smooth scene: bilinear interpolation of an LCG lattice (no library generator, so every platform sees the same bytes)
struct Scene {
    uint8_t lat[LH][LW];
    Scene() {
        uint32_t s = 2463534242u;
        for (int y = 0; y < LH; y++)
            for (int x = 0; x < LW; x++) {
                s = s * 1664525u + 1013904223u;
                lat[y][x] = (uint8_t)(s >> 24);
            }
    }
    uint8_t at(int x, int y) const {
        const int x0 = x / CELL, y0 = y / CELL, fx = x % CELL, fy = y % CELL;
        const int top = lat[y0][x0] * (CELL - fx) + lat[y0][x0 + 1] * fx, bot = lat[y0 + 1][x0] * (CELL - fx) + lat[y0 + 1][x0 + 1] * fx;
        return (uint8_t)((top * (CELL - fy) + bot * fy) / (CELL * CELL));
    }
};

void check_record(const hnet_align::Record& r, int K) {
    CHECK(r.accepted <= r.trials && r.trials <= K && std::isfinite(r.mse0) && std::isfinite(r.mse) && std::isfinite(r.lambda));
    for (int k = 0; k < 64; k++) CHECK(std::isfinite(r.info[k]));
    for (int k = 0; k < 8; k++) CHECK(std::isfinite(r.grad[k]));
}
}  // namespace

int main(int argc, char** argv) {
    using photo_ref::IMG_H;
    using photo_ref::IMG_W;
    using photo_ref::NPIX;
    namespace pa = hnet_align;
    namespace pr = photo_align_pyr_ref;
    const Scene scene;
    constexpr int DX = 18, DY = -10;
    std::vector<uint8_t> i1(NPIX), i2(NPIX), flat(NPIX, 93), white(NPIX, 255), checker(NPIX), stripes(NPIX);
    for (int v = 0; v < IMG_H; v++)
        for (int u = 0; u < IMG_W; u++) {
            i1[v * IMG_W + u] = scene.at(u + MARGIN, v + MARGIN);
            i2[v * IMG_W + u] = scene.at(u + MARGIN - DX, v + MARGIN - DY);      // img2(x + (DX, DY)) = img1(x)
            checker[v * IMG_W + u] = ((u + v) & 1) ? 255 : 0;
        }
    for (int v = 0; v < IMG_H; v++) memcpy(&stripes[v * IMG_W], &i2[100 * IMG_W], IMG_W);
    const float zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    // the pyramid: sizes, the cascade, and the rounding at the ends of the range
    {
        static_assert(pa::level_w(1) == 160 && pa::level_h(1) == 112 && pa::level_w(3) == 40 && pa::level_h(3) == 28 && pa::level_offset(3) == 22400, "level geometry");
        const pr::Pyramid pw(white.data()), pc(checker.data()), ps(i1.data());
        for (int k = 0; k < pa::PYR_BYTES; k++) CHECK(pw.store[k] == 255);
        for (int k = 0; k < pa::PYR_BYTES; k++) CHECK(pc.store[k] == 128);                  // (0 + 255 + 255 + 0 + 2) >> 2, then 128 all the way up
        CHECK(ps.lv[1][0] == (uint8_t)((i1[0] + i1[1] + i1[IMG_W] + i1[IMG_W + 1] + 2) >> 2));
        const uint8_t* l1 = ps.lv[1];
        CHECK(ps.lv[2][81] == (uint8_t)((l1[2 * 160 + 2] + l1[2 * 160 + 3] + l1[3 * 160 + 2] + l1[3 * 160 + 3] + 2) >> 2));
        std::vector<uint8_t> packed(2 * pa::PYR_BYTES);
        photo_align_pyr_ref_pyramid(i1.data(), 1, packed.data());
        CHECK(memcmp(packed.data(), ps.store, pa::PYR_BYTES) == 0);
        CHECK(pa::level_centre(0, 7) == 7.0f && pa::level_centre(1, 7) == 14.5f && pa::level_centre(3, 39) == 315.5f);
        CHECK(pa::level_min_valid(20000, 3) == 312 && pa::level_min_valid(20000, 0) == 20000);
    }
    // the moved scene from zero offsets: four levels end on (DX, DY) at every corner (the scene is smooth: what one level cannot reach is the business of cases.bin)
    {
        pa::Opts o;
        pa::default_opts(o);
        o.max_iterations = 8;
        pa::Record recs[pa::MAX_LEVELS], single;
        pr::align(i1.data(), i2.data(), zero, o, 4, recs);
        double worst = 0.0;
        for (int k = 0; k < 8; k++) worst = std::fmax(worst, std::fabs((double)recs[0].offsets_px[k] - (k % 2 ? DY : DX)));
        for (int L = 3; L >= 0; L--)
            printf("moved scene, level %d: flags %d, trials %d, accepted %d, n_valid %d -> %d, mse %.3f -> %.3f\n", L, recs[L].flags, recs[L].trials, recs[L].accepted,
                   recs[L].n_valid0, recs[L].n_valid, recs[L].mse0, recs[L].mse);
        printf("moved scene: worst corner error %.4f px\n", worst);
        CHECK(worst < 0.1);
        for (int L = 0; L < 4; L++) {
            check_record(recs[L], 8);
            CHECK(!(recs[L].flags & (pa::SINGULAR | pa::DEGENERATE | pa::FEW_PIXELS)) && recs[L].mse <= recs[L].mse0);
            CHECK(recs[L].n_valid0 <= (pa::level_w(L) - 1) * (pa::level_h(L) - 1));
        }
        // levels = 1 is the single-level reference, byte for byte
        pa::Record one[1];
        o.max_iterations = 32;
        memset(&single, 0, sizeof single);
        memset(one, 0, sizeof one);
        photo_align_ref::align(i1.data(), i2.data(), zero, o, single);
        pr::align(i1.data(), i2.data(), zero, o, 1, one);
        CHECK(memcmp(&single, one, sizeof single) == 0);
        double off1 = 0.0;
        for (int k = 0; k < 8; k++) off1 = std::fmax(off1, std::fabs((double)single.offsets_px[k] - (k % 2 ? DY : DX)));
        printf("moved scene, one level, 32 trials: worst corner error %.4f px\n", off1);
    }
    // hostile starts at four levels, min_valid = 0 and the default
    {
        const float big = 1e30f, huge = 3e38f, inf = INFINITY;
        float line[8] = {0, 0, 10, 5, 20, 10, 30, 15}, far[8], nanp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 8; k++) { line[k] -= (float)hnet::p4(k); far[k] = k % 2 ? 0.0f : 400.0f; }
        const uint32_t payload = 0x7FC12345u;
        memcpy(&nanp[3], &payload, 4);
        struct Start { const char* name; const uint8_t* img2; float x[8]; int flags; };      // flags -1: not pinned
        Start starts[] = {
            {"constant", flat.data(), {0.5f, -0.25f, 1.0f, 0.0f, -1.5f, 0.75f, 0.0f, 2.0f}, pa::SINGULAR},
            {"stripes", stripes.data(), {0, 0, 0, 0, 0, 0, 0, 0}, pa::SINGULAR},
            {"line", i2.data(), {0}, pa::DEGENERATE},
            {"far", i2.data(), {0}, pa::FEW_PIXELS},
            {"nan", i2.data(), {0}, pa::DEGENERATE},
            {"inf", i2.data(), {0, 0, 0, inf, 0, 0, 0, 0}, pa::DEGENERATE},
            {"1e30all", i2.data(), {big, big, big, big, big, big, big, big}, pa::DEGENERATE},
            {"1e30one", i2.data(), {big, 0, 0, 0, 0, 0, 0, 0}, pa::FEW_PIXELS},
            {"3e38", i2.data(), {huge, huge, 0, 0, 0, 0, 0, 0}, -1},
            {"bowtie", i2.data(), {319, 0, 0, 0, 0, 0, -319, 0}, -1},
            {"shift(318,0)", i2.data(), {318, 0, 318, 0, 318, 0, 318, 0}, -1},
        };
        memcpy(starts[2].x, line, 32);
        memcpy(starts[3].x, far, 32);
        memcpy(starts[4].x, nanp, 32);
        for (int mv = 0; mv <= 20000; mv += 20000)
            for (const Start& st : starts) {
                pa::Opts o;
                pa::default_opts(o);
                o.max_iterations = 8;
                o.min_valid = mv;
                pa::Record recs[pa::MAX_LEVELS];
                pr::align(i1.data(), st.img2, st.x, o, 4, recs);
                for (int L = 0; L < 4; L++) {
                    if (!std::isnan(st.x[3])) check_record(recs[L], 8);
                    if (st.flags >= 0) {
                        if (recs[L].flags != st.flags) printf("%s min_valid %d level %d: flags %d, n_valid0 %d\n", st.name, mv, L, recs[L].flags, recs[L].n_valid0);
                        CHECK(recs[L].flags == st.flags && recs[L].trials == 0);
                        CHECK(memcmp(recs[L].offsets_px, st.x, 32) == 0);
                        if (st.flags & (pa::DEGENERATE | pa::FEW_PIXELS)) {
                            CHECK(recs[L].n_valid0 == 0 && recs[L].mse0 == 0.0);
                            for (int k = 0; k < 64; k++) CHECK(recs[L].info[k] == 0.0);
                        }
                    }
                }
                if (st.img2 == flat.data())
                    for (int L = 0; L < 4; L++)
                        for (int k = 0; k < 64; k++) CHECK(recs[L].info[k] == 0.0);
            }
    }
    // the basin cases of the python test, when it passed them
    if (argc == 2) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        int32_t hdr[3];
        float gate;
        if (fread(hdr, sizeof hdr, 1, f) != 1 || fread(&gate, 4, 1, f) != 1 || hdr[0] < 1 || hdr[0] > 64 || hdr[1] < 1 || hdr[1] > pa::MAX_LEVELS || hdr[2] < 0 ||
            hdr[2] > pa::MAX_ITERATIONS) {
            fprintf(stderr, "bad header\n");
            fclose(f);
            return 2;
        }
        const int n = hdr[0];
        std::vector<uint8_t> a((size_t)n * NPIX), b(a.size());
        std::vector<double> truth((size_t)n * 8);
        const bool ok = fread(a.data(), 1, a.size(), f) == a.size() && fread(b.data(), 1, b.size(), f) == b.size() &&
                        fread(truth.data(), 8, truth.size(), f) == truth.size();
        fclose(f);
        if (!ok) { fprintf(stderr, "short input\n"); return 2; }
        pa::Opts o;
        pa::default_opts(o);
        o.max_iterations = hdr[2];
        std::vector<pa::Record> out((size_t)n), lv((size_t)n * hdr[1]);
        std::vector<float> x0((size_t)n * 8, 0.0f);
        photo_align_pyr_ref_run(a.data(), b.data(), n, x0.data(), &o, hdr[1], out.data(), lv.data());
        for (int i = 0; i < n; i++) {
            double worst = 0.0;
            for (int k = 0; k < 8; k++) worst = std::fmax(worst, std::fabs((double)out[i].offsets_px[k] - truth[i * 8 + k]));
            printf("basin case %d: %.4f px from the truth (gate %.3f)\n", i, worst, gate);
            CHECK(worst < gate);
            CHECK(memcmp(&out[i], &lv[(size_t)i * hdr[1]], sizeof(pa::Record)) == 0);
            for (int L = 0; L < hdr[1]; L++) check_record(lv[(size_t)i * hdr[1] + L], hdr[2]);
        }
    }
    if (failures) { printf("photo_align_pyr_check: %d FAILED\n", failures); return 1; }
    printf("photo_align_pyr_check: ok\n");
    return 0;
}
