// photo_robust_check.cpp — the core of the gain / bias + Huber alignment reference (tests/cpp/photo_robust_ref.cpp) and the shared functions of
// include/hnet_photo_robust.h on fixed inputs, meant for AddressSanitizer + UBSan on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I <rocm>/include
//       -I cuahn_vio_amd/csrc -I include tests/cpp/photo_robust_check.cpp -o photo_robust_check && ./photo_robust_check
// A fixed scene moved by (6, -4) pixels whose second frame is 0.7 x + 25: four levels with the model find the move, the gain and the bias; with a
// 40 x 60 block of noise besides, k = 10 ends closer to the move than the quadratic loss; with the model off and k = 0 every level's common part is the coarse-to-fine reference byte for byte; the residual and the
// weights at the edges of their ranges; and the hostile starts at four levels with the model on, gain0 = 1e-30 and 1e30 and k = 1e-6 among them (the
// float-to-int conversions of far-out positions and the ten-parameter step on degenerate matrices are the point).
// Exit status 0 = all hold.
#include "photo_robust_ref.cpp"

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

void check_record(const hnet_robust::Record& r, int K) {
    const hnet_align::Record& x = r.px;
    CHECK(x.accepted <= x.trials && x.trials <= K && std::isfinite(x.mse0) && std::isfinite(x.mse) && std::isfinite(x.lambda));
    CHECK(std::isfinite(r.gain) && r.gain > 0.0 && std::isfinite(r.bias) && r.n_outliers >= 0 && r.n_outliers <= x.n_valid && r.n_outliers0 <= x.n_valid0);
    for (int k = 0; k < 64; k++) CHECK(std::isfinite(x.info[k]));
    for (int k = 0; k < 100; k++) CHECK(std::isfinite(r.info10[k]));
    for (int k = 0; k < 10; k++) CHECK(std::isfinite(r.grad10[k]));
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) CHECK(r.info10[i * 10 + j] == x.info[i * 8 + j]);
}
}  // namespace

int main() {
    using photo_ref::IMG_H;
    using photo_ref::IMG_W;
    using photo_ref::NPIX;
    namespace pa = hnet_align;
    namespace pr = hnet_robust;
    namespace rr = photo_robust_ref;
    const Scene scene;
    constexpr int DX = 6, DY = -4;
    std::vector<uint8_t> i1(NPIX), i2(NPIX), ex(NPIX), sp(NPIX), flat(NPIX, 93), stripes(NPIX);
    uint32_t s = 88172645u;
    for (int v = 0; v < IMG_H; v++)
        for (int u = 0; u < IMG_W; u++) {
            i1[v * IMG_W + u] = scene.at(u + MARGIN, v + MARGIN);
            i2[v * IMG_W + u] = scene.at(u + MARGIN - DX, v + MARGIN - DY);      // img2(x + (DX, DY)) = img1(x)
            int g = (int)floor(0.7 * i2[v * IMG_W + u] + 25.0 + 0.5);
            ex[v * IMG_W + u] = (uint8_t)g;
            if (v >= 60 && v < 100 && u >= 100 && u < 160) {
                s = s * 1664525u + 1013904223u;
                g = (int)(s >> 24);
            }
            sp[v * IMG_W + u] = (uint8_t)(g < 0 ? 0 : (g > 255 ? 255 : g));
        }
    for (int v = 0; v < IMG_H; v++) memcpy(&stripes[v * IMG_W], &i2[100 * IMG_W], IMG_W);
    const float zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    // the residual and the weights
    {
        float r, omega;
        double rho;
        CHECK(!pr::residual(1.0f, 0.0f, 0.0f, 0.5f, 0.25f, r, omega, rho) && r == 63.75f && omega == 1.0f && rho == 63.75 * 63.75);
        CHECK(pr::residual(1.0f, 0.0f, 10.0f, 0.5f, 0.25f, r, omega, rho) && r == 63.75f && omega == 10.0f / 63.75f && rho == 10.0 * (2.0 * 63.75 - 10.0));
        CHECK(!pr::residual(1.0f, 0.0f, 63.75f, 0.5f, 0.25f, r, omega, rho) && omega == 1.0f);          // |r| == k is an inlier
        CHECK(pr::residual(2.0f, pr::bias_f(-25.5), 10.0f, 0.25f, 0.75f, r, omega, rho) && r < 0.0f && omega > 0.0f && omega < 1.0f);
        CHECK(pr::sym_index(0, 0) == 0 && pr::sym_index(10, 10) == 65 && pr::sym_index(9, 10) == 64 && pr::sym_index(1, 1) == 11);
        double tt[66];
        for (int k = 0; k < 66; k++) tt[k] = k;
        CHECK(pr::ss_entry(tt, 0) == 0 && pr::ss_entry(tt, 8) == 8 && pr::ss_entry(tt, 9) == 11 && pr::ss_entry(tt, 44) == pr::sym_index(8, 8));
        pr::Opts o;
        pr::default_opts(o);
        CHECK(pr::opts_valid(o) && o.brightness == 1 && o.huber_k == 10.0 && o.gain0 == 1.0 && o.bias0 == 0.0);
        o.gain0 = 0.0;
        CHECK(!pr::opts_valid(o));
    }
    // the scene with the exposure step, then with the block too, from zero offsets: four levels, the model, k = 10 and k = 0
    {
        pr::Opts o;
        pr::default_opts(o);
        o.base.max_iterations = 24;
        pr::Record recs[pa::MAX_LEVELS];
        double worst[3] = {0.0, 0.0, 0.0};
        for (int c = 0; c < 3; c++) {               // 0: exposure step only; 1: with the block; 2: with the block and quadratic
            o.huber_k = c < 2 ? 10.0 : 0.0;
            rr::align(i1.data(), c == 0 ? ex.data() : sp.data(), zero, o, 4, recs);
            for (int k = 0; k < 8; k++) worst[c] = std::fmax(worst[c], std::fabs((double)recs[0].px.offsets_px[k] - (k % 2 ? DY : DX)));
            for (int L = 3; L >= 0; L--)
                printf("scene %d, level %d: flags %d, trials %d, accepted %d, n_valid %d -> %d, outliers %d -> %d, cost %.3f -> %.3f, gain %.4f, bias %.3f\n", c, L,
                       recs[L].px.flags, recs[L].px.trials, recs[L].px.accepted, recs[L].px.n_valid0, recs[L].px.n_valid, recs[L].n_outliers0, recs[L].n_outliers,
                       recs[L].px.mse0, recs[L].px.mse, recs[L].gain, recs[L].bias);
            printf("scene %d: worst corner error %.4f px\n", c, worst[c]);
            CHECK(std::fabs(recs[0].gain - 1.0 / 0.7) < 0.1 && std::fabs(recs[0].bias + 25.0 / 0.7) < 8.0);
            for (int L = 0; L < 4; L++) {
                check_record(recs[L], 24);
                CHECK(!(recs[L].px.flags & (pa::SINGULAR | pa::DEGENERATE | pa::FEW_PIXELS)) && recs[L].px.mse <= recs[L].px.mse0);
            }
        }
        // the exposure step alone is found to the rounding of the frame (measured 0.015 px).  This scene's gradients are weak (16-pixel bilinear cells), so
        // 2400 pixels of noise pull hard: 0.92 px off with the quadratic loss, 0.49 px with k = 10 (measured); the Huber weights must be the closer
        CHECK(worst[0] < 0.1);
        CHECK(worst[1] < worst[2]);
        // the model off and k = 0: the coarse-to-fine reference byte for byte, on the clean and on the spoiled pair
        for (const uint8_t* b : {i2.data(), sp.data()}) {
            o.brightness = 0;
            o.huber_k = 0.0;
            pa::Record want[pa::MAX_LEVELS];
            memset(want, 0, sizeof want);
            memset(recs, 0, sizeof recs);
            photo_align_pyr_ref::align(i1.data(), b, zero, o.base, 4, want);
            rr::align(i1.data(), b, zero, o, 4, recs);
            for (int L = 0; L < 4; L++) {
                CHECK(memcmp(&recs[L].px, &want[L], sizeof(pa::Record)) == 0);
                CHECK(recs[L].gain == 1.0 && recs[L].bias == 0.0 && recs[L].n_outliers == 0);
                for (int k = 80; k < 100; k++) CHECK(recs[L].info10[k] == 0.0);
            }
        }
    }
    // hostile starts at four levels with the model on, min_valid = 0 and the default
    {
        const float big = 1e30f, huge = 3e38f, inf = INFINITY;
        float line[8] = {0, 0, 10, 5, 20, 10, 30, 15}, far[8], nanp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 8; k++) { line[k] -= (float)hnet::p4(k); far[k] = k % 2 ? 0.0f : 400.0f; }
        const uint32_t payload = 0x7FC12345u;
        memcpy(&nanp[3], &payload, 4);
        struct Start { const char* name; const uint8_t* img2; float x[8]; int flags; double gain0, k; };      // flags -1: not pinned
        Start starts[] = {
            {"constant", flat.data(), {0.5f, -0.25f, 1.0f, 0.0f, -1.5f, 0.75f, 0.0f, 2.0f}, pa::SINGULAR, 1.0, 10.0},
            {"stripes", stripes.data(), {0, 0, 0, 0, 0, 0, 0, 0}, pa::SINGULAR, 1.0, 10.0},
            {"line", i2.data(), {0}, pa::DEGENERATE, 1.0, 10.0},
            {"far", i2.data(), {0}, pa::FEW_PIXELS, 1.0, 10.0},
            {"nan", i2.data(), {0}, pa::DEGENERATE, 1.0, 10.0},
            {"inf", i2.data(), {0, 0, 0, inf, 0, 0, 0, 0}, pa::DEGENERATE, 1.0, 10.0},
            {"1e30all", i2.data(), {big, big, big, big, big, big, big, big}, pa::DEGENERATE, 1.0, 10.0},
            {"1e30one", i2.data(), {big, 0, 0, 0, 0, 0, 0, 0}, pa::FEW_PIXELS, 1.0, 10.0},
            {"3e38", i2.data(), {huge, huge, 0, 0, 0, 0, 0, 0}, -1, 1.0, 10.0},
            {"bowtie", i2.data(), {319, 0, 0, 0, 0, 0, -319, 0}, -1, 1.0, 10.0},
            {"gain0 1e-30", sp.data(), {0}, -1, 1e-30, 10.0},
            {"gain0 1e30", sp.data(), {0}, -1, 1e30, 10.0},
            {"gain0 1e30, quadratic", sp.data(), {0}, -1, 1e30, 0.0},
            {"all outliers", sp.data(), {0}, -1, 1.0, 1e-6},
        };
        memcpy(starts[2].x, line, 32);
        memcpy(starts[3].x, far, 32);
        memcpy(starts[4].x, nanp, 32);
        for (int mv = 0; mv <= 20000; mv += 20000)
            for (const Start& st : starts) {
                pr::Opts o;
                pr::default_opts(o);
                o.base.max_iterations = 8;
                o.base.min_valid = mv;
                o.gain0 = st.gain0;
                o.huber_k = st.k;
                pr::Record recs[pa::MAX_LEVELS];
                rr::align(i1.data(), st.img2, st.x, o, 4, recs);
                for (int L = 0; L < 4; L++) {
                    if (!std::isnan(st.x[3])) check_record(recs[L], 8);
                    if (st.flags >= 0) {
                        if (recs[L].px.flags != st.flags) printf("%s min_valid %d level %d: flags %d, n_valid0 %d\n", st.name, mv, L, recs[L].px.flags, recs[L].px.n_valid0);
                        CHECK(recs[L].px.flags == st.flags && recs[L].px.trials == 0 && recs[L].gain == 1.0 && recs[L].bias == 0.0);
                        CHECK(memcmp(recs[L].px.offsets_px, st.x, 32) == 0);
                        if (st.flags & (pa::DEGENERATE | pa::FEW_PIXELS)) {
                            CHECK(recs[L].px.n_valid0 == 0 && recs[L].px.mse0 == 0.0 && recs[L].n_outliers0 == 0);
                            for (int k = 0; k < 100; k++) CHECK(recs[L].info10[k] == 0.0);
                        }
                    } else if (mv == 0) {
                        printf("%s level %d: flags %d, trials %d, accepted %d, gain %.4g, bias %.4g, outliers %d of %d\n", st.name, L, recs[L].px.flags,
                               recs[L].px.trials, recs[L].px.accepted, recs[L].gain, recs[L].bias, recs[L].n_outliers, recs[L].px.n_valid);
                    }
                }
            }
    }
    if (failures) { printf("photo_robust_check: %d FAILED\n", failures); return 1; }
    printf("photo_robust_check: ok\n");
    return 0;
}
