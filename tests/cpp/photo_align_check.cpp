// photo_align_check.cpp — the core of the photometric alignment reference (tests/cpp/photo_align_ref.cpp) and the shared step function
// (include/hnet_photo_align.h) on fixed inputs, meant for AddressSanitizer + UBSan on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I <rocm>/include
//       -I cuahn_vio_amd/csrc -I include tests/cpp/photo_align_check.cpp -o photo_align_check && ./photo_align_check
// Two pairs: a smooth scene seen twice, the second time moved by (2, 1) pixels (the alignment has to find that), and the same img1 against a constant img2
// (nothing to find: SINGULAR with a zero information matrix); on the first pair also a start without a homography and one far outside.
// Then the hostile starts and options of tests/photo_hostile.py: starts on and beyond the valid bound, NaN, inf, 1e30 and 3e38 offsets, the bowtie (the
// float-to-int conversions of far-out positions are the point), a frame of noise, a black frame against a white one, and options that make the loop
// refuse: the largest legal lambda0 over 32 trials, min_valid one above the count, eps_px = 0 and 100; lambda0 above 1e100 is not valid.
// Exit status 0 = all hold.
#include "photo_align_ref.cpp"

#include <cstdlib>

namespace {
int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

constexpr int CELL = 16, LW = 24, LH = 18;      // lattice of 16-pixel cells covering 368 x 272

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
}  // namespace

int main() {
    using photo_ref::IMG_H;
    using photo_ref::IMG_W;
    using photo_ref::NPIX;
    namespace pa = hnet_align;
    const Scene scene;
    std::vector<uint8_t> i1(NPIX), i2(NPIX), flat(NPIX, 93);
    for (int v = 0; v < IMG_H; v++)
        for (int u = 0; u < IMG_W; u++) {
            i1[v * IMG_W + u] = scene.at(u + 8, v + 8);
            i2[v * IMG_W + u] = scene.at(u + 8 - 2, v + 8 - 1);           // img2(x + (2, 1)) = img1(x)
        }
    pa::Opts o;
    pa::default_opts(o);
    CHECK(pa::opts_valid(o) && o.max_iterations == 6 && o.min_valid == 20000);
    const float zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    // the moved scene from zero offsets: every corner ends at (2, 1)
    {
        pa::Record r;
        o.max_iterations = 10;
        photo_align_ref::align(i1.data(), i2.data(), zero, o, r);
        double worst = 0.0;
        for (int k = 0; k < 8; k++) worst = std::fmax(worst, std::fabs((double)r.offsets_px[k] - (k % 2 ? 1.0 : 2.0)));
        printf("moved scene: flags %d, trials %d, accepted %d, mse %.4f -> %.4f, worst corner error %.4f px\n", r.flags, r.trials, r.accepted, r.mse0, r.mse, worst);
        CHECK(worst < 0.05);
        CHECK(r.mse < r.mse0 && r.accepted >= 1 && r.accepted <= r.trials && r.trials <= 10);
        CHECK(!(r.flags & (pa::SINGULAR | pa::DEGENERATE | pa::FEW_PIXELS)));
        for (int k = 0; k < 64; k++) CHECK(std::isfinite(r.info[k]) && r.info[k] == r.info[(k % 8) * 8 + k / 8]);
        // the linearisation alone: the start offsets come back, no trial was made
        pa::Record r0;
        o.max_iterations = 0;
        photo_align_ref::align(i1.data(), i2.data(), zero, o, r0);
        CHECK(r0.trials == 0 && r0.accepted == 0 && r0.flags == 0 && r0.mse == r0.mse0 && r0.mse0 == r.mse0 && r0.n_valid0 == 223 * 319);
        CHECK(memcmp(r0.offsets_px, zero, sizeof zero) == 0);
    }
    // a constant img2: no gradient anywhere, A = 0 exactly, SINGULAR, the start offsets bit for bit
    {
        pa::Record r;
        o.max_iterations = 6;
        const float start[8] = {0.5f, -0.25f, 1.0f, 0.0f, -1.5f, 0.75f, 0.0f, 2.0f};
        photo_align_ref::align(i1.data(), flat.data(), start, o, r);
        CHECK(r.flags == pa::SINGULAR && r.trials == 0 && r.n_valid0 > 60000 && r.mse0 > 0.0 && r.mse == r.mse0);
        CHECK(memcmp(r.offsets_px, start, sizeof start) == 0);
        for (int k = 0; k < 64; k++) CHECK(r.info[k] == 0.0);
        for (int k = 0; k < 8; k++) CHECK(r.grad[k] == 0.0);
    }
    // a start whose quadrilateral is a line, and one 400 px away
    {
        pa::Record r;
        float line[8] = {0, 0, 10, 5, 20, 10, 30, 15}, far[8];
        for (int k = 0; k < 8; k++) { line[k] -= (float)hnet::p4(k); far[k] = k % 2 ? 0.0f : 400.0f; }
        photo_align_ref::align(i1.data(), i2.data(), line, o, r);
        CHECK(r.flags == pa::DEGENERATE && r.n_valid0 == 0 && r.mse0 == 0.0 && memcmp(r.offsets_px, line, sizeof line) == 0);
        for (int k = 0; k < 64; k++) CHECK(r.info[k] == 0.0);
        photo_align_ref::align(i1.data(), i2.data(), far, o, r);
        CHECK(r.flags == pa::FEW_PIXELS && r.n_valid0 == 0 && memcmp(r.offsets_px, far, sizeof far) == 0);
        for (int k = 0; k < 64; k++) CHECK(r.info[k] == 0.0);
    }
    // the step function on a hand-made system: A = diag(1 .. 8), g = A x* -> one undamped step lands on -x*; a zero row is SINGULAR
    {
        double A[64] = {}, g[8], L[64], dx[8];
        for (int i = 0; i < 8; i++) { A[i * 8 + i] = i + 1.0; g[i] = (i + 1.0) * (0.1 * i - 0.3); }
        CHECK(pa::solve_damped(A, g, 0.0, L, dx));
        for (int i = 0; i < 8; i++) CHECK(std::fabs(dx[i] + (0.1 * i - 0.3)) < 1e-15);
        CHECK(pa::solve_damped(A, g, 1.0, L, dx));
        for (int i = 0; i < 8; i++) CHECK(std::fabs(dx[i] + 0.5 * (0.1 * i - 0.3)) < 1e-15);
        A[3 * 8 + 3] = 0.0;
        CHECK(!pa::solve_damped(A, g, 1e-3, L, dx));
        A[3 * 8 + 3] = NAN;
        CHECK(!pa::solve_damped(A, g, 1e-3, L, dx));
    }
    // hostile starts, min_valid = 0: n_valid0 depends on the start alone (the table of test_photo_hostile_cpu.py)
    {
        const float big = 1e30f, huge = 3e38f, inf = INFINITY;
        struct Start { const char* name; float x[8]; int n_valid0, flags; bool pin_flags; };
        const Start starts[] = {
            {"shift(1,0)", {1, 0, 1, 0, 1, 0, 1, 0}, 223 * 318, 0, true},
            {"shift(0,1)", {0, 1, 0, 1, 0, 1, 0, 1}, 222 * 319, 0, true},
            {"shift(-1,-1)", {-1, -1, -1, -1, -1, -1, -1, -1}, 71137, 0, true},
            {"shift(310,0)", {310, 0, 310, 0, 310, 0, 310, 0}, 2007, 0, false},               // (flags 0 or SINGULAR: the scene's business)
            {"shift(318,0)", {318, 0, 318, 0, 318, 0, 318, 0}, 223, pa::SINGULAR, true},
            {"shift(0,222)", {0, 222, 0, 222, 0, 222, 0, 222}, 319, pa::SINGULAR, true},
            {"shift(319,0)", {319, 0, 319, 0, 319, 0, 319, 0}, 0, pa::FEW_PIXELS, true},
            {"shift(0,223)", {0, 223, 0, 223, 0, 223, 0, 223}, 0, pa::FEW_PIXELS, true},
            {"nan", {NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN}, 0, pa::DEGENERATE, true},
            {"inf", {0, 0, 0, inf, 0, 0, 0, 0}, 0, pa::DEGENERATE, true},
            {"1e30all", {big, big, big, big, big, big, big, big}, 0, pa::DEGENERATE, true},
            {"1e30one", {big, 0, 0, 0, 0, 0, 0, 0}, 0, pa::FEW_PIXELS, true},
            {"3e38", {huge, huge, 0, 0, 0, 0, 0, 0}, 23941, pa::SINGULAR, false},
            {"bowtie", {319, 0, 0, 0, 0, 0, -319, 0}, 639, 0, false},
        };
        constexpr int N = sizeof starts / sizeof starts[0];
        std::vector<float> xs(N * 8);
        std::vector<int32_t> edges(N, -1);
        for (int b = 0; b < N; b++) memcpy(&xs[b * 8], starts[b].x, sizeof starts[b].x);
        photo_align_ref_edge(nullptr, nullptr, N, xs.data(), edges.data());
        for (int K = 0; K <= 6; K += 6)
            for (int b = 0; b < N; b++) {
                pa::Record r;
                pa::default_opts(o);
                o.max_iterations = K;
                o.min_valid = 0;
                photo_align_ref::align(i1.data(), i2.data(), starts[b].x, o, r);
                if (r.n_valid0 != starts[b].n_valid0 || (K == 0 && starts[b].pin_flags && r.flags != starts[b].flags))
                    printf("%s K=%d: n_valid0 %d, flags %d, n_edge %d\n", starts[b].name, K, r.n_valid0, r.flags, edges[b]);
                CHECK(r.n_valid0 == starts[b].n_valid0);
                if (K == 0 && starts[b].pin_flags) CHECK(r.flags == starts[b].flags);
                CHECK(r.accepted <= r.trials && r.trials <= K && std::isfinite(r.mse0) && std::isfinite(r.mse) && std::isfinite(r.lambda));
                for (int k = 0; k < 64; k++) CHECK(std::isfinite(r.info[k]));
                for (int k = 0; k < 8; k++) CHECK(std::isfinite(r.grad[k]));
                if (r.flags & (pa::DEGENERATE | pa::FEW_PIXELS)) CHECK(r.trials == 0 && r.mse0 == 0.0 && memcmp(r.offsets_px, starts[b].x, 32) == 0);
                CHECK(edges[b] >= 0 && edges[b] <= NPIX);
            }
        CHECK(edges[8] == 0 && edges[0] > 0);
    }
    // options that make the loop refuse, on the moved scene from zero offsets
    {
        pa::Record r, d;
        pa::default_opts(o);
        o.max_iterations = 10;
        photo_align_ref::align(i1.data(), i2.data(), zero, o, d);
        o.eps_px = 0.0;                                                      // never CONVERGED
        photo_align_ref::align(i1.data(), i2.data(), zero, o, r);
        CHECK(!(r.flags & pa::CONVERGED) && r.trials == 10 && r.mse <= d.mse);
        o.eps_px = 100.0;                                                    // the first accepted step is CONVERGED
        photo_align_ref::align(i1.data(), i2.data(), zero, o, r);
        CHECK(r.flags == pa::CONVERGED && r.accepted == 1 && r.trials >= 1);
        pa::default_opts(o);
        o.max_iterations = 32;
        o.lambda0 = pa::MAX_LAMBDA0;                                         // the largest legal damping: 32 refusals, lambda 1e132, never SINGULAR
        CHECK(pa::opts_valid(o));
        photo_align_ref::align(i1.data(), i2.data(), zero, o, r);
        printf("lambda0 1e100: flags %d, trials %d, accepted %d, lambda %.3g\n", r.flags, r.trials, r.accepted, r.lambda);
        CHECK(r.flags == 0 && r.trials == 32 && r.accepted == 0 && r.lambda > 0.99e132 && r.lambda < 1.01e132 && memcmp(r.offsets_px, zero, 32) == 0);
        for (double lam : {1e280, 1e290, 1e300, 1.0000001e100, (double)INFINITY, (double)NAN, 0.0, -1.0}) {
            o.lambda0 = lam;
            CHECK(!pa::opts_valid(o) && !photo_align_ref_opts_valid(&o));
        }
        o.lambda0 = 1e-300;
        CHECK(pa::opts_valid(o));
        o.max_iterations = 10;
        photo_align_ref::align(i1.data(), i2.data(), zero, o, r);
        CHECK(r.trials == d.trials && r.accepted == d.accepted && r.flags == d.flags && std::isfinite(r.lambda) && r.lambda > 0.0);
        pa::default_opts(o);
        o.min_valid = 223 * 319 + 1;
        photo_align_ref::align(i1.data(), i2.data(), zero, o, r);
        CHECK(r.flags == pa::FEW_PIXELS && r.n_valid0 == 223 * 319 && r.trials == 0);
        o.min_valid = 223 * 319;                                             // every trial is judged on its count too
        photo_align_ref::align(i1.data(), i2.data(), zero, o, r);
        CHECK(!(r.flags & pa::FEW_PIXELS) && r.n_valid >= 223 * 319 && r.trials >= 1);
    }
    // maximal gradients: a frame of noise against itself moved by (2, 1), and a black frame against a white one (no gradient, the largest residual)
    {
        std::vector<uint8_t> n1(NPIX), n2(NPIX), black(NPIX, 0), white(NPIX, 255);
        uint32_t s = 777u;
        for (int i = 0; i < NPIX; i++) {
            s = s * 1664525u + 1013904223u;
            n1[i] = (uint8_t)(s >> 24);
        }
        for (int v = 0; v < IMG_H; v++)
            for (int u = 0; u < IMG_W; u++) n2[v * IMG_W + u] = n1[((v + IMG_H - 1) % IMG_H) * IMG_W + (u + IMG_W - 2) % IMG_W];
        pa::Record r;
        pa::default_opts(o);
        photo_align_ref::align(n1.data(), n2.data(), zero, o, r);
        CHECK(!(r.flags & (pa::SINGULAR | pa::DEGENERATE | pa::FEW_PIXELS)) && r.mse <= r.mse0 && std::isfinite(r.mse0) && std::isfinite(r.lambda));
        for (int k = 0; k < 64; k++) CHECK(std::isfinite(r.info[k]));
        photo_align_ref::align(black.data(), white.data(), zero, o, r);
        CHECK(r.flags == pa::SINGULAR && r.mse0 == 255.0 * 255.0 && r.trials == 0);
        for (int k = 0; k < 64; k++) CHECK(r.info[k] == 0.0);
    }
    if (failures) { printf("photo_align_check: %d FAILED\n", failures); return 1; }
    printf("photo_align_check: ok\n");
    return 0;
}
