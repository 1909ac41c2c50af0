// filters_photo_refine_check.cpp — include/hnet_photo_refine.h as a stand-alone program for AddressSanitizer + UBSan (tests/test_filters_photo_refine_cpu.py):
// refine_measurement on a synthetic record (usable, and every UNUSABLE reason), the marginal against a direct Schur complement, and
// hnet_ekf::iterated_update_photo_refined with a scripted gate and a stub aligner on its paths.  No image, no library: the header is dependency free.
// Build: g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I include tests/cpp/filters_photo_refine_check.cpp -o check && ./check
#include "hnet_photo_refine.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace hnet_ekf;
namespace rf = hnet_refine;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static double rnd(unsigned& s) { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24) - 0.5; }

static hnet_robust::Record make_record(unsigned seed) {
    hnet_robust::Record r;
    std::memset(&r, 0, sizeof r);
    double M[100];
    for (double& m : M) m = rnd(seed) * 30.0;
    for (int i = 0; i < 10; i++)
        for (int j = 0; j < 10; j++) {
            double a = i == j ? 500.0 : 0.0;
            for (int k = 0; k < 10; k++) a += M[i * 10 + k] * M[j * 10 + k];
            r.info10[i * 10 + j] = a;
        }
    for (int i = 0; i < 10; i++) r.grad10[i] = rnd(seed);
    for (int i = 0; i < 8; i++) {
        r.px.offsets_px[i] = (float)(rnd(seed) * 2.0);
        r.px.grad[i] = r.grad10[i];
        for (int j = 0; j < 8; j++) r.px.info[i * 8 + j] = r.info10[i * 10 + j];
    }
    r.px.mse0 = 40.0;
    r.px.mse = 25.0;
    r.px.n_valid0 = r.px.n_valid = 70000;
    r.px.trials = 3;
    r.px.accepted = 2;
    r.px.flags = hnet_align::CONVERGED;
    r.gain = 1.0;
    return r;
}

struct FakeNet {
    const float* net72;
    double t_frame;
    int img_counter = 11, calls = 0, it = -1;
    const float* cur = nullptr;
    struct M { const float* v; double operator()(int i, int j) const { return v[i * 8 + j]; } };
    struct V { const float* v; double operator()(int i, int) const { return v[i]; } };
    template <class P> void network_inference(const P&, int iteration) { cur = net72 + (size_t)iteration * 72; it = iteration; calls++; }
    double get_latest_inference_time() const { return t_frame; }
    V get_pred_mean() const { return V{cur}; }
    M get_pred_Cov() const { return M{cur + 8}; }
};
struct Script {
    const FakeNet* net;
    const double* ratio;                 // per iteration: the estimate's mean residual over the prior's
    PhotoRecord operator()(const double*) { return PhotoRecord{1000.0 * (net->it < 0 ? 1.0 : ratio[net->it]) + 3.0, 1000.0 * (net->it < 0 ? 1.0 : ratio[net->it]), 50000, 0}; }
};
struct Stub {
    hnet_robust::Record rec;
    int accepted, calls = 0;
    void operator()(const float* x0, hnet_robust::Record& out, int& acc) {
        calls++;
        out = rec;
        for (int i = 0; i < 8; i++) out.px.offsets_px[i] = x0[i] + 0.25f;
        acc = accepted;
    }
};

static State make_state(unsigned seed) {
    static State s;
    std::memset(&s, 0, sizeof s);
    s.q[0] = 1.0;
    for (int c = 0; c < 4; c++)
        for (int k = 0; k < 3; k++) s.offset[c][k] = rnd(seed) * 0.01;
    std::vector<double> A(NS * NS);
    for (double& a : A) a = rnd(seed) * 0.02;
    for (int i = 0; i < NS; i++)
        for (int j = 0; j < NS; j++) {
            double a = i == j ? 1e-4 : 0.0;
            for (int k = 0; k < NS; k++) a += A[i * NS + k] * A[j * NS + k];
            s.cov[i * NS + j] = a;
        }
    return s;
}

int main() {
    rf::Opts o;
    rf::default_opts(o);
    CHECK(!rf::opts_valid(o));           // cov_scale = 0: the caller must choose it
    o.cov_scale = 3.0;
    CHECK(rf::opts_valid(o));
    const hnet_robust::Record good = make_record(7);
    float m72[72];
    double r_px[64];
    int32_t flags = 0;
    CHECK(rf::refine_measurement(good, 2, o, 10.0, m72, r_px, flags) && flags == 0);
    // R - floor^2 I = scale * mse * inverse(info8): (R - floor) info8 = scale * mse I
    double info8[64], grad8[8];
    CHECK(rf::marginal(good, info8, grad8));
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) {
            double a = 0.0;
            for (int k = 0; k < 8; k++) a += (r_px[i * 8 + k] - (i == k ? o.sigma_floor_px * o.sigma_floor_px : 0.0)) * info8[k * 8 + j];
            CHECK(std::fabs(a - (i == j ? o.cov_scale * good.px.mse : 0.0)) < 1e-9 * o.cov_scale * good.px.mse);
            CHECK(r_px[i * 8 + j] == r_px[j * 8 + i] && m72[8 + i * 8 + j] == (float)(r_px[i * 8 + j] / 10.0));
        }
    struct { hnet_robust::Record r; int acc; double k, max_mse; int want; } cases[8] = {
        {good, 2, 0.0, 0.0, rf::BAD_K_NET_COV}, {good, 2, (double)NAN, 0.0, rf::BAD_K_NET_COV}, {good, 2, 10.0, 0.0, rf::STOPPED}, {good, 0, 10.0, 0.0, rf::NO_STEP},
        {good, 2, 10.0, 24.0, rf::MSE_ABOVE_MAX}, {good, 2, 10.0, 0.0, rf::NO_FACTOR}, {good, 2, 10.0, 0.0, rf::NO_FACTOR}, {good, 2, 10.0, 0.0, rf::NON_FINITE}};
    cases[2].r.px.flags |= hnet_align::SINGULAR;
    cases[5].r.info10[99] = cases[5].r.info10[89] * cases[5].r.info10[89] / cases[5].r.info10[88] * 0.999;      // the brightness block loses its factor
    for (int j = 0; j < 10; j++) cases[6].r.info10[3 * 10 + j] = cases[6].r.info10[j * 10 + 3] = 0.0;          // a zero row and column: rank 7
    cases[7].r.px.mse = 1e308;
    for (auto& c : cases) {
        rf::Opts oc = o;
        oc.max_mse = c.max_mse;
        if (c.want == rf::NON_FINITE) oc.cov_scale = 1e10;
        float keep72[72];
        double keep_r[64];
        for (float& v : keep72) v = 7.0f;
        for (double& v : keep_r) v = 7.0;
        int32_t fl = 0;
        CHECK(!rf::refine_measurement(c.r, c.acc, oc, c.k, keep72, keep_r, fl) && fl == c.want);
        for (float v : keep72) CHECK(v == 7.0f);
        for (double v : keep_r) CHECK(v == 7.0);
    }
    // the loop: refusal at 0 with refinement on / off, no refusal, refusal at 1, a NIS gate that refuses the fallback
    int applied = 0;
    for (int path = 0; path < 5; path++) {
        State s = make_state(100 + path), s_gated = s;
        unsigned seed = 5 + path;
        std::vector<float> net(3 * 72, 0.0f);
        for (int it = 0; it < 3; it++)
            for (int i = 0; i < 8; i++) {
                net[it * 72 + i] = (float)(s.offset[i / 2][i % 2] * F_PIX + rnd(seed) * 4.0);
                net[it * 72 + 8 + i * 9] = 2.0f;
            }
        const double ratios[5][3] = {{9, .5, .5}, {9, .5, .5}, {.5, .5, .5}, {.5, 9, .5}, {9, .5, .5}};
        const double max_nis = path == 4 ? 1e-12 : 0.0;
        FakeNet n1{net.data(), 2.5}, n2{net.data(), 2.5};
        Script p1{&n1, ratios[path]}, p2{&n2, ratios[path]};
        Stub stub{good, 2};
        Innovation rec1[3], rec2[3];
        PhotoRecord pr1[4], pr2[4];
        double prior[8];
        rf::Record out;
        const int d1 = iterated_update_photo_refined(s, n1, 3, 10.0, prior, 2.5, max_nis, rec1, p1, 2.0, 0, pr1, path == 1 ? nullptr : &o, stub, out);
        const int d2 = iterated_update_photo_gated(s_gated, n2, 3, 10.0, prior, 2.5, max_nis, rec2, p2, 2.0, 0, pr2);
        CHECK(n1.calls == 3 && std::memcmp(rec1, rec2, sizeof rec1) == 0 && std::memcmp(pr1, pr2, sizeof pr1) == 0);
        const bool same = std::memcmp(&s, &s_gated, sizeof s) == 0;
        if (path == 0) {
            CHECK(stub.calls == 1 && out.flags == (rf::ASKED | rf::APPLIED) && d1 == 1 && d2 == 0 && !same && out.iteration == 3 && out.flag == INNOV_USED);
            applied++;
        } else if (path == 4) {
            CHECK(stub.calls == 1 && out.flags == (rf::ASKED | rf::NIS_REJECTED) && d1 == 0 && same && out.flag == INNOV_REJECTED);
        } else {
            CHECK(stub.calls == 0 && out.flags == 0 && d1 == d2 && same);
        }
        for (int c = 0; c < 4; c++)
            for (int k = 0; k < 3; k++) CHECK(s.offset[c][k] == 0.0);
    }
    std::printf("photo refine check: measurement, 8 unusable cases, 5 loop paths (%d applied) ok\n", applied);
    return 0;
}
