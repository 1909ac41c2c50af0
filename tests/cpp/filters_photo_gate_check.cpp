// filters_photo_gate_check.cpp — a stand-alone program over the photometric-gate additions of include/hnet_ekf.h (photo_reject,
// iterated_update_photo_gated), for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_filters_photo_gate_cpu.py).  It makes its own inputs and
// checks:
//   1. photo_reject at its edges: off, DEGENERATE and too few pixels inside on either side, NaN sums, exact equality of the two products;
//   2. iterated_update_photo_gated with max_ratio <= 0 against iterated_update_gated: state, return value, records and network calls, bit for bit,
//      1 - 3 iterations, reference gate open and closed, with and without a NIS gate; the photometric callable is never called;
//   3. the loop: a rejection at iteration 0, 1 and 2 of 3 (updates applied, both kinds of flags, the state against a NIS rejection at the same iteration),
//      a NIS rejection and a singular S before a would-be photometric rejection.
// Build: g++ -std=c++14 -I include tests/cpp/filters_photo_gate_check.cpp -o <program>
#include "hnet_ekf.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace hnet_ekf;

namespace {
struct Lcg {
    unsigned long long s;
    double next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0 - 0.5; }
};

struct FakeNet {
    const double* net72;                 // [iters][72]: mean 8 | cov 64
    bool open;
    double t_frame;
    int img_counter;
    int calls = 0;
    int it = -1;
    const double* cur = nullptr;
    struct M { const double* v; double operator()(int i, int j) const { return v[i * 8 + j]; } };
    struct V { const double* v; double operator()(int i, int) const { return v[i]; } };
    template <class P> void network_inference(const P&, int iteration) { cur = net72 + (size_t)iteration * 72; it = iteration; calls++; }
    double get_latest_inference_time() const { return open ? t_frame : t_frame - 1.0; }
    V get_pred_mean() const { return V{cur}; }
    M get_pred_Cov() const { return M{cur + 8}; }
};
// scripted records: [0] of the prior (asked for before the first forward), [1 + it] of forward it's mean
struct Script {
    const FakeNet* net;
    const PhotoRecord* rec;
    int calls = 0;
    PhotoRecord operator()(const double*) { calls++; return rec[net->it < 0 ? 0 : 1 + net->it]; }
};

void random_state(Lcg& g, State& s) {
    std::memset(&s, 0, sizeof s);
    s.q[0] = 1.0;
    s.p[2] = -1.2;
    for (int i = 0; i < 3; i++) { s.v[i] = g.next(); s.ba[i] = 0.1 * g.next(); s.bg[i] = 0.01 * g.next(); }
    for (int c = 0; c < 4; c++)
        for (int k = 0; k < 3; k++) s.offset[c][k] = 0.01 * g.next();
    std::vector<double> a(NS * NS);
    for (auto& x : a) x = 0.02 * g.next();
    for (int i = 0; i < NS; i++)
        for (int j = 0; j < NS; j++) {
            double v = i == j ? 1e-4 : 0.0;
            for (int k = 0; k < NS; k++) v += a[i * NS + k] * a[j * NS + k];
            s.cov[i * NS + j] = v;
        }
}
void random_net(Lcg& g, const State& s, double spread, double* net72) {
    double px[8], cam[8];
    prior_pixels(s, px, cam);
    for (int i = 0; i < 8; i++) net72[i] = px[i] + spread * g.next();
    double a[64];
    for (auto& x : a) x = 3.0 * g.next();
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) {
            double v = i == j ? 0.5 : 0.0;
            for (int k = 0; k < 8; k++) v += a[i * 8 + k] * a[j * 8 + k];
            net72[8 + i * 8 + j] = v;
        }
}
bool same(const State& a, const State& b) { return std::memcmp(&a, &b, sizeof a) == 0; }
PhotoRecord rec(double sum_inside, int n, int flags = 0) { return PhotoRecord{sum_inside + 5.0, sum_inside, n, flags}; }
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } } while (0)
}  // namespace

int main() {
    Lcg g{91};
    const double kc = 10.0;
    // 1. the rule
    {
        const PhotoRecord p = rec(1000.0, 50000), e = rec(3000.0, 50000);
        CHECK(photo_reject(p, e, 2.0, 0) && !photo_reject(p, e, 4.0, 0));
        CHECK(!photo_reject(p, e, 0.0, 0) && !photo_reject(p, e, -1.0, 0) && !photo_reject(p, rec(0.0, 0, PHOTO_DEGENERATE), 0.0, 0));
        CHECK(photo_reject(p, rec(10.0, 50000, PHOTO_DEGENERATE), 1e30, 0) && !photo_reject(rec(1000.0, 50000, PHOTO_DEGENERATE), e, 2.0, 0));
        CHECK(photo_reject(p, rec(0.0, 0), 1e30, 0) && !photo_reject(rec(0.0, 0), e, 2.0, 0));
        CHECK(photo_reject(p, rec(3000.0, 49999), 4.0, 50000) && !photo_reject(p, rec(3000.0, 50000), 4.0, 50000));
        CHECK(!photo_reject(rec(1000.0, 49999), e, 2.0, 50000) && photo_reject(rec(1000.0, 50000), e, 2.0, 50000));
        CHECK(!photo_reject(p, rec((double)NAN, 50000), 2.0, 0) && !photo_reject(rec((double)NAN, 50000), e, 2.0, 0));
        const PhotoRecord p2 = rec(1024.0, 40000), e2 = rec(1536.0, 20000);          // 1536 x 40000 == (3 x 1024) x 20000
        CHECK(!photo_reject(p2, e2, 3.0, 0) && photo_reject(p2, rec(std::nextafter(1536.0, 2000.0), 20000), 3.0, 0));
    }
    // 2. gate off: iterated_update_gated, bit for bit
    int compared = 0;
    for (int iters = 1; iters <= 3; iters++)
        for (int open = 0; open < 2; open++)
            for (int c = 0; c < 4; c++) {
                State s;
                random_state(g, s);
                std::vector<double> net((size_t)iters * 72);
                for (int it = 0; it < iters; it++) random_net(g, s, it == 1 ? 60.0 : 4.0, &net[(size_t)it * 72]);
                std::vector<Innovation> r0(iters), ra(iters), rb(iters);
                std::vector<PhotoRecord> script(1 + iters, rec(9e9, 50000)), prec(1 + iters);
                script[0] = rec(1.0, 50000);
                double pv[8], pa[8], pb[8];
                State u = s;
                FakeNet n0{net.data(), open != 0, 2.5, 12};
                iterated_update_gated(u, n0, iters, kc, pv, 2.5, 0.0, r0.data());
                const double max_nis = c < 2 ? 0.0 : 2.0 * r0[0].nis;                 // (with iteration 1 disagreeing: a rejection there)
                State a = s, b = s;
                FakeNet na{net.data(), open != 0, 2.5, 12}, nb = na;
                Script ph{&nb, script.data()};
                const int da = iterated_update_gated(a, na, iters, kc, pa, 2.5, max_nis, ra.data());
                const int db = iterated_update_photo_gated(b, nb, iters, kc, pb, 2.5, max_nis, rb.data(), ph, c % 2 ? 0.0 : -1.0, 0, prec.data());
                CHECK(da == db && na.calls == nb.calls && nb.calls == iters && same(a, b) && std::memcmp(pa, pb, sizeof pa) == 0 && ph.calls == 0);
                for (int it = 0; it < iters; it++) CHECK(std::memcmp(&ra[it], &rb[it], sizeof ra[it]) == 0);
                for (int k = 0; k <= iters; k++) CHECK(prec[k].n_inside == 0 && prec[k].flags == 0 && prec[k].sum == 0.0);
                compared++;
            }
    // 3. the loop
    for (int at = 0; at < 3; at++) {
        const int iters = 3;
        State s;
        random_state(g, s);
        std::vector<double> net((size_t)iters * 72);
        for (int it = 0; it < iters; it++) random_net(g, s, 4.0, &net[(size_t)it * 72]);
        std::vector<PhotoRecord> script(1 + iters, rec(500.0, 50000)), prec(1 + iters);
        script[0] = rec(1000.0, 50000);
        script[1 + at] = rec(2500.0, 50000);
        std::vector<Innovation> r(iters), rn(iters), r0(iters);
        double pv[8];
        State a = s;
        FakeNet na{net.data(), true, 2.5, 12};
        Script ph{&na, script.data()};
        CHECK(iterated_update_photo_gated(a, na, iters, kc, pv, 2.5, 0.0, r.data(), ph, 2.0, 0, prec.data()) == at && na.calls == iters && ph.calls == 2 + at);
        for (int it = 0; it < iters; it++) {
            CHECK(r[it].flag == (it < at ? INNOV_USED : INNOV_SKIPPED));
            CHECK(prec[1 + it].flags == (it == at ? PHOTO_REJECTED : 0) && prec[1 + it].n_inside == (it <= at ? 50000 : 0));
            if (it >= at) CHECK(r[it].nis == 0.0 && r[it].r[0] == 0.0);
        }
        // the same updates through a NIS rejection at `at`
        State u = s;
        FakeNet n0{net.data(), true, 2.5, 12};
        CHECK(iterated_update_gated(u, n0, iters, kc, pv, 2.5, 0.0, r0.data()) == iters);
        double top = 0.0;
        for (int it = 0; it < iters; it++) top = r0[it].nis > top ? r0[it].nis : top;
        std::vector<double> huge = net;
        for (int i = 0; i < 8; i++) huge[(size_t)at * 72 + i] += 1e4;
        State b = s;
        FakeNet nb{huge.data(), true, 2.5, 12};
        CHECK(iterated_update_gated(b, nb, iters, kc, pv, 2.5, 10.0 * top, rn.data()) == at && rn[at].flag == INNOV_REJECTED && same(a, b));
        // a NIS rejection at iteration 1 before a would-be photometric rejection at iteration 2
        if (at == 2) {
            State c = s;
            FakeNet nc{huge.data(), true, 2.5, 12};
            for (int i = 0; i < 8; i++) { huge[(size_t)2 * 72 + i] -= 1e4; huge[(size_t)1 * 72 + i] += 1e4; }
            Script pc{&nc, script.data()};
            CHECK(iterated_update_photo_gated(c, nc, iters, kc, pv, 2.5, 10.0 * top, r.data(), pc, 2.0, 0, prec.data()) == 1 && pc.calls == 3);
            CHECK(r[0].flag == INNOV_USED && r[1].flag == INNOV_REJECTED && r[2].flag == INNOV_SKIPPED);
            for (int k = 0; k <= iters; k++) CHECK(!(prec[k].flags & PHOTO_REJECTED));
            CHECK(prec[3].n_inside == 0);
        }
        // singular S at iteration 0: the loop ends, nothing later is judged
        State z = s;
        std::memset(z.cov, 0, sizeof z.cov);
        std::vector<double> zn = net;
        for (int it = 0; it < iters; it++) std::memset(&zn[(size_t)it * 72 + 8], 0, 64 * sizeof(double));
        script[1] = rec(500.0, 50000);
        script[2] = rec(9000.0, 50000);
        FakeNet nz{zn.data(), true, 2.5, 12};
        Script pz{&nz, script.data()};
        CHECK(iterated_update_photo_gated(z, nz, iters, kc, pv, 2.5, 0.0, r.data(), pz, 2.0, 0, prec.data()) == 0 && nz.calls == 1 && pz.calls == 2);
        CHECK(r[0].flag == INNOV_SINGULAR && r[1].flag == INNOV_SKIPPED && r[2].flag == INNOV_SKIPPED);
        for (int k = 0; k <= iters; k++) CHECK(!(prec[k].flags & PHOTO_REJECTED));
    }
    std::printf("photometric gate check: %d gate-off cases equal, rule and loop ok\n", compared);
    return 0;
}
