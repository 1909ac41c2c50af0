// filters_innov_check.cpp — a stand-alone program over the innovation additions of include/hnet_ekf.h (innovation, iterated_update_gated), for
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_filters_innov_cpu.py).  It makes its own inputs and checks:
//   1. innovation(): r and s_diag against their definitions, the NIS against r . y with S y = r solved by elimination (no inverse) - 1e-10 relative;
//   2. iterated_update_gated with the gate off against iterated_update: state, return value and network calls, bit for bit, 1 - 3 iterations, reference
//      gate open and closed;
//   3. the gate rule: max_nis just below / above the NIS of iteration 0, a rejection at iteration 1 that keeps update 0, and every flag
//      (NONE, USED, REJECTED, SKIPPED, SINGULAR with zero P and zero network covariance).
// Build: g++ -std=c++14 -I include tests/cpp/filters_innov_check.cpp -o <program>
#include "hnet_ekf.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace hnet_ekf;

namespace {
// a small deterministic generator (no <random>: the values only have to be varied)
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
    const double* cur = nullptr;
    struct M { const double* v; double operator()(int i, int j) const { return v[i * 8 + j]; } };
    struct V { const double* v; double operator()(int i, int) const { return v[i]; } };
    template <class P> void network_inference(const P&, int it) { cur = net72 + (size_t)it * 72; calls++; }
    double get_latest_inference_time() const { return open ? t_frame : t_frame - 1.0; }
    V get_pred_mean() const { return V{cur}; }
    M get_pred_Cov() const { return M{cur + 8}; }
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
// mean near the prior (in pixels) with an offset of `spread` pixels, an SPD covariance in pixels squared
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
// S y = r by elimination with partial pivoting
bool solve8(double* S, double* r) {
    for (int c = 0; c < 8; c++) {
        int p = c;
        for (int i = c + 1; i < 8; i++)
            if (std::fabs(S[i * 8 + c]) > std::fabs(S[p * 8 + c])) p = i;
        if (S[p * 8 + c] == 0.0) return false;
        for (int j = 0; j < 8; j++) { const double t = S[c * 8 + j]; S[c * 8 + j] = S[p * 8 + j]; S[p * 8 + j] = t; }
        { const double t = r[c]; r[c] = r[p]; r[p] = t; }
        for (int i = c + 1; i < 8; i++) {
            const double f = S[i * 8 + c] / S[c * 8 + c];
            for (int j = c; j < 8; j++) S[i * 8 + j] -= f * S[c * 8 + j];
            r[i] -= f * r[c];
        }
    }
    for (int c = 7; c >= 0; c--) {
        for (int j = c + 1; j < 8; j++) r[c] -= S[c * 8 + j] * r[j];
        r[c] /= S[c * 8 + c];
    }
    return true;
}
bool same(const State& a, const State& b) { return std::memcmp(&a, &b, sizeof a) == 0; }
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } } while (0)
}  // namespace

int main() {
    Lcg g{77};
    const double kc = 10.0;
    // 1. the record against its definition
    double worst = 0.0;
    for (int c = 0; c < 50; c++) {
        State s;
        random_state(g, s);
        double net[72], px[8], cam[8];
        random_net(g, s, 4.0, net);
        prior_pixels(s, px, cam);
        const State before = s;
        Innovation o;
        CHECK(innovation(s, net, net + 8, cam, kc, o) && o.flag == INNOV_USED && same(s, before));
        double S[64], r[8], y[8];
        for (int i = 0; i < 8; i++) {
            r[i] = net[i] / F_PIX - cam[i];
            for (int j = 0; j < 8; j++)
                S[i * 8 + j] = s.cov[(15 + 3 * (i / 2) + i % 2) * NS + 15 + 3 * (j / 2) + j % 2] + kc * net[8 + i * 8 + j] / (F_PIX * F_PIX);
        }
        for (int i = 0; i < 8; i++) {
            CHECK(o.r[i] == r[i] && o.s_diag[i] == S[i * 8 + i]);
            y[i] = r[i];
        }
        CHECK(solve8(S, y));
        double nis = 0.0;
        for (int i = 0; i < 8; i++) nis += r[i] * y[i];
        CHECK(nis > 0.0);
        const double rel = std::fabs(o.nis - nis) / nis;
        worst = rel > worst ? rel : worst;
        CHECK(rel < 1e-10);
    }
    // 2. gate off: iterated_update, bit for bit
    int compared = 0;
    for (int iters = 1; iters <= 3; iters++)
        for (int open = 0; open < 2; open++)
            for (int c = 0; c < 4; c++) {
                State s;
                random_state(g, s);
                std::vector<double> net((size_t)iters * 72);
                for (int it = 0; it < iters; it++) random_net(g, s, 4.0, &net[(size_t)it * 72]);
                State a = s, b = s;
                FakeNet na{net.data(), open != 0, 2.5, 12}, nb = na;
                double pa[8], pb[8];
                std::vector<Innovation> rec(iters);
                const int da = iterated_update(a, na, iters, kc, pa, 2.5);
                const int db = iterated_update_gated(b, nb, iters, kc, pb, 2.5, c % 2 ? 0.0 : -1.0, rec.data());
                CHECK(da == db && da == (open ? iters : 0) && na.calls == nb.calls && same(a, b) && std::memcmp(pa, pb, sizeof pa) == 0);
                for (int it = 0; it < iters; it++) CHECK(rec[it].flag == (open ? INNOV_USED : INNOV_NONE));
                if (!open) CHECK(rec[0].nis == 0.0 && rec[0].r[3] == 0.0);
                compared++;
            }
    // 3. the gate rule
    for (int iters = 1; iters <= 3; iters++) {
        State s;
        random_state(g, s);
        std::vector<double> net((size_t)iters * 72);
        for (int it = 0; it < iters; it++) random_net(g, s, it == 1 ? 60.0 : 4.0, &net[(size_t)it * 72]);      // iteration 1 disagrees strongly
        std::vector<Innovation> ungated(iters), rec(iters);
        State u = s;
        double pv[8];
        FakeNet n0{net.data(), true, 2.5, 12};
        CHECK(iterated_update_gated(u, n0, iters, kc, pv, 2.5, 0.0, ungated.data()) == iters);
        const double nis0 = ungated[0].nis;
        CHECK(nis0 > 0.0);
        // just above: nothing rejected unless iteration 1 is beyond it as well
        if (iters == 1) {
            State a = s;
            FakeNet n1{net.data(), true, 2.5, 12};
            CHECK(iterated_update_gated(a, n1, iters, kc, pv, 2.5, nis0 * (1 + 1e-12), rec.data()) == 1 && same(a, u) && rec[0].flag == INNOV_USED);
        }
        // just below: no update at all, only the reset; the network still runs in every iteration
        State a = s, want = s;
        reset_4pt_offset(want);
        FakeNet n2{net.data(), true, 2.5, 12};
        CHECK(iterated_update_gated(a, n2, iters, kc, pv, 2.5, nis0 * (1 - 1e-12), rec.data()) == 0 && same(a, want) && n2.calls == iters);
        CHECK(rec[0].flag == INNOV_REJECTED && rec[0].nis == nis0);
        for (int it = 1; it < iters; it++) CHECK(rec[it].flag == INNOV_SKIPPED && rec[it].nis == 0.0);
        if (iters >= 2) {
            // a gate between the two: update 0 stays, iteration 1 is rejected, iteration 2 skipped
            CHECK(ungated[1].nis > 4 * nis0);
            State b = s, w2 = s;
            double px[8], cam[8];
            prior_pixels(w2, px, cam);
            CHECK(update(w2, net.data(), net.data() + 8, cam, kc, true));
            reset_4pt_offset(w2);
            FakeNet n3{net.data(), true, 2.5, 12};
            CHECK(iterated_update_gated(b, n3, iters, kc, pv, 2.5, 2 * nis0, rec.data()) == 1 && same(b, w2) && n3.calls == iters);
            CHECK(rec[0].flag == INNOV_USED && rec[1].flag == INNOV_REJECTED && rec[1].nis == ungated[1].nis);
            if (iters == 3) CHECK(rec[2].flag == INNOV_SKIPPED);
        }
        // singular: zero P and zero network covariance
        State z = s;
        std::memset(z.cov, 0, sizeof z.cov);
        std::vector<double> zn = net;
        for (int it = 0; it < iters; it++) std::memset(&zn[(size_t)it * 72 + 8], 0, 64 * sizeof(double));
        State zp = z, zg = z;
        FakeNet n4{zn.data(), true, 2.5, 12}, n5 = n4;
        const int dp = iterated_update(zp, n4, iters, kc, pv, 2.5);
        const int dg = iterated_update_gated(zg, n5, iters, kc, pv, 2.5, 15.507, rec.data());
        CHECK(dp == 0 && dg == 0 && same(zp, zg) && n4.calls == n5.calls && n5.calls == 1);
        CHECK(rec[0].flag == INNOV_SINGULAR && std::isnan(rec[0].nis) && rec[0].s_diag[0] == 0.0);
        for (int it = 1; it < iters; it++) CHECK(rec[it].flag == INNOV_SKIPPED);
    }
    std::printf("innovation check: worst relative NIS difference %.3g, %d gate-off cases equal, gate rule ok\n", worst, compared);
    return 0;
}
