// filters_feed_ref.cpp — the host reference of the fed filters (include/hnet.h, hnet_filters_feed_imu / hnet_filters_advance) as a small shared library for
// the tests and tools/filters_bench.py: include/hnet_ekf.h's initialize_with_imu / initialize_cov / trim_imu_* / select_span behind a C interface on
// the hnet.h structs.  Build: g++ -std=c++17 -O2 -shared -fPIC -I include tests/cpp/filters_feed_ref.cpp -o <lib>.so
// With -DFEED_CHECK_MAIN it is a program that runs the same functions on streams it makes itself (tests/test_sanitizers_feed_cpu.py: ASan + UBSan).
#include "hnet.h"
#include "hnet_ekf.h"

#include <cstdio>
#include <cstring>
#include <vector>

using hnet_ekf::ImuData;
using hnet_ekf::State;

static_assert(sizeof(hnet_filter_state) == sizeof(double) + sizeof(State), "hnet_filter_state = t + hnet_ekf::State");
static_assert(sizeof(hnet_imu) == sizeof(ImuData), "hnet_imu = hnet_ekf::ImuData");

namespace {
const ImuData* rd(const hnet_imu* r) { return reinterpret_cast<const ImuData*>(r); }
}  // namespace

extern "C" {

// hnet_ekf::initialize_with_imu on r[0 .. n) (already trimmed by the caller): 1 and st = {time0, the mean; offsets and covariance untouched}, or 0
int feed_ref_init(const hnet_imu* r, int n, const hnet_init_params* ip, double gravity_mag, hnet_filter_state* st) {
    State s;
    std::memcpy(&s, &st->p[0], sizeof s);
    double time0 = 0.0;
    if (!hnet_ekf::initialize_with_imu(rd(r), n, ip->window_time, ip->imu_thresh, ip->init_height, ip->wait_for_jerk != 0, gravity_mag, time0, s)) return 0;
    std::memcpy(&st->p[0], &s, sizeof s);
    st->t = time0;
    return 1;
}

void feed_ref_init_cov(hnet_filter_state* st) {
    State s;
    std::memcpy(&s, &st->p[0], sizeof s);
    hnet_ekf::initialize_cov(s);
    std::memcpy(&st->p[0], &s, sizeof s);
}

int feed_ref_trim_init(const hnet_imu* r, int n, double newest, double window_time) { return hnet_ekf::trim_imu_init(rd(r), n, newest, window_time); }
int feed_ref_trim_prop(const hnet_imu* r, int n, double newest) { return hnet_ekf::trim_imu_prop(rd(r), n, newest); }

int feed_ref_select(const hnet_imu* r, int n, double t0, double t1, hnet_imu* out) {
    return hnet_ekf::select_imu_readings(rd(r), n, t0, t1, reinterpret_cast<ImuData*>(out));
}

// the device's way: the two counts (here by a plain loop), hnet_ekf::select_span, then select_imu_readings on that span only.  span[2]: first, len
int feed_ref_select_span(const hnet_imu* r, int n, double t0, double t1, hnet_imu* out, int* span) {
    int n_lt = 0, n_le = 0;
    for (int i = 0; i < n; i++) {
        n_lt += r[i].t < t0;
        n_le += r[i].t <= t1;
    }
    int first = 0;
    const int len = hnet_ekf::select_span(n, n_lt, n_le, &first);
    if (span) { span[0] = first; span[1] = len; }
    return hnet_ekf::select_imu_readings(rd(r) + first, len, t0, t1, reinterpret_cast<ImuData*>(out));
}

}  // extern "C"

#ifdef FEED_CHECK_MAIN
namespace {
// a small deterministic generator (no <random>: the values only have to be varied)
struct Lcg {
    unsigned long long s;
    double next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0 - 0.5; }
};
std::vector<hnet_imu> stream(int n, double dt, double t_jerk, double amp, Lcg& g) {
    std::vector<hnet_imu> r(n);
    for (int i = 0; i < n; i++) {
        r[i].t = i * dt;
        const double a = r[i].t >= t_jerk ? amp : 0.01;
        for (int k = 0; k < 3; k++) { r[i].wm[k] = 0.01 * g.next(); r[i].am[k] = a * g.next(); }
        r[i].am[2] += 9.7;
        r[i].am[0] += 1.3;
    }
    return r;
}
}  // namespace

int main() {
    Lcg g{12345};
    hnet_init_params ip = {1.0, 0.5, 0.1, 1};
    int accepted = 0, refused = 0;
    for (int c = 0; c < 6; c++) {
        // still then jerk, always moving, never moving, too short, one-reading windows, no readings
        const int n = c == 3 ? 150 : c == 4 ? 3 : c == 5 ? 0 : 600;
        std::vector<hnet_imu> r = stream(n, c == 4 ? 1.0 : 0.005, c == 1 ? 0.0 : c == 2 ? 1e9 : 2.0, 8.0, g);
        const int k = n ? feed_ref_trim_init(r.data(), n, r[n - 1].t, ip.window_time) : 0;
        hnet_filter_state st;
        std::memset(&st, 0, sizeof st);
        if (feed_ref_init(r.data() + k, n - k, &ip, 9.81, &st)) {
            feed_ref_init_cov(&st);
            accepted++;
            if (!(st.cov[2 * 27 + 2] >= 0.0) || !(st.q[0] == st.q[0])) return 2;
        } else refused++;
        if (n && feed_ref_trim_prop(r.data(), n, r[n - 1].t + 11.0 - r[n / 2].t) < 0) return 3;
    }
    // select on the span == select on the whole history, on random windows over histories with repeated stamps
    int compared = 0;
    for (int c = 0; c < 400; c++) {
        const int n = (int)((g.next() + 0.5) * 40);
        std::vector<hnet_imu> r(n);
        double t = g.next();
        for (int i = 0; i < n; i++) {
            t += g.next() < -0.3 ? 0.0 : 0.01 * (g.next() + 0.5);
            r[i].t = t;
            for (int k = 0; k < 3; k++) { r[i].wm[k] = g.next(); r[i].am[k] = g.next(); }
        }
        const double t0 = g.next() * 0.3, t1 = t0 + 0.2 * (g.next() + 0.5) + 1e-9;
        std::vector<hnet_imu> a(n + 2), b(n + 2);
        int span[2];
        const int ma = feed_ref_select(r.data(), n, t0, t1, a.data());
        const int mb = feed_ref_select_span(r.data(), n, t0, t1, b.data(), span);
        if (ma != mb || (ma > 0 && std::memcmp(a.data(), b.data(), sizeof(hnet_imu) * ma) != 0)) {
            std::printf("span selection differs in case %d\n", c);
            return 4;
        }
        compared += ma > 1;
    }
    std::printf("feed check: accepted %d refused %d, %d non-trivial windows equal\n", accepted, refused, compared);
    return accepted >= 1 && refused >= 3 && compared > 50 ? 0 : 5;
}
#endif
