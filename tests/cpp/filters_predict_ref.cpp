// filters_predict_ref.cpp — the host reference of hnet_filters_predict (include/hnet.h) as a small shared library for the tests and
// tools/filters_bench.py: include/hnet_ekf.h's propagate_mean_with_imu / odometry_from_state / prior_pixels behind a C interface on the hnet.h structs,
// propagate_with_imu next to them (the same host build: the bitwise comparison of tests/test_filters_predict_cpu.py), and the host alternative to the
// device call for K sessions on T threads.  Build: g++ -std=c++17 -O2 -shared -fPIC -pthread -I include tests/cpp/filters_predict_ref.cpp -o <lib>.so
// With -DPREDICT_CHECK_MAIN it is a program that runs the same functions on inputs it makes itself (tests/test_sanitizers_predict_cpu.py: ASan + UBSan).
#include "hnet.h"
#include "hnet_ekf.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

using hnet_ekf::ImuData;
using hnet_ekf::State;

static_assert(sizeof(hnet_filter_state) == sizeof(double) + sizeof(State), "hnet_filter_state = t + hnet_ekf::State");
static_assert(sizeof(hnet_imu) == sizeof(ImuData), "hnet_imu = hnet_ekf::ImuData");
static_assert(sizeof(hnet_odometry) == sizeof(hnet_ekf::Odometry) + 8 * sizeof(double) + 2 * sizeof(int32_t), "hnet_odometry = hnet_ekf::Odometry + prior + 2 ints");

namespace {
State load(const hnet_filter_state& r) { State s; std::memcpy(&s, &r.p[0], sizeof s); return s; }
void save(const State& s, hnet_filter_state& r) { std::memcpy(&r.p[0], &s, sizeof s); }
hnet_ekf::Extrinsics ext(const hnet_filter_params& p) {
    hnet_ekf::Extrinsics e;
    std::memcpy(e.c_R_i, p.c_R_i, sizeof e.c_R_i);
    std::memcpy(e.i_t_i2c, p.i_t_i2c, sizeof e.i_t_i2c);
    return e;
}
const ImuData* rd(const hnet_imu* r) { return reinterpret_cast<const ImuData*>(r); }
}  // namespace

extern "C" {

// hnet_ekf::propagate_mean_with_imu; the state time becomes t_query unless refused (-1)
int pred_ref_mean(hnet_filter_state* st, const hnet_filter_params* p, double t_query, const hnet_imu* r, int n) {
    State s = load(*st);
    std::vector<ImuData> scratch(n + 2);
    const int k = hnet_ekf::propagate_mean_with_imu(s, ext(*p), st->t, t_query, rd(r), n, p->gravity_mag, p->imu_avg != 0, p->cam_imu_dt, scratch.data());
    if (k < 0) return k;
    save(s, *st);
    st->t = t_query;
    return k;
}

// hnet_ekf::propagate_with_imu (mean and covariance) in this build, for the comparison with pred_ref_mean
int pred_ref_full(hnet_filter_state* st, const hnet_filter_params* p, double t_frame, const hnet_imu* r, int n) {
    State s = load(*st);
    double q[hnet_ekf::NW];
    hnet_ekf::noise_q_diag(p->sigma_w, p->sigma_a, p->sigma_wb, p->sigma_ab, q);
    std::vector<ImuData> scratch(n + 2);
    const int k = hnet_ekf::propagate_with_imu(s, ext(*p), st->t, t_frame, rd(r), n, q, p->gravity_mag, p->imu_avg != 0, p->cam_imu_dt, scratch.data());
    if (k < 0) return k;
    save(s, *st);
    st->t = t_frame;
    return k;
}

// hnet_ekf::odometry_from_state + prior_pixels of the state as it is (intervals and status are left alone)
void pred_ref_odometry(const hnet_filter_state* st, double cam_imu_dt, hnet_odometry* out) {
    const State s = load(*st);
    hnet_ekf::Odometry o;
    hnet_ekf::odometry_from_state(s, st->t, cam_imu_dt, o);
    std::memcpy(out, &o, sizeof o);
    double cam[8];
    hnet_ekf::prior_pixels(s, out->prior_px, cam);
}

// what hnet_filters_predict computes for an initialised session whose whole fed history is r[0 .. n) (time order): readings more than 10 s behind the
// newest are not used, t_query <= the state's t describes the state as it is, a newest reading not past the query waits
void pred_ref_predict(const hnet_filter_state* st, const hnet_filter_params* p, double t_query, const hnet_imu* r, int n, hnet_odometry* out) {
    std::memset(out, 0, sizeof *out);
    hnet_filter_state w = *st;
    if (!(t_query > st->t)) {
        pred_ref_odometry(&w, p->cam_imu_dt, out);
        out->status = HNET_PRED_AT_STATE;
        return;
    }
    if (n < 1 || !(t_query < r[n - 1].t - p->cam_imu_dt)) {
        out->status = HNET_PRED_WAIT_IMU;
        return;
    }
    const int k = hnet_ekf::trim_imu_prop(rd(r), n, r[n - 1].t);
    const int done = pred_ref_mean(&w, p, t_query, r + k, n - k);
    pred_ref_odometry(&w, p->cam_imu_dt, out);
    out->intervals = done;
    out->status = HNET_PRED_OK;
}

// the host alternative to one hnet_filters_predict call: K downloaded states, each session's history imu[off[k] .. off[k + 1]), on `threads` threads
void pred_ref_predict_batch(const hnet_filter_state* st, const hnet_filter_params* p, int K, const double* t_query, const hnet_imu* imu, const int64_t* off,
                            int threads, hnet_odometry* out) {
    auto one = [&](int k) { pred_ref_predict(st + k, p + k, t_query[k], imu + off[k], (int)(off[k + 1] - off[k]), out + k); };
    if (threads <= 1) {
        for (int k = 0; k < K; k++) one(k);
        return;
    }
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; t++)
        ts.emplace_back([&, t]() { for (int k = t; k < K; k += threads) one(k); });
    for (auto& th : ts) th.join();
}

}  // extern "C"

#ifdef PREDICT_CHECK_MAIN
namespace {
// a small deterministic generator (no <random>: the values only have to be varied)
struct Lcg {
    unsigned long long s;
    double next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0 - 0.5; }
};
}  // namespace

int main() {
    Lcg g{2024};
    hnet_filter_params p;
    std::memset(&p, 0, sizeof p);
    const double cri[9] = {0, -1, 0, 0, 0, -1, 1, 0, 0};
    std::memcpy(p.c_R_i, cri, sizeof cri);
    p.i_t_i2c[0] = 0.02; p.i_t_i2c[1] = -0.01; p.i_t_i2c[2] = 0.03;
    p.sigma_w = 0.005; p.sigma_a = 0.01; p.sigma_wb = 1e-3; p.sigma_ab = 0.04; p.gravity_mag = 9.81; p.k_net_cov = 10.0;
    int equal = 0, statuses[4] = {0, 0, 0, 0};
    const int counts[6] = {0, 1, 2, 40, -1, -2};                        // intervals; -1: an empty history, -2: one reading
    for (int c = 0; c < 12; c++) {
        const int n_int = counts[c % 6];
        p.imu_avg = c < 6;
        p.cam_imu_dt = c % 2 ? 0.0013 : -0.0148489;
        const int n = n_int == -1 ? 0 : n_int == -2 ? 1 : n_int + 2;
        hnet_filter_state st;
        std::memset(&st, 0, sizeof st);
        st.t = 1.0;
        st.q[0] = 1.0;
        st.p[2] = -1.2;
        for (int i = 0; i < 3; i++) { st.v[i] = g.next(); st.ba[i] = 0.1 * g.next(); st.bg[i] = 0.01 * g.next(); }
        for (int i = 0; i < 12; i++) st.offset[i] = 0.01 * g.next();
        for (int i = 0; i < 27; i++) st.cov[i * 27 + i] = 1e-4;
        std::vector<hnet_imu> r(n);
        for (int i = 0; i < n; i++) {
            r[i].t = st.t + p.cam_imu_dt - 0.0007 + 0.002 * i;
            for (int k = 0; k < 3; k++) { r[i].wm[k] = 0.6 * g.next(); r[i].am[k] = g.next(); }
            r[i].am[2] += 9.81;
        }
        const double tq = st.t + 0.002 * (n_int > 0 ? n_int : 0.1) + 0.0004;
        hnet_filter_state a = st, b = st;
        const int ka = pred_ref_mean(&a, &p, tq, r.data(), n), kb = pred_ref_full(&b, &p, tq, r.data(), n);
        if (ka != kb || std::memcmp(&a, &b, 29 * sizeof(double)) != 0) { std::printf("case %d: mean differs (%d, %d intervals)\n", c, ka, kb); return 2; }
        if (std::memcmp(a.cov, st.cov, sizeof st.cov) != 0) { std::printf("case %d: cov written\n", c); return 3; }
        equal += ka > 0;
        hnet_odometry o;
        pred_ref_predict(&st, &p, tq, r.data(), n, &o);
        statuses[o.status]++;
        if (o.status == HNET_PRED_OK && (o.intervals != ka || std::memcmp(o.p, a.p, 10 * sizeof(double)) != 0)) return 4;
        pred_ref_predict(&st, &p, st.t, r.data(), n, &o);
        if (o.status != HNET_PRED_AT_STATE || o.t_cam != st.t || o.intervals != 0) return 5;
        if (pred_ref_mean(&a, &p, a.t, r.data(), n) != -1) return 6;
    }
    // odometry: Rot2Euler's two branches (pitch at 90 degrees: q = rotation by 90 degrees about x, times a rotation about y)
    hnet_filter_state st;
    std::memset(&st, 0, sizeof st);
    const double h = std::sqrt(0.5), a = 0.3;
    st.q[0] = h * std::cos(a / 2); st.q[1] = h * std::cos(a / 2); st.q[2] = h * std::sin(a / 2); st.q[3] = h * std::sin(a / 2);
    st.p[0] = 0.3; st.p[1] = -0.2; st.p[2] = -1.0;
    hnet_odometry o;
    std::memset(&o, 0, sizeof o);
    pred_ref_odometry(&st, 0.01, &o);
    if (!(std::fabs(std::fabs(o.rpy[1]) - 1.5707963267948966) < 1e-9) || o.rpy[2] != 0.0) { std::printf("pitch %.17g yaw %.17g\n", o.rpy[1], o.rpy[2]); return 7; }
    std::vector<hnet_filter_state> sts(5, st);
    std::vector<hnet_filter_params> ps(5, p);
    std::vector<hnet_odometry> os(5);
    const double tq[5] = {0, 0, 0, 0, 0};
    const int64_t off[6] = {0, 0, 0, 0, 0, 0};
    hnet_imu none;
    std::memset(&none, 0, sizeof none);
    pred_ref_predict_batch(sts.data(), ps.data(), 5, tq, &none, off, 3, os.data());
    for (int k = 0; k < 5; k++)
        if (os[k].status != HNET_PRED_AT_STATE) return 8;
    std::printf("predict check: %d propagated cases equal, statuses ok %d wait %d\n", equal, statuses[HNET_PRED_OK], statuses[HNET_PRED_WAIT_IMU]);
    return equal >= 6 && statuses[HNET_PRED_OK] >= 8 && statuses[HNET_PRED_WAIT_IMU] >= 2 ? 0 : 9;
}
#endif
