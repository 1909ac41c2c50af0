// filters_ref.cpp — the host reference of hnet_filters (include/hnet.h) as a small shared library for the tests and tools/filters_bench.py:
// include/hnet_ekf.h's propagate_with_imu / iterated_update behind a C interface on the hnet.h structs, plus the batched host loop of
// INTEGRATION.md §6 on T threads.  Build: g++ -std=c++17 -O2 -shared -fPIC -pthread -I include tests/cpp/filters_ref.cpp -o <lib>.so
#include "hnet.h"
#include "hnet_ekf.h"

#include <algorithm>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

using hnet_ekf::ImuData;
using hnet_ekf::State;

static_assert(sizeof(hnet_filter_state) == sizeof(double) + sizeof(State), "hnet_filter_state = t + hnet_ekf::State");
static_assert(sizeof(hnet_imu) == sizeof(ImuData), "hnet_imu = hnet_ekf::ImuData");

namespace {
State load(const hnet_filter_state& r) { State s; std::memcpy(&s, &r.p[0], sizeof s); return s; }
void save(const State& s, hnet_filter_state& r) { std::memcpy(&r.p[0], &s, sizeof s); }
hnet_ekf::Extrinsics ext(const hnet_filter_params& p) {
    hnet_ekf::Extrinsics e;
    std::memcpy(e.c_R_i, p.c_R_i, sizeof e.c_R_i);
    std::memcpy(e.i_t_i2c, p.i_t_i2c, sizeof e.i_t_i2c);
    return e;
}

// the network surface iterated_update drives: record it of net72 [iters][72], the gate as latest time / image count
struct FakeNet {
    const float* net72;
    int gate;
    double t_frame;
    int img_counter;
    const float* cur = nullptr;
    struct M { const float* v; double operator()(int i, int j) const { return v[i * 8 + j]; } };
    struct V { const float* v; double operator()(int i, int) const { return v[i]; } };
    template <class P> void network_inference(const P&, int it) { cur = net72 + (size_t)it * 72; }
    double get_latest_inference_time() const { return gate ? t_frame : t_frame - 1.0; }
    V get_pred_mean() const { return V{cur}; }
    M get_pred_Cov() const { return M{cur + 8}; }
};
}  // namespace

extern "C" {

int ref_select(const hnet_imu* r, int n, double t0, double t1, hnet_imu* out) {
    return hnet_ekf::select_imu_readings(reinterpret_cast<const ImuData*>(r), n, t0, t1, reinterpret_cast<ImuData*>(out));
}

void ref_interval_inputs(const hnet_filter_state* st, const hnet_imu* a, const hnet_imu* b, int imu_avg, double* w_hat, double* a_hat, double* dt) {
    const State s = load(*st);
    *dt = hnet_ekf::imu_interval_inputs(s, *reinterpret_cast<const ImuData*>(a), *reinterpret_cast<const ImuData*>(b), imu_avg != 0, w_hat, a_hat);
}

// hnet_ekf::propagate_with_imu; the state time becomes t_frame unless refused (-1)
int ref_propagate_with_imu(hnet_filter_state* st, const hnet_filter_params* p, double t_frame, const hnet_imu* r, int n) {
    State s = load(*st);
    double q[hnet_ekf::NW];
    hnet_ekf::noise_q_diag(p->sigma_w, p->sigma_a, p->sigma_wb, p->sigma_ab, q);
    std::vector<ImuData> scratch(n + 2);
    const int k = hnet_ekf::propagate_with_imu(s, ext(*p), st->t, t_frame, reinterpret_cast<const ImuData*>(r), n, q, p->gravity_mag, p->imu_avg != 0,
                                               p->cam_imu_dt, scratch.data());
    if (k < 0) return k;
    save(s, *st);
    st->t = t_frame;
    return k;
}

// ref_propagate_with_imu's loop, interval by interval (the header's select_imu_readings, imu_interval_inputs and propagate in its order), with the
// quaternion after every interval in q_trace [n + 1][4] (may be null) and the largest |w_hat| dt in *max_angle (may be null): what the input
// qualifications of tests/filters_edges.py read.  The state it leaves is ref_propagate_with_imu's, bit for bit (tests/test_filters_edges_cpu.py).
int ref_propagate_trace(hnet_filter_state* st, const hnet_filter_params* p, double t_frame, const hnet_imu* r, int n, double* q_trace, double* max_angle) {
    if (!(t_frame > st->t)) return -1;
    State s = load(*st);
    double q[hnet_ekf::NW];
    hnet_ekf::noise_q_diag(p->sigma_w, p->sigma_a, p->sigma_wb, p->sigma_ab, q);
    std::vector<ImuData> sel(n + 2);
    const int m = hnet_ekf::select_imu_readings(reinterpret_cast<const ImuData*>(r), n, st->t + p->cam_imu_dt, t_frame + p->cam_imu_dt, sel.data());
    int done = 0;
    if (max_angle) *max_angle = 0.0;
    for (int i = 0; i + 1 < m; i++) {
        double w_hat[3], a_hat[3];
        const double dt = hnet_ekf::imu_interval_inputs(s, sel[i], sel[i + 1], p->imu_avg != 0, w_hat, a_hat);
        hnet_ekf::propagate(s, ext(*p), dt, w_hat, a_hat, q, p->gravity_mag);
        if (q_trace) std::memcpy(q_trace + 4 * done, s.q, sizeof s.q);
        if (max_angle) *max_angle = std::max(*max_angle, std::sqrt(hnet_ekf::m3::dot(w_hat, w_hat)) * dt);
        done++;
    }
    save(s, *st);
    st->t = t_frame;
    return done;
}

// the fp32 prior a forward reads: (float)(offset x 159.5)
void ref_prior(const hnet_filter_state* st, float* prior_px) {
    double px[8], cam[8];
    hnet_ekf::prior_pixels(load(*st), px, cam);
    for (int i = 0; i < 8; i++) prior_px[i] = (float)px[i];
}

// hnet_ekf::iterated_update fed with net72 [iters][72]; gate: the network's latest time is the frame's and it has seen > 10 images.
// Returns the updates applied, -1 - applied when a singular S ended the loop early.
int ref_iterated_update(hnet_filter_state* st, const hnet_filter_params* p, int iters, const float* net72, int gate) {
    State s = load(*st);
    FakeNet net{net72, gate, st->t, gate ? 11 : 0};
    double prior[8];
    const int done = hnet_ekf::iterated_update(s, net, iters, p->k_net_cov, prior, st->t);
    save(s, *st);
    return gate && done < iters ? -1 - done : done;
}

// INTEGRATION.md §6 steps 1 and 4 for K sessions on `threads` host threads (session k -> thread k % threads)
static void par(int K, int threads, const std::function<void(int)>& fn);
int ref_propagate_batch(hnet_filter_state* st, const hnet_filter_params* p, int K, const double* t_frame, const hnet_imu* imu, const int64_t* off,
                        int threads) {
    std::vector<int> bad(K, 0);
    par(K, threads, [&](int k) {
        bad[k] = ref_propagate_with_imu(st + k, p + k, t_frame[k], imu + off[k], (int)(off[k + 1] - off[k])) < 0;
    });
    return (int)std::count(bad.begin(), bad.end(), 1);
}

// one IEKF iteration's update of K sessions from hnet_sessions_infer's outputs (mean [K][8], cov [K][64]) with the priors prior_cam [K][8]
void ref_update_batch(hnet_filter_state* st, const hnet_filter_params* p, int K, const float* mean, const float* cov, const double* prior_cam,
                      const int32_t* gate, int update_offset, int threads) {
    par(K, threads, [&](int k) {
        if (!gate[k]) return;
        State s = load(st[k]);
        double m[8], c[64];
        for (int i = 0; i < 8; i++) m[i] = mean[k * 8 + i];
        for (int i = 0; i < 64; i++) c[i] = cov[k * 64 + i];
        if (hnet_ekf::update(s, m, c, prior_cam + k * 8, p[k].k_net_cov, update_offset != 0)) save(s, st[k]);
    });
}

void ref_reset_batch(hnet_filter_state* st, int K) {
    for (int k = 0; k < K; k++) {
        State s = load(st[k]);
        hnet_ekf::reset_4pt_offset(s);
        save(s, st[k]);
    }
}

}  // extern "C"

static void par(int K, int threads, const std::function<void(int)>& fn) {
    if (threads <= 1) {
        for (int k = 0; k < K; k++) fn(k);
        return;
    }
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; t++)
        ts.emplace_back([&, t]() { for (int k = t; k < K; k += threads) fn(k); });
    for (auto& th : ts) th.join();
}
