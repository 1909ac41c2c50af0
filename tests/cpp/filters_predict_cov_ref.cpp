// filters_predict_cov_ref.cpp — the host reference of hnet_filters_predict_cov (include/hnet.h) as a small shared library for the tests and
// tools/filters_bench.py, after the pattern of filters_predict_ref.cpp: include/hnet_ekf.h's propagate_with_imu / odometry_from_state /
// odometry_cov_from_state / prior_pixels behind a C interface on the hnet.h structs, the host alternative to the device call for K sessions on T threads,
// what the convention test needs (the Jacobian, update()'s perturbation, w_pos and Rot()), and propagate_jacobians as it stood before
// propagate_jacobians_fill was split off, kept verbatim for the byte comparison.
// Build: g++ -std=c++17 -O2 -shared -fPIC -pthread -I include tests/cpp/filters_predict_cov_ref.cpp -o <lib>.so
// With -DPREDICT_COV_CHECK_MAIN it is a program that runs the same functions on inputs it makes itself (tests/test_sanitizers_predict_cov_cpu.py).
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
static_assert(sizeof(hnet_odometry_cov) == sizeof(hnet_ekf::OdometryCov), "hnet_odometry_cov = hnet_ekf::OdometryCov");

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

namespace before {
using namespace hnet_ekf;
/* include/hnet_ekf.h's propagate_jacobians before the split, verbatim apart from its name */
inline void propagate_jacobians_before_split(const State& s, const Extrinsics& e, double dt, const double w_hat[3], double* F, double* Fw,
                                             double gravity_mag) {
    std::memset(F, 0, sizeof(double) * NS * NS);
    std::memset(Fw, 0, sizeof(double) * NS * NW);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double R[9], Rt[9];
    quat_to_rot(s.q, R);
    m3::transpose(R, Rt);
    const double grav[3] = {0.0, 0.0, -gravity_mag}, muw[3] = {0.0, 0.0, -1.0};
    double wc[3], vc[3], muc[3], t3[3], t3b[3];
    mat3_vec(e.c_R_i, w_hat, wc);                                           /* :212 */
    cross(w_hat, e.i_t_i2c, t3);
    for (int i = 0; i < 3; i++) t3[i] += s.v[i];
    mat3_vec(e.c_R_i, t3, vc);                                              /* :213 */
    mat3_vec(Rt, muw, t3);
    mat3_vec(e.c_R_i, t3, muc);                                             /* :214 */
    double ppt[3];
    for (int i = 0; i < 3; i++) ppt[i] = s.p[i] + e.i_t_i2c[i];
    mat3_vec(R, ppt, t3b);
    const double dc = t3b[2];                                               /* :215 */
    const int P_ = 0, Q_ = 3, V_ = 6, BA = 9, BG = 12;
    double Sw[9], Sp[9], Sv[9], B[9];
    m3::skew(w_hat, Sw); m3::skew(s.p, Sp); m3::skew(s.v, Sv);
    for (int i = 0; i < 9; i++) B[i] = I3[i] - dt * Sw[i];
    set_block(F, NS, P_, P_, B);                                            /* :224 */
    set_block(F, NS, P_, V_, I3, dt);
    set_block(F, NS, P_, BG, Sp, -dt);
    {                                                                       /* :228 rotation of the quaternion of (w_hat dt), transposed */
        const double rv[3] = {w_hat[0] * dt, w_hat[1] * dt, w_hat[2] * dt};
        const double n = std::sqrt(m3::dot(rv, rv));
        double qd[4] = {1.0, 0.0, 0.0, 0.0};
        if (n > 1e-300) { qd[0] = std::cos(0.5 * n); for (int i = 0; i < 3; i++) qd[1 + i] = std::sin(0.5 * n) * rv[i] / n; }
        double Rd[9], Rdt[9], Jr[9];
        quat_to_rot(qd, Rd);
        m3::transpose(Rd, Rdt);
        set_block(F, NS, Q_, Q_, Rdt);
        jr_theta(rv, Jr);
        set_block(F, NS, Q_, BG, Jr, -dt);                                   /* :229 */
    }
    mat3_vec(Rt, grav, t3);
    m3::skew(t3, B);
    set_block(F, NS, V_, Q_, B, dt);                                        /* :231 */
    for (int i = 0; i < 9; i++) B[i] = I3[i] - dt * Sw[i];
    set_block(F, NS, V_, V_, B);
    set_block(F, NS, V_, BA, I3, -dt);
    set_block(F, NS, V_, BG, Sv, -dt);
    set_block(F, NS, BA, BA, I3);                                           /* :236-237 */
    set_block(F, NS, BG, BG, I3);
    /* 4-point offsets (:239-319) */
    const double scalar = vc[2] / dc;                                       /* :240-241 */
    double Swc[9];
    m3::skew(wc, Swc);
    double J_dc_p[3] = {R[6], R[7], R[8]};                                  /* ez^T R (:293) */
    double Sppt[9], RS[9], J_dc_q[3];
    m3::skew(ppt, Sppt);
    m3::mul(R, Sppt, RS);
    for (int j = 0; j < 3; j++) J_dc_q[j] = -RS[6 + j];                     /* ez^T (-R skew(p + t)) (:294) */
    double Smu[9], J_muc_q[9];
    mat3_vec(Rt, muw, t3);
    m3::skew(t3, Smu);
    m3::mul(e.c_R_i, Smu, J_muc_q);                                         /* :295 */
    double St[9], J_vc_bw[9];
    m3::skew(e.i_t_i2c, St);
    m3::mul(e.c_R_i, St, J_vc_bw);                                          /* Propagator.h:193 */
    for (int c = 0; c < 4; c++) {
        double pt[3];
        for (int i = 0; i < 3; i++) pt[i] = corner_xy1(c)[i] + s.offset[c][i];        /* :217-220 */
        const double mupt = m3::dot(muc, pt);
        double ezSw[3] = {Swc[6], Swc[7], Swc[8]};                          /* ez^T skew(wc) */
        const double ezSwpt = m3::dot(ezSw, pt);
        double J_df_pt[9], vm[9], pte[9], ptm[9];
        m3::outer(vc, muc, vm);
        m3::outer(pt, ezSw, pte);
        m3::outer(pt, muc, ptm);
        for (int i = 0; i < 9; i++)                                         /* :244-247 */
            J_df_pt[i] = Swc[i] + vm[i] / dc - ezSwpt * I3[i] - pte[i] - scalar * (mupt * I3[i] + ptm[i]);
        double common[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) common[i * 3 + j] = I3[i * 3 + j] - (j == 2 ? pt[i] : 0.0);    /* I - pt ez^T (:248) */
        double cv[3];
        mat3_vec(common, vc, cv);
        double J_df_dc[3];
        for (int i = 0; i < 3; i++) J_df_dc[i] = -mupt * cv[i] / (dc * dc);                           /* :249 */
        double J_df_vc[9], J_df_muc[9], J_df_wc[9], Spt[9];
        for (int i = 0; i < 9; i++) J_df_vc[i] = mupt * common[i] / dc;                                /* :250 */
        m3::outer(cv, pt, J_df_muc);
        for (int i = 0; i < 9; i++) J_df_muc[i] /= dc;                                                 /* :251 */
        m3::skew(pt, Spt);
        m3::mul(common, Spt, J_df_wc);
        for (int i = 0; i < 9; i++) J_df_wc[i] = -J_df_wc[i];                                          /* :252 */
        const int o = 15 + 3 * c;
        double blk[9], t9[9], t9b[9];
        m3::outer(J_df_dc, J_dc_p, blk);
        set_block(F, NS, o, P_, blk, -dt);                                                             /* :298 */
        m3::outer(J_df_dc, J_dc_q, blk);
        m3::mul(J_df_muc, J_muc_q, t9);
        for (int i = 0; i < 9; i++) blk[i] += t9[i];
        set_block(F, NS, o, Q_, blk, -dt);                                                             /* :299 */
        m3::mul(J_df_vc, e.c_R_i, blk);
        set_block(F, NS, o, V_, blk, -dt);                                                             /* :300 */
        m3::mul(J_df_vc, J_vc_bw, t9);
        m3::mul(J_df_wc, e.c_R_i, t9b);                                                                /* J_wc_bw = -c_R_i */
        for (int i = 0; i < 9; i++) blk[i] = t9[i] - t9b[i];
        set_block(F, NS, o, BG, blk, -dt);                                                             /* :301 */
        for (int i = 0; i < 9; i++) blk[i] = I3[i] - dt * J_df_pt[i];
        set_block(F, NS, o, o, blk);                                                                   /* :302 */
    }
    /* noise Jacobian (:322-333) */
    auto copy_block = [&](int r0, int cw, int fr, int fc, double sc) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Fw[(r0 + i) * NW + cw + j] = sc * F[(fr + i) * NS + fc + j];
    };
    copy_block(P_, 0, P_, BG, -1.0);
    copy_block(P_, 12, P_, V_, 1.0);
    copy_block(Q_, 0, Q_, BG, -1.0);
    copy_block(V_, 0, V_, BG, -1.0);
    copy_block(V_, 3, P_, V_, 1.0);
    copy_block(BA, 6, P_, V_, 1.0);
    copy_block(BG, 9, P_, V_, 1.0);
    for (int c = 0; c < 4; c++) copy_block(15 + 3 * c, 0, 15 + 3 * c, BG, -1.0);
}
}  // namespace before
}  // namespace

extern "C" {

// hnet_ekf::odometry_cov_from_state of the state as it is
void pcov_ref_odometry_cov(const hnet_filter_state* st, hnet_odometry_cov* out) {
    const State s = load(*st);
    hnet_ekf::OdometryCov c;
    hnet_ekf::odometry_cov_from_state(s, c);
    std::memcpy(out, &c, sizeof c);
}

// hnet_ekf::odometry_from_state + prior_pixels of the state as it is (intervals and status are left alone)
void pcov_ref_odometry(const hnet_filter_state* st, double cam_imu_dt, hnet_odometry* out) {
    const State s = load(*st);
    hnet_ekf::Odometry o;
    hnet_ekf::odometry_from_state(s, st->t, cam_imu_dt, o);
    std::memcpy(out, &o, sizeof o);
    double cam[8];
    hnet_ekf::prior_pixels(s, out->prior_px, cam);
}

// what hnet_filters_predict_cov computes for an initialised session whose whole fed history is r[0 .. n) (time order), by the rules of
// filters_predict_ref.cpp's pred_ref_predict; full: null or [729]
void pcov_ref_predict(const hnet_filter_state* st, const hnet_filter_params* p, double t_query, const hnet_imu* r, int n, hnet_odometry* out,
                      hnet_odometry_cov* cov, double* full) {
    std::memset(out, 0, sizeof *out);
    std::memset(cov, 0, sizeof *cov);
    if (full) std::memset(full, 0, sizeof(double) * hnet_ekf::NS * hnet_ekf::NS);
    hnet_filter_state w = *st;
    if (t_query > st->t) {
        if (n < 1 || !(t_query < r[n - 1].t - p->cam_imu_dt)) {
            out->status = HNET_PRED_WAIT_IMU;
            return;
        }
        const int k = hnet_ekf::trim_imu_prop(rd(r), n, r[n - 1].t);
        State s = load(w);
        double q[hnet_ekf::NW];
        hnet_ekf::noise_q_diag(p->sigma_w, p->sigma_a, p->sigma_wb, p->sigma_ab, q);
        std::vector<ImuData> scratch(n - k + 2);
        const int done = hnet_ekf::propagate_with_imu(s, ext(*p), st->t, t_query, rd(r) + k, n - k, q, p->gravity_mag, p->imu_avg != 0, p->cam_imu_dt, scratch.data());
        save(s, w);
        w.t = t_query;
        out->intervals = done;
        out->status = HNET_PRED_OK;
        pcov_ref_odometry(&w, p->cam_imu_dt, out);
    } else {
        pcov_ref_odometry(&w, p->cam_imu_dt, out);
        out->status = HNET_PRED_AT_STATE;
    }
    pcov_ref_odometry_cov(&w, cov);
    if (full) std::memcpy(full, w.cov, sizeof w.cov);
}

// the host alternative to one hnet_filters_predict_cov call: K downloaded states, each session's history imu[off[k] .. off[k + 1]), on `threads` threads
void pcov_ref_predict_batch(const hnet_filter_state* st, const hnet_filter_params* p, int K, const double* t_query, const hnet_imu* imu, const int64_t* off,
                            int threads, hnet_odometry* out, hnet_odometry_cov* cov, double* full) {
    auto one = [&](int k) {
        pcov_ref_predict(st + k, p + k, t_query[k], imu + off[k], (int)(off[k + 1] - off[k]), out + k, cov + k, full ? full + (size_t)k * hnet_ekf::NS * hnet_ekf::NS : nullptr);
    };
    if (threads <= 1) {
        for (int k = 0; k < K; k++) one(k);
        return;
    }
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; t++)
        ts.emplace_back([&, t]() { for (int k = t; k < K; k += threads) one(k); });
    for (auto& th : ts) th.join();
}

// ---- the convention test: the header's J, the perturbation update() applies to p and q, and (w_pos, Rot()) of a state
void pcov_ref_jacobian(const hnet_filter_state* st, double J[36]) { hnet_ekf::pose_cov_jacobian(load(*st), J); }
void pcov_ref_perturb(hnet_filter_state* st, const double dx[6]) {
    for (int i = 0; i < 3; i++) st->p[i] += dx[i];
    hnet_ekf::quat_apply_rotvec(dx + 3, st->q);
}
void pcov_ref_wpos_rot(const hnet_filter_state* st, double w_pos[3], double R[9]) {
    hnet_ekf::quat_to_rot(st->q, R);
    hnet_ekf::mat3_vec(R, st->p, w_pos);
}

// ---- the fill split: F [729] and Fw [405] three ways.  `a`: the body before the split; `b`: propagate_jacobians as it is now;
// `c`: buffers zeroed once (by the caller of a whole sequence: here at the first of `reps` calls) + propagate_jacobians_fill, called `reps` times in a row
void pcov_ref_jacobians3(const hnet_filter_state* st, const hnet_filter_params* p, double dt, const double w_hat[3], int reps, double* Fa, double* Fwa,
                         double* Fb, double* Fwb, double* Fc, double* Fwc) {
    const State s = load(*st);
    const hnet_ekf::Extrinsics e = ext(*p);
    before::propagate_jacobians_before_split(s, e, dt, w_hat, Fa, Fwa, p->gravity_mag);
    hnet_ekf::propagate_jacobians(s, e, dt, w_hat, Fb, Fwb, p->gravity_mag);
    for (int r = 0; r < reps; r++) hnet_ekf::propagate_jacobians_fill(s, e, dt, w_hat, Fc, Fwc, p->gravity_mag);
}

}  // extern "C"

#ifdef PREDICT_COV_CHECK_MAIN
namespace {
// a small deterministic generator (no <random>: the values only have to be varied)
struct Lcg {
    unsigned long long s;
    double next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0 - 0.5; }
};
}  // namespace

int main() {
    Lcg g{2025};
    hnet_filter_params p;
    std::memset(&p, 0, sizeof p);
    const double cri[9] = {0, -1, 0, 0, 0, -1, 1, 0, 0};
    std::memcpy(p.c_R_i, cri, sizeof cri);
    p.i_t_i2c[0] = 0.02; p.i_t_i2c[1] = -0.01; p.i_t_i2c[2] = 0.03;
    p.sigma_w = 0.005; p.sigma_a = 0.01; p.sigma_wb = 1e-3; p.sigma_ab = 0.04; p.gravity_mag = 9.81; p.k_net_cov = 10.0;
    int moved = 0, statuses[4] = {0, 0, 0, 0};
    const int counts[6] = {0, 1, 2, 40, -1, -2};                        // intervals; -1: an empty history, -2: one reading
    const int NE = hnet_ekf::NS * hnet_ekf::NS;
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
        hnet_odometry o;
        hnet_odometry_cov oc, oc2;
        std::vector<double> full(NE);
        pcov_ref_predict(&st, &p, tq, r.data(), n, &o, &oc, full.data());
        statuses[o.status]++;
        if (o.status == HNET_PRED_OK) {
            if (o.intervals != (n_int > 0 ? n_int + 1 : 0)) { std::printf("case %d: %d intervals\n", c, o.intervals); return 2; }
            if (o.intervals > 0 && std::memcmp(full.data(), st.cov, sizeof st.cov) == 0) return 3;
            if (o.intervals == 0 && std::memcmp(full.data(), st.cov, sizeof st.cov) != 0) return 4;
            moved += o.intervals > 0;
            for (int i = 0; i < 8; i++)
                if (oc.prior_cov_px[i * 9] != 159.5 * 159.5 * full[hnet_ekf::meas_row(i) * 28]) return 5;
        } else {
            for (int i = 0; i < NE; i++)
                if (full[i] != 0.0) return 6;
            for (int i = 0; i < 36; i++)
                if (oc.pose_cov[i] != 0.0) return 7;
        }
        pcov_ref_predict(&st, &p, st.t, r.data(), n, &o, &oc, nullptr);      // at the state: its covariance as it is
        pcov_ref_odometry_cov(&st, &oc2);
        if (o.status != HNET_PRED_AT_STATE || std::memcmp(&oc, &oc2, sizeof oc) != 0) return 8;
        // the fill split on this state, three calls in a row into buffers zeroed once
        std::vector<double> Fa(NE, 1.0), Fb(NE, 2.0), Fc(NE, 0.0), Wa(27 * 15, 1.0), Wb(27 * 15, 2.0), Wc(27 * 15, 0.0);
        const double w_hat[3] = {0.3 * g.next(), 0.3 * g.next(), c == 3 ? 0.0 : 0.3 * g.next()};
        pcov_ref_jacobians3(&st, &p, c % 3 == 0 ? 1e-9 : 0.002, w_hat, 3, Fa.data(), Wa.data(), Fb.data(), Wb.data(), Fc.data(), Wc.data());
        if (std::memcmp(Fa.data(), Fb.data(), NE * 8) || std::memcmp(Fa.data(), Fc.data(), NE * 8) || std::memcmp(Wa.data(), Wb.data(), 27 * 15 * 8) ||
            std::memcmp(Wa.data(), Wc.data(), 27 * 15 * 8)) return 9;
    }
    std::vector<hnet_filter_state> sts(5);
    std::memset(sts.data(), 0, 5 * sizeof(hnet_filter_state));
    for (auto& s : sts) s.q[0] = 1.0;
    std::vector<hnet_filter_params> ps(5, p);
    std::vector<hnet_odometry> os(5);
    std::vector<hnet_odometry_cov> cs(5);
    std::vector<double> fulls(5 * NE);
    const double tq[5] = {0, 0, 0, 0, 0};
    const int64_t off[6] = {0, 0, 0, 0, 0, 0};
    hnet_imu none;
    std::memset(&none, 0, sizeof none);
    pcov_ref_predict_batch(sts.data(), ps.data(), 5, tq, &none, off, 3, os.data(), cs.data(), fulls.data());
    for (int k = 0; k < 5; k++)
        if (os[k].status != HNET_PRED_AT_STATE) return 10;
    std::printf("predict_cov check: %d propagated cases moved the covariance, statuses ok %d wait %d\n", moved, statuses[HNET_PRED_OK], statuses[HNET_PRED_WAIT_IMU]);
    return moved >= 6 && statuses[HNET_PRED_OK] >= 8 && statuses[HNET_PRED_WAIT_IMU] >= 2 ? 0 : 11;
}
#endif
