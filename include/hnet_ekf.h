/* hnet_ekf.h — the filter step that CONSUMES the HomographyNet output, dependency free.
 *
 * Restates, in plain C++ (double, no Eigen), what cuahn::UpdaterHNet::update does with the network's 8 corner
 * offsets and their 8x8 covariance (reference cuahn/src/update/UpdaterHNet.cpp:28-61, constants UpdaterHNet.h:57-64),
 * the glue around it in VioManager::feed_measurement (cuahn/src/core/VioManager.cpp:227-275: prior = state offsets
 * x 159.5, iterated EKF loop, offsets reset) and State::reset_4pt_offset (cuahn/src/state/State.cpp:101-111).
 * It exists so that the drop-in claim of INTEGRATION.md can be exercised end to end without ROS / Eigen / OpenCV:
 * tests/cpp/iekf_demo.cpp runs adapter -> this update for a few frames on the GPU box, and tests/test_ekf_cpu.py
 * checks every function against the numpy restatement oracle/ekf_oracle.py.
 *
 * State layout (27 error states, State.h:115-123): p 0..2, q 3..5, v 6..8, ba 9..11, bg 12..14, corner offsets
 * ul 15..17, bl 18..20, br 21..23, ur 24..26 (each corner (x, y, z) in normalised camera coordinates; the network
 * measures (x, y)).  Quaternion: Hamilton, (w, x, y, z).
 * Units: the network speaks pixels of the f = 159.5 virtual camera; the filter divides means by 159.5 and
 * covariances by 159.5^2 = 25440.25 (UpdaterHNet.cpp:31-33).
 */
#ifndef HNET_EKF_H
#define HNET_EKF_H

#include <cmath>
#include <cstring>

namespace hnet_ekf {

constexpr int NS = 27;                 /* error-state dimension */
constexpr double F_PIX = 159.5;        /* (320-1)/2 / tan(45 deg), CamBase.h:166-169 */

struct State {
    double p[3];
    double q[4];                       /* Hamilton (w, x, y, z) */
    double v[3];
    double ba[3];
    double bg[3];
    double offset[4][3];               /* ul, bl, br, ur (State.h:110-113 order) */
    double cov[NS * NS];               /* row major */
};

/* VioManager.cpp:230-234 — the prior handed to network_inference: (x, y) of the four corner offsets, x 159.5 */
inline void prior_pixels(const State& s, double prior_px[8], double prior_cam[8]) {
    for (int c = 0; c < 4; c++)
        for (int k = 0; k < 2; k++) {
            prior_cam[2 * c + k] = s.offset[c][k];
            prior_px[2 * c + k] = s.offset[c][k] * F_PIX;
        }
}

/* in-place inverse of an n x n matrix (n <= 8), Gauss-Jordan with partial pivoting; returns false if singular */
inline bool invert(double* a, int n) {
    double inv[64];
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) inv[i * n + j] = i == j ? 1.0 : 0.0;
    for (int col = 0; col < n; col++) {
        int piv = col;
        for (int r = col + 1; r < n; r++)
            if (std::fabs(a[r * n + col]) > std::fabs(a[piv * n + col])) piv = r;
        if (a[piv * n + col] == 0.0) return false;
        if (piv != col)
            for (int j = 0; j < n; j++) {
                double t = a[col * n + j]; a[col * n + j] = a[piv * n + j]; a[piv * n + j] = t;
                t = inv[col * n + j]; inv[col * n + j] = inv[piv * n + j]; inv[piv * n + j] = t;
            }
        const double d = 1.0 / a[col * n + col];
        for (int j = 0; j < n; j++) { a[col * n + j] *= d; inv[col * n + j] *= d; }
        for (int r = 0; r < n; r++) {
            if (r == col) continue;
            const double f = a[r * n + col];
            if (f == 0.0) continue;
            for (int j = 0; j < n; j++) { a[r * n + j] -= f * a[col * n + j]; inv[r * n + j] -= f * inv[col * n + j]; }
        }
    }
    std::memcpy(a, inv, sizeof(double) * n * n);
    return true;
}

/* quat_ops.h:526-538 Ham_quat_update(rot_vec) * q, then quatnorm (quat_ops.h:479-484: sign flip on the LAST component) */
inline void quat_apply_rotvec(const double rv[3], double q[4]) {
    const double ang = std::sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
    const double c = std::cos(0.5 * ang);
    /* the reference divides by the angle without a guard (0/0 for a zero update); the limit is used here */
    const double sc = ang > 0.0 ? std::sin(0.5 * ang) / ang : 0.5;
    const double d[3] = {sc * rv[0], sc * rv[1], sc * rv[2]};
    /* matrix: [[c, -d^T], [d, c I + skew(-d)]] */
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    double r[4];
    r[0] = c * w - d[0] * x - d[1] * y - d[2] * z;
    r[1] = d[0] * w + c * x + d[2] * y - d[1] * z;
    r[2] = d[1] * w - d[2] * x + c * y + d[0] * z;
    r[3] = d[2] * w + d[1] * x - d[0] * y + c * z;
    if (r[3] < 0.0) for (int i = 0; i < 4; i++) r[i] = -r[i];
    const double n = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
    for (int i = 0; i < 4; i++) q[i] = r[i] / n;
}

/* ---- prior generation: the discrete mean propagation that produces the corner offsets the network
 * receives as prior.  Propagator::predict_and_compute prerequisites (cuahn/src/state/Propagator.cpp:211-220) and
 * Propagator::predict_mean_discrete (:342-364).  Body frame forward-left-up; the ground plane normal in the world is
 * (0, 0, -1) (Propagator.h:101).  The covariance propagation (F, Fw Jacobians, :222-330) follows below (propagate_jacobians). */
struct Extrinsics {
    double c_R_i[9];                   /* camera <- IMU rotation, row major (State.h:108) */
    double i_t_i2c[3];                 /* IMU -> camera translation in the IMU frame (State.h:107) */
};

/* the four image corners in normalised camera coordinates (State.h:110-113), order ul, bl, br, ur */
inline const double* corner_xy1(int c) {
    static const double k[4][3] = {{-1.0, -0.69906, 1.0}, {-1.0, 0.69906, 1.0}, {1.0, 0.69906, 1.0}, {1.0, -0.69906, 1.0}};
    return k[c];
}

/* quat_ops.h:549-553 Ham_quat_2_Rot: local -> global rotation of a Hamilton quaternion (w, x, y, z) */
inline void quat_to_rot(const double q[4], double R[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double s = w * w - (x * x + y * y + z * z);
    const double v[3] = {x, y, z};
    const double sk[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[i * 3 + j] = (i == j ? s : 0.0) + 2.0 * v[i] * v[j] + 2.0 * w * sk[i * 3 + j];
}

inline void mat3_vec(const double* M, const double* v, double* o) {
    for (int i = 0; i < 3; i++) o[i] = M[i * 3] * v[0] + M[i * 3 + 1] * v[1] + M[i * 3 + 2] * v[2];
}
inline void cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

inline void propagate_mean(State& s, const Extrinsics& e, double dt, const double w_hat[3], const double a_hat[3], double gravity_mag = 9.81) {
    double R[9], Rt[9];
    quat_to_rot(s.q, R);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rt[i * 3 + j] = R[j * 3 + i];
    /* Propagator.cpp:212-215 */
    double wc[3], vc[3], muc[3], tmp[3], tmp2[3];
    mat3_vec(e.c_R_i, w_hat, wc);
    cross(w_hat, e.i_t_i2c, tmp);
    for (int i = 0; i < 3; i++) tmp[i] += s.v[i];
    mat3_vec(e.c_R_i, tmp, vc);
    const double muw[3] = {0.0, 0.0, -1.0};
    mat3_vec(Rt, muw, tmp);
    mat3_vec(e.c_R_i, tmp, muc);
    for (int i = 0; i < 3; i++) tmp[i] = s.p[i] + e.i_t_i2c[i];
    mat3_vec(R, tmp, tmp2);
    const double dc = tmp2[2];
    /* corner dynamics use the state BEFORE the IMU part is advanced (:217-220, :357-362) */
    double Hm[9];
    const double skw[9] = {0, -wc[2], wc[1], wc[2], 0, -wc[0], -wc[1], wc[0], 0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Hm[i * 3 + j] = skw[i * 3 + j] + vc[i] * muc[j] / dc;
    double new_off[4][3];
    for (int c = 0; c < 4; c++) {
        double pt[3], Hp[3];
        for (int i = 0; i < 3; i++) pt[i] = corner_xy1(c)[i] + s.offset[c][i];
        mat3_vec(Hm, pt, Hp);
        /* -(I - pt ez^T) H pt = -(Hp - pt * Hp_z) */
        for (int i = 0; i < 3; i++) new_off[c][i] = s.offset[c][i] + dt * (-(Hp[i] - pt[i] * Hp[2]));
    }
    /* :347-354 (the position / velocity are expressed in the body frame in this filter) */
    double wdt[3] = {w_hat[0] * dt, w_hat[1] * dt, w_hat[2] * dt};
    double nq[4] = {s.q[0], s.q[1], s.q[2], s.q[3]};
    quat_apply_rotvec(wdt, nq);
    double wxv[3], wxp[3], g[3];
    cross(w_hat, s.v, wxv);
    cross(w_hat, s.p, wxp);
    const double grav[3] = {0.0, 0.0, -gravity_mag};
    mat3_vec(Rt, grav, g);
    double nv[3], np[3];
    for (int i = 0; i < 3; i++) {
        nv[i] = s.v[i] + dt * (-wxv[i] + a_hat[i] + g[i]);
        np[i] = s.p[i] + dt * (-wxp[i] + s.v[i]);
    }
    for (int i = 0; i < 3; i++) { s.p[i] = np[i]; s.v[i] = nv[i]; }
    for (int i = 0; i < 4; i++) s.q[i] = nq[i];
    std::memcpy(s.offset, new_off, sizeof new_off);
}

/* ---- covariance propagation: Propagator::predict_and_compute's Jacobians (Propagator.cpp:222-333),
 * the noise matrix of the Propagator constructor (Propagator.h:86-96) and StateHelper::propagate_Cov (StateHelper.cpp:28-32).
 * Error-state order p q v ba bg ul bl br ur (3 each); the attitude error is a rotation vector applied on the right
 * (q <- q (x) dq, what Ham_quat_update(dtheta) * q computes); noise order (gyro, accel, accel walk, gyro walk, 4pt) x 3.
 * tests/test_ekf_cpu.py checks every block of F against central differences of propagate_mean() (independent of the formulas)
 * and the whole thing against the numpy restatement. */
constexpr int NW = 15;                 /* noise dimension */

namespace m3 {
inline void skew(const double* w, double* S) { S[0] = 0; S[1] = -w[2]; S[2] = w[1]; S[3] = w[2]; S[4] = 0; S[5] = -w[0]; S[6] = -w[1]; S[7] = w[0]; S[8] = 0; }
inline void mul(const double* A, const double* B, double* C) {      /* C = A B (3x3) */
    double t[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) t[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
    std::memcpy(C, t, sizeof t);
}
inline void transpose(const double* A, double* T) {
    double t[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) t[i * 3 + j] = A[j * 3 + i];
    std::memcpy(T, t, sizeof t);
}
inline void outer(const double* a, const double* b, double* C) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = a[i] * b[j];
}
inline double dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
}  // namespace m3

/* quat_ops.h:573-580 (the reference divides by |theta| without a guard; the limit I is used at 0) */
inline void jr_theta(const double th[3], double J[9]) {
    const double n = std::sqrt(m3::dot(th, th));
    for (int i = 0; i < 9; i++) J[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (n < 1e-12) return;
    double S[9], SS[9];
    m3::skew(th, S);
    m3::mul(S, S, SS);
    const double a = (1.0 - std::cos(n)) / (n * n), b = (n - std::sin(n)) / (n * n * n);
    for (int i = 0; i < 9; i++) J[i] += -a * S[i] + b * SS[i];
}

inline void set_block(double* M, int ld, int r0, int c0, const double* B, double scale = 1.0) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[(r0 + i) * ld + c0 + j] = scale * B[i * 3 + j];
}

/* The body of propagate_jacobians below: every entry of F [27 x 27] and Fw [27 x 15] (row major) that can be non-zero is WRITTEN, none is read before
 * it is written and no other entry is touched; which entries those are does not depend on the arguments.  A caller that zeroed both once may therefore
 * call this for one interval after another (filter_predict_cov_kernel zeroes them once with all lanes); tests/test_filters_predict_cov_cpu.py compares
 * zeroed buffers + this with the body as it stood before the split, byte for byte. */
inline void propagate_jacobians_fill(const State& s, const Extrinsics& e, double dt, const double w_hat[3], double* F, double* Fw,
                                     double gravity_mag = 9.81) {
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

/* F [27 x 27], Fw [27 x 15], row major, evaluated at `s` BEFORE the mean is advanced (Propagator.cpp:211-220, :222-333) */
inline void propagate_jacobians(const State& s, const Extrinsics& e, double dt, const double w_hat[3], double* F, double* Fw,
                                double gravity_mag = 9.81) {
    std::memset(F, 0, sizeof(double) * NS * NS);
    std::memset(Fw, 0, sizeof(double) * NS * NW);
    propagate_jacobians_fill(s, e, dt, w_hat, F, Fw, gravity_mag);
}

/* Propagator.h:86-96: diagonal of Q, order gyro, accel, accel random walk, gyro random walk, 4pt */
inline void noise_q_diag(double sigma_w, double sigma_a, double sigma_wb, double sigma_ab, double q[NW]) {
    const double v[5] = {sigma_w * sigma_w, sigma_a * sigma_a, sigma_ab * sigma_ab, sigma_wb * sigma_wb, 1.0e-4};
    for (int i = 0; i < NW; i++) q[i] = v[i / 3];
}

/* StateHelper::propagate_Cov (StateHelper.cpp:28-32): P <- F P F^T + Fw diag(q) Fw^T */
inline void propagate_cov(double* P, const double* F, const double* Fw, const double q[NW]) {
    static thread_local double T[NS * NS], O[NS * NS];
    for (int i = 0; i < NS; i++)
        for (int j = 0; j < NS; j++) {
            double a = 0.0;
            for (int k = 0; k < NS; k++) a += F[i * NS + k] * P[k * NS + j];
            T[i * NS + j] = a;
        }
    for (int i = 0; i < NS; i++)
        for (int j = 0; j < NS; j++) {
            double a = 0.0;
            for (int k = 0; k < NS; k++) a += T[i * NS + k] * F[j * NS + k];
            for (int k = 0; k < NW; k++) a += Fw[i * NW + k] * q[k] * Fw[j * NW + k];
            O[i * NS + j] = a;
        }
    std::memcpy(P, O, sizeof(double) * NS * NS);
}

/* one IMU interval of Propagator::propagate_with_imu's loop (:63-67): Jacobians at the old state, mean, covariance */
inline void propagate(State& s, const Extrinsics& e, double dt, const double w_hat[3], const double a_hat[3], const double q[NW],
                      double gravity_mag = 9.81) {
    static thread_local double F[NS * NS], Fw[NS * NW];
    propagate_jacobians(s, e, dt, w_hat, F, Fw, gravity_mag);
    propagate_mean(s, e, dt, w_hat, a_hat, gravity_mag);
    propagate_cov(s.cov, F, Fw, q);
}

/* UpdaterHNet::update (UpdaterHNet.cpp:28-61).  net_mean_px[8], net_cov_px[64]: what get_pred_mean()/get_pred_Cov()
 * return; propagated[8]: the prior in camera units (prior_pixels() / 159.5); k_net_cov: UpdaterOptions.h:33 (10.0).
 * Returns false if the innovation covariance is singular (the reference would produce inf/nan). */
inline bool update(State& s, const double net_mean_px[8], const double net_cov_px[64], const double propagated[8], double k_net_cov,
                   bool update_offset) {
    /* H selects (x, y) of each corner: rows 2c+k <- state 15 + 3c + k;  Hn = I8 */
    int sel[8];
    for (int c = 0; c < 4; c++) { sel[2 * c] = 15 + 3 * c; sel[2 * c + 1] = 16 + 3 * c; }
    double S[64], PHt[NS * 8];
    for (int i = 0; i < NS; i++)
        for (int j = 0; j < 8; j++) PHt[i * 8 + j] = s.cov[i * NS + sel[j]];
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) S[i * 8 + j] = s.cov[sel[i] * NS + sel[j]] + k_net_cov * net_cov_px[i * 8 + j] / (F_PIX * F_PIX);
    if (!invert(S, 8)) return false;
    double K[NS * 8];
    for (int i = 0; i < NS; i++)
        for (int j = 0; j < 8; j++) {
            double a = 0.0;
            for (int k = 0; k < 8; k++) a += PHt[i * 8 + k] * S[k * 8 + j];
            K[i * 8 + j] = a;
        }
    double inno[8];
    for (int i = 0; i < 8; i++) inno[i] = net_mean_px[i] / F_PIX - propagated[i];
    /* Cov <- (I - K H) Cov  (not the Joseph form, as the reference) */
    double KH_P[NS * NS];
    for (int i = 0; i < NS; i++)
        for (int j = 0; j < NS; j++) {
            double a = 0.0;
            for (int k = 0; k < 8; k++) a += K[i * 8 + k] * s.cov[sel[k] * NS + j];
            KH_P[i * NS + j] = a;
        }
    for (int i = 0; i < NS * NS; i++) s.cov[i] -= KH_P[i];
    double dx[NS];
    const int rows = update_offset ? NS : 15;          /* last IEKF iteration: the offsets are about to be reset anyway */
    for (int i = 0; i < NS; i++) dx[i] = 0.0;
    for (int i = 0; i < rows; i++)
        for (int k = 0; k < 8; k++) dx[i] += K[i * 8 + k] * inno[k];
    for (int i = 0; i < 3; i++) s.p[i] += dx[i];
    quat_apply_rotvec(dx + 3, s.q);
    for (int i = 0; i < 3; i++) { s.v[i] += dx[6 + i]; s.ba[i] += dx[9 + i]; s.bg[i] += dx[12 + i]; }
    if (update_offset)
        for (int c = 0; c < 4; c++)
            for (int k = 0; k < 3; k++) s.offset[c][k] += dx[15 + 3 * c + k];
    return true;
}

/* State::reset_4pt_offset (State.cpp:101-111): offsets to zero, covariance keeps only the IMU 15 x 15 block */
inline void reset_4pt_offset(State& s) {
    std::memset(s.offset, 0, sizeof s.offset);
    for (int i = 0; i < NS; i++)
        for (int j = 0; j < NS; j++)
            if (i >= 15 || j >= 15) s.cov[i * NS + j] = 0.0;
}

/* The iterated update of VioManager.cpp:227-275 around any object with the reference's HomographyNet surface
 * (network_inference / get_pred_mean / get_pred_Cov returning something indexable as (i) resp. (i, j),
 * get_latest_inference_time(), public img_counter).  As in the reference the network runs in EVERY iteration, but the filter is
 * only updated when the network's latest image is the frame being processed and more than 10 images have been seen
 * (VioManager.cpp:257: `HNet->get_latest_inference_time() == time_stamp && HNet->img_counter > 10`); the offsets are reset
 * afterwards either way (:275).  Returns the number of updates applied. */
template <class Net, class Vec8>
inline int iterated_update(State& s, Net& net, int max_iekf_iteration, double k_net_cov, Vec8& prior_px_vec, double time_stamp) {
    int done = 0;
    for (int it = 0; it < max_iekf_iteration; it++) {
        double prior_px[8], prior_cam[8];
        prior_pixels(s, prior_px, prior_cam);
        for (int i = 0; i < 8; i++) prior_px_vec[i] = prior_px[i];
        net.network_inference(prior_px_vec, it);
        if (net.get_latest_inference_time() == time_stamp && net.img_counter > 10) {
            const auto m = net.get_pred_mean();
            const auto C = net.get_pred_Cov();
            double mean[8], cov[64];
            for (int i = 0; i < 8; i++) {
                mean[i] = m(i, 0);
                for (int j = 0; j < 8; j++) cov[i * 8 + j] = C(i, j);
            }
            if (!update(s, mean, cov, prior_cam, k_net_cov, it != max_iekf_iteration - 1)) break;
            done++;
        }
    }
    reset_4pt_offset(s);
    return done;
}

/* ---- innovation records, the normalised innovation squared and an opt-in gate on it.  The reference dropped OpenVINS' chi-squared test when
 * UpdaterHNet replaced the feature updaters (UpdaterHNet.cpp:28-61 applies every measurement); these are additions next to update() and
 * iterated_update(), which stay as they are.  NIS = r^T S^-1 r with r and S as update() forms them; for a consistent filter it is chi-squared
 * with 8 degrees of freedom (mean 8; quantiles 15.507 at 95 %, 20.090 at 99 %, 26.124 at 99.9 %).  The device filters (hnet_filters_enable_innovations,
 * include/hnet.h) restate innovation() in filter_innovation_kernel; tests/test_filters_innov_cpu.py checks it against numpy. */
enum { INNOV_NONE = 0,                 /* the reference's gate (VioManager.cpp:257) was closed: nothing measured */
       INNOV_USED = 1,                 /* the update was applied */
       INNOV_REJECTED = 2,             /* the NIS exceeded max_nis: this update and the step's later ones are skipped */
       INNOV_SINGULAR = 3,             /* S was singular: update() refuses it */
       INNOV_SKIPPED = 4 };            /* after an earlier rejection or singular S in the same step, or a photometric rejection at this or an earlier iteration */
/* r: the innovation mean / 159.5 - prior; s_diag: the diagonal of S = H P H^T + k_net_cov C / 159.5^2; nis: NaN when S is singular.
 * A NONE or SKIPPED record holds zeros in r, s_diag and nis: nothing was formed for it. */
struct Innovation {
    double r[8], s_diag[8], nis;
    int flag;
};

/* r, the diagonal of S and the NIS of the measurement update() would apply to `s`: the same expressions for S and the innovation, the same
 * invert(), then nis = sum_i r_i (sum_j Sinv_ij r_j) in that order.  Returns false on a singular S (nis = NaN, flag SINGULAR), else flag USED;
 * `s` is not written. */
inline bool innovation(const State& s, const double net_mean_px[8], const double net_cov_px[64], const double propagated[8], double k_net_cov,
                       Innovation& o) {
    int sel[8];
    for (int c = 0; c < 4; c++) { sel[2 * c] = 15 + 3 * c; sel[2 * c + 1] = 16 + 3 * c; }
    double S[64];
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) S[i * 8 + j] = s.cov[sel[i] * NS + sel[j]] + k_net_cov * net_cov_px[i * 8 + j] / (F_PIX * F_PIX);
    for (int i = 0; i < 8; i++) {
        o.s_diag[i] = S[i * 8 + i];
        o.r[i] = net_mean_px[i] / F_PIX - propagated[i];
    }
    if (!invert(S, 8)) {
        o.nis = (double)NAN;
        o.flag = INNOV_SINGULAR;
        return false;
    }
    double nis = 0.0;
    for (int i = 0; i < 8; i++) {
        double a = 0.0;
        for (int j = 0; j < 8; j++) a += S[i * 8 + j] * o.r[j];
        nis += o.r[i] * a;
    }
    o.nis = nis;
    o.flag = INNOV_USED;
    return true;
}

/* iterated_update with one Innovation per iteration in rec[max_iekf_iteration] and a gate on the NIS.  max_nis <= 0: no gate, and state,
 * return value and the calls made to `net` are iterated_update's, bit for bit.  With a gate: at an iteration whose reference gate is open and whose
 * NIS exceeds max_nis, that update and every later update of the call are skipped (REJECTED, then SKIPPED); updates already applied stay, the
 * network still runs in every iteration and the offsets are reset as always.  A NaN NIS does not reject (update()'s singular path handles a
 * singular S: SINGULAR, the loop ends as iterated_update's does and the iterations it never ran are SKIPPED). */
template <class Net, class Vec8>
inline int iterated_update_gated(State& s, Net& net, int max_iekf_iteration, double k_net_cov, Vec8& prior_px_vec, double time_stamp, double max_nis,
                                 Innovation* rec) {
    int done = 0;
    bool skip = false;
    for (int it = 0; it < max_iekf_iteration; it++) {
        std::memset(&rec[it], 0, sizeof rec[it]);
        rec[it].flag = INNOV_NONE;
    }
    for (int it = 0; it < max_iekf_iteration; it++) {
        double prior_px[8], prior_cam[8];
        prior_pixels(s, prior_px, prior_cam);
        for (int i = 0; i < 8; i++) prior_px_vec[i] = prior_px[i];
        net.network_inference(prior_px_vec, it);
        if (net.get_latest_inference_time() == time_stamp && net.img_counter > 10) {
            if (skip) { rec[it].flag = INNOV_SKIPPED; continue; }
            const auto m = net.get_pred_mean();
            const auto C = net.get_pred_Cov();
            double mean[8], cov[64];
            for (int i = 0; i < 8; i++) {
                mean[i] = m(i, 0);
                for (int j = 0; j < 8; j++) cov[i * 8 + j] = C(i, j);
            }
            innovation(s, mean, cov, prior_cam, k_net_cov, rec[it]);
            if (max_nis > 0.0 && rec[it].nis > max_nis) {
                rec[it].flag = INNOV_REJECTED;
                skip = true;
                continue;
            }
            if (!update(s, mean, cov, prior_cam, k_net_cov, it != max_iekf_iteration - 1)) {
                for (int k = it + 1; k < max_iekf_iteration; k++) rec[k].flag = INNOV_SKIPPED;
                break;
            }
            done++;
        }
    }
    reset_4pt_offset(s);
    return done;
}

/* ---- an opt-in photometric gate: refuse an update whose estimate explains the frame pair worse than the IMU prior did.  A record is the reference's
 * error map |warp(img2, H) - img1| * 255 (model_to_trace.py:319-327) summed for H = (float) dlt_solve(p4 + offsets): `sum` over all pixels,
 * `sum_inside` / `n_inside` over the pixels that sample inside img2 (include/hnet.h hnet_photo_residual; the device forms them in csrc/kernels_photo.hip).
 * The reference has no such test (UpdaterHNet.cpp:28-61 applies every measurement); like the NIS gate these are additions. */
enum { PHOTO_DEGENERATE = 1,           /* H has a non-finite entry: every sample is 0, n_inside = 0 */
       PHOTO_REJECTED = 2 };           /* photo_reject refused this estimate: its update and the call's later ones are skipped */
struct PhotoRecord {
    double sum, sum_inside;
    int n_inside, flags;
};

/* The rule.  max_ratio <= 0 (or NaN): never.  An estimate that is DEGENERATE or has fewer than max(min_inside, 1) pixels inside is refused; otherwise a
 * prior that is DEGENERATE or has fewer than that inside gives nothing to compare with: accepted.  Otherwise refused iff the estimate's mean residual
 * inside exceeds max_ratio times the prior's, compared on products, est.sum_inside * prior.n_inside > (max_ratio * prior.sum_inside) * est.n_inside:
 * no quotient and no addition, so host and device round it identically whatever the contraction setting.  A NaN on either side does not refuse (as a
 * NaN NIS does not). */
inline bool photo_reject(const PhotoRecord& prior, const PhotoRecord& est, double max_ratio, int min_inside) {
    if (!(max_ratio > 0.0)) return false;
    const int need = min_inside > 1 ? min_inside : 1;
    if ((est.flags & PHOTO_DEGENERATE) || est.n_inside < need) return true;
    if ((prior.flags & PHOTO_DEGENERATE) || prior.n_inside < need) return false;
    const double lhs = est.sum_inside * (double)prior.n_inside;
    const double rhs = (max_ratio * prior.sum_inside) * (double)est.n_inside;
    return lhs > rhs;
}

/* iterated_update_gated with the photometric gate in front of the NIS gate.  photo(off_px): the PhotoRecord of 8 corner offsets in pixels (the fp32
 * values the device works on, widened) on the current frame pair.  prec[1 + max_iekf_iteration]: prec[0] the record of iteration 0's fp32 prior,
 * prec[1 + it] the record of forward it's mean where it was judged; records never formed are zeros.  max_ratio <= 0: `photo` is never called, prec is
 * zeros, and state, return value, rec and the calls made to `net` are iterated_update_gated's, bit for bit.  With a gate: at every iteration whose
 * reference gate is open and that no earlier singular S, NIS rejection or photometric rejection of the call precedes, the estimate's record is formed
 * and photo_reject applied against prec[0]; on rejection the record takes PHOTO_REJECTED, this update and every later one of the call are skipped
 * (rec[it] and the later open iterations SKIPPED), updates already applied stay, the network still runs in every iteration and the offsets are reset
 * as always.  Only an estimate that passes goes on to the NIS record, the NIS gate and the update. */
template <class Net, class Vec8, class Photo>
inline int iterated_update_photo_gated(State& s, Net& net, int max_iekf_iteration, double k_net_cov, Vec8& prior_px_vec, double time_stamp, double max_nis,
                                       Innovation* rec, Photo& photo, double max_ratio, int min_inside, PhotoRecord* prec) {
    int done = 0;
    bool skip = false;
    const bool gated = max_ratio > 0.0;
    for (int it = 0; it < max_iekf_iteration; it++) {
        std::memset(&rec[it], 0, sizeof rec[it]);
        rec[it].flag = INNOV_NONE;
    }
    std::memset(prec, 0, sizeof(PhotoRecord) * (size_t)(1 + max_iekf_iteration));
    for (int it = 0; it < max_iekf_iteration; it++) {
        double prior_px[8], prior_cam[8];
        prior_pixels(s, prior_px, prior_cam);
        for (int i = 0; i < 8; i++) prior_px_vec[i] = prior_px[i];
        if (gated && it == 0) {
            double p32[8];
            for (int i = 0; i < 8; i++) p32[i] = (double)(float)prior_px[i];
            prec[0] = photo(p32);
        }
        net.network_inference(prior_px_vec, it);
        if (net.get_latest_inference_time() == time_stamp && net.img_counter > 10) {
            if (skip) { rec[it].flag = INNOV_SKIPPED; continue; }
            const auto m = net.get_pred_mean();
            const auto C = net.get_pred_Cov();
            double mean[8], cov[64];
            for (int i = 0; i < 8; i++) {
                mean[i] = m(i, 0);
                for (int j = 0; j < 8; j++) cov[i * 8 + j] = C(i, j);
            }
            if (gated) {
                prec[1 + it] = photo(mean);
                if (photo_reject(prec[0], prec[1 + it], max_ratio, min_inside)) {
                    prec[1 + it].flags |= PHOTO_REJECTED;
                    rec[it].flag = INNOV_SKIPPED;
                    skip = true;
                    continue;
                }
            }
            innovation(s, mean, cov, prior_cam, k_net_cov, rec[it]);
            if (max_nis > 0.0 && rec[it].nis > max_nis) {
                rec[it].flag = INNOV_REJECTED;
                skip = true;
                continue;
            }
            if (!update(s, mean, cov, prior_cam, k_net_cov, it != max_iekf_iteration - 1)) {
                for (int k = it + 1; k < max_iekf_iteration; k++) rec[k].flag = INNOV_SKIPPED;
                break;
            }
            done++;
        }
    }
    reset_4pt_offset(s);
    return done;
}

/* ---- IMU propagation over one camera interval: what Propagator::propagate_with_imu (Propagator.cpp:28-76) does with the
 * buffered IMU readings.  The device filters (hnet_filters, include/hnet.h) select the readings with these functions on the host and run the
 * intervals on the device; tests/test_filters_cpu.py checks them against a numpy restatement. */
struct ImuData {
    double t;                          /* time stamp (IMU clock) */
    double wm[3];                      /* measured angular velocity */
    double am[3];                      /* measured specific force */
};

/* Propagator.h:179-190: linear interpolation of two readings at time t */
inline ImuData interpolate_data(const ImuData& a, const ImuData& b, double t) {
    const double lambda = (t - a.t) / (b.t - a.t);
    ImuData d;
    d.t = t;
    for (int i = 0; i < 3; i++) {
        d.am[i] = (1 - lambda) * a.am[i] + lambda * b.am[i];
        d.wm[i] = (1 - lambda) * a.wm[i] + lambda * b.wm[i];
    }
    return d;
}

/* Propagator::select_imu_readings (Propagator.cpp:81-175): the readings that cover [t0, t1] out of readings[0 .. n), split at both ends,
 * zero-dt readings (< 1e-12) removed.  `out` has room for n + 2 entries; returns how many were written (fewer than two: nothing to
 * integrate, as the reference's warning cases). */
inline int select_imu_readings(const ImuData* readings, int n, double t0, double t1, ImuData* out) {
    int m = 0;
    if (n <= 0) return 0;
    for (int i = 0; i < n - 1; i++) {
        if (readings[i + 1].t > t0 && readings[i].t < t0) {                          /* start of the period: split */
            out[m++] = interpolate_data(readings[i], readings[i + 1], t0);
            continue;
        }
        if (readings[i].t >= t0 && readings[i + 1].t <= t1) {                        /* middle: the whole reading */
            out[m++] = readings[i];
            continue;
        }
        if (readings[i + 1].t > t1) {                                                /* end of the period */
            if (readings[i].t > t1 && i == 0) break;                                 /* IMU slower than the camera, nothing before t0 */
            else if (readings[i].t > t1) out[m++] = interpolate_data(readings[i - 1], readings[i], t1);
            else out[m++] = readings[i];
            if (out[m - 1].t != t1) out[m++] = interpolate_data(readings[i], readings[i + 1], t1);
            break;
        }
    }
    if (m == 0) return 0;
    for (int i = 0; i < m - 1; i++)                                                  /* zero dt: drop the earlier reading */
        if (std::fabs(out[i + 1].t - out[i].t) < 1e-12) {
            for (int j = i; j < m - 1; j++) out[j] = out[j + 1];
            m--;
            i--;
        }
    return m;
}

/* Propagator::predict_and_compute (Propagator.cpp:186-204): the corrected inputs of the interval a -> b with the state's current biases,
 * the average of both ends with imu_avg (StateOptions.h:39, true by default), the later reading otherwise; returns dt */
inline double imu_interval_inputs(const State& s, const ImuData& a, const ImuData& b, bool imu_avg, double w_hat[3], double a_hat[3]) {
    for (int i = 0; i < 3; i++) {
        const double w1 = a.wm[i] - s.bg[i], a1 = a.am[i] - s.ba[i];
        const double w2 = b.wm[i] - s.bg[i], a2 = b.am[i] - s.ba[i];
        w_hat[i] = imu_avg ? .5 * (w1 + w2) : w2;
        a_hat[i] = imu_avg ? .5 * (a1 + a2) : a2;
    }
    return b.t - a.t;
}

/* Propagator::propagate_with_imu (Propagator.cpp:28-76) with a fixed camera-IMU time offset cam_imu_dt (t_imu = t_cam + cam_imu_dt;
 * calib_cam_timeoffset is false in uzhfpv.launch:42).  t_state / t_frame: camera clock.  Refuses t_frame <= t_state (the reference exits,
 * :32-43) and returns -1; otherwise runs one propagate() per selected interval and returns their number.  With fewer than two selected
 * readings no interval runs, and the state time still becomes t_frame (:75): the caller records it.  `scratch` has room for n + 2 readings. */
inline int propagate_with_imu(State& s, const Extrinsics& e, double t_state, double t_frame, const ImuData* readings, int n,
                              const double q[NW], double gravity_mag, bool imu_avg, double cam_imu_dt, ImuData* scratch) {
    if (!(t_frame > t_state)) return -1;
    const int m = select_imu_readings(readings, n, t_state + cam_imu_dt, t_frame + cam_imu_dt, scratch);
    int done = 0;
    for (int i = 0; i + 1 < m; i++) {
        double w_hat[3], a_hat[3];
        const double dt = imu_interval_inputs(s, scratch[i], scratch[i + 1], imu_avg, w_hat, a_hat);
        propagate(s, e, dt, w_hat, a_hat, q, gravity_mag);
        done++;
    }
    return done;
}

/* ---- prediction between frames: the mean at a query time past the state's, and what the reference's publishers form from it.
 * OpenVINS' fast_state_propagate, which carried the state on to the newest inertial reading for the odometry message, is still in the reference,
 * commented out (Propagator.h:151); its node publishes visualize_odometry from the IMU callback "for onboard feedback control"
 * (ros_subscribe_cuahn.cpp:134).  hnet_filters_predict (include/hnet.h) runs these on the device's IMU rings; tests/test_filters_predict_cpu.py. */

/* The loop of propagate_with_imu without propagate_jacobians and propagate_cov: the same select_imu_readings, imu_interval_inputs and propagate_mean
 * in the same order, so p, q, v, ba, bg and the offsets come out as propagate_with_imu leaves them; s.cov is neither read nor written.  t_state /
 * t_query: camera clock.  Returns the number of intervals, or -1 for t_query <= t_state (nothing written).  `scratch` has room for n + 2 readings. */
inline int propagate_mean_with_imu(State& s, const Extrinsics& e, double t_state, double t_query, const ImuData* readings, int n,
                                   double gravity_mag, bool imu_avg, double cam_imu_dt, ImuData* scratch) {
    if (!(t_query > t_state)) return -1;
    const int m = select_imu_readings(readings, n, t_state + cam_imu_dt, t_query + cam_imu_dt, scratch);
    int done = 0;
    for (int i = 0; i + 1 < m; i++) {
        double w_hat[3], a_hat[3];
        const double dt = imu_interval_inputs(s, scratch[i], scratch[i + 1], imu_avg, w_hat, a_hat);
        propagate_mean(s, e, dt, w_hat, a_hat, gravity_mag);
        done++;
    }
    return done;
}

/* What RosVisualizer::publish_state (RosVisualizer.cpp:157-174) and RosVisualizer::visualize_odometry (:113-144) form from a state: 24 packed doubles,
 * the head of hnet_odometry (include/hnet.h). */
struct Odometry {
    double t_cam, t_imu;               /* the state's time; + cam_imu_dt, the stamp of both messages (:157-158, :113-114) */
    double p[3], q[4], v[3];           /* the mean as it is (State layout); q is published as it is (:165-168) */
    double w_pos[3];                   /* Rot() * pos (:171, :132) */
    double rpy[3];                     /* roll, pitch, yaw of b_R_w (:123-128) */
    double body_pos[3], body_vel[3];   /* front-right-down: (-w_pos[1], -w_pos[0], -w_pos[2]) (:134-136), (-v[1], -v[0], -v[2]) (:141-144) */
};

/* RosVisualizer::Rot2Euler (RosVisualizer.cpp:303-315) of a row-major 3 x 3 matrix, the sy < 1e-6 branch (pitch near 90 degrees) included */
inline void rot_to_euler(const double R[9], double& roll, double& pitch, double& yaw) {
    const double sy = std::sqrt(R[1 * 3 + 2] * R[1 * 3 + 2] + R[2 * 3 + 2] * R[2 * 3 + 2]);
    if (sy < 1e-6) {
        yaw = 0.0;
        roll = std::atan2(-R[2 * 3 + 1], R[1 * 3 + 1]);
    } else {
        yaw = std::atan2(R[0 * 3 + 1], R[0 * 3 + 0]);
        roll = std::atan2(R[1 * 3 + 2], R[2 * 3 + 2]);
    }
    pitch = std::atan2(-R[0 * 3 + 2], sy);
}

/* Rot() of the reference's pose (PoseCUAHN.h:119 -> HamQuat.h:80,104) is Ham_quat_2_Rot of the state's quaternion (quat_ops.h:546-550): quat_to_rot above.
 * b_R_w = i0_R_w^T Rot()^T i0_R_w (:123) with i0_R_w = [0 -1 0; -1 0 0; 0 0 -1] (:64), multiplied left to right as Eigen evaluates it. */
inline void odometry_from_state(const State& s, double t_cam, double cam_imu_dt, Odometry& o) {
    o.t_cam = t_cam;
    o.t_imu = t_cam + cam_imu_dt;
    for (int i = 0; i < 3; i++) { o.p[i] = s.p[i]; o.v[i] = s.v[i]; }
    for (int i = 0; i < 4; i++) o.q[i] = s.q[i];
    double R[9], Rt[9], A[9], B[9];
    quat_to_rot(s.q, R);
    mat3_vec(R, s.p, o.w_pos);
    const double i0_R_w[9] = {0.0, -1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0};      /* symmetric: its own transpose */
    m3::transpose(R, Rt);
    m3::mul(i0_R_w, Rt, A);
    m3::mul(A, i0_R_w, B);
    rot_to_euler(B, o.rpy[0], o.rpy[1], o.rpy[2]);
    o.body_pos[0] = -o.w_pos[1]; o.body_pos[1] = -o.w_pos[0]; o.body_pos[2] = -o.w_pos[2];
    o.body_vel[0] = -s.v[1]; o.body_vel[1] = -s.v[0]; o.body_vel[2] = -s.v[2];
}

/* ---- the covariance of what odometry_from_state and prior_pixels form (hnet_filters_predict_cov, include/hnet.h).  The reference publishes
 * geometry_msgs::PoseWithCovarianceStamped from publish_state and never fills its covariance (RosVisualizer.cpp:161-176).
 * The error state perturbs the attitude on the RIGHT: update() applies q <- q (x) dq(dtheta) through quat_apply_rotvec, so Rot() <- R Exp(dtheta) with
 * R = quat_to_rot(q) (J_dc_q = -ez^T R skew(p + t) in propagate_jacobians_fill says the same), and p is additive in the IMU frame.  With
 * w_pos = R p:  d w_pos = R dp - R skew(p) dtheta, and R Exp(dtheta) = Exp(R dtheta) R: the rotation vector about the FIXED axes of the frame
 * `global` is R dtheta.  Hence J = [[R, -R skew(p)], [0, R]] on (dp, dtheta) = error states 0 .. 5, and pose_cov = J P6 J^T in the order of a ROS
 * PoseWithCovariance (x, y, z, rotation about x, y, z).  tests/test_filters_predict_cov_cpu.py pins J against central differences of update()'s own
 * perturbation.  There is no roll / pitch / yaw covariance: the Euler Jacobian is singular at rot_to_euler's sy < 1e-6 branch. */
struct OdometryCov {
    double pose_cov[36];               /* (w_pos, rotation vector about the axes of `global`), row major 6 x 6 */
    double body_pos_cov[9];            /* of Odometry::body_pos: the signed permutation (-y, -x, -z) applied to pose_cov[0:3, 0:3] */
    double body_vel_cov[9];            /* of Odometry::body_vel: the same permutation applied to cov[6:9, 6:9] */
    double prior_cov_px[64];           /* of prior_pixels' prior_px: 159.5^2 cov[sel(i)][sel(j)], row major 8 x 8 */
};

/* the error state that measurement component j selects (update(), innovation(): 15 + 3 c + k) */
inline int meas_row(int j) { return 15 + 3 * (j >> 1) + (j & 1); }
/* (-y, -x, -z): component i of body_pos / body_vel is minus component frd_src(i); the two signs of a covariance element cancel */
inline int frd_src(int i) { return i == 0 ? 1 : i == 1 ? 0 : 2; }

/* J [6 x 6], row major */
inline void pose_cov_jacobian(const State& s, double J[36]) {
    double R[9], Sp[9], RS[9];
    quat_to_rot(s.q, R);
    m3::skew(s.p, Sp);
    m3::mul(R, Sp, RS);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            J[i * 6 + j] = R[i * 3 + j];
            J[i * 6 + 3 + j] = -RS[i * 3 + j];
            J[(3 + i) * 6 + j] = 0.0;
            J[(3 + i) * 6 + 3 + j] = R[i * 3 + j];
        }
}
/* element (i, j) of T = J P6 and of T J^T, the inner index ascending (the style of propagate_cov: the device forms one element per lane with these) */
inline double pose_cov_left(const double J[36], const double* cov, int i, int j) {
    double a = 0.0;
    for (int k = 0; k < 6; k++) a += J[i * 6 + k] * cov[k * NS + j];
    return a;
}
inline double pose_cov_elem(const double T[36], const double J[36], int i, int j) {
    double a = 0.0;
    for (int k = 0; k < 6; k++) a += T[i * 6 + k] * J[j * 6 + k];
    return a;
}
inline double body_vel_cov_elem(const double* cov, int i, int j) { return cov[(6 + frd_src(i)) * NS + 6 + frd_src(j)]; }
inline double prior_cov_px_elem(const double* cov, int i, int j) { return (F_PIX * F_PIX) * cov[meas_row(i) * NS + meas_row(j)]; }

inline void odometry_cov_from_state(const State& s, OdometryCov& c) {
    double J[36], T[36];
    pose_cov_jacobian(s, J);
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) T[i * 6 + j] = pose_cov_left(J, s.cov, i, j);
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) c.pose_cov[i * 6 + j] = pose_cov_elem(T, J, i, j);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            c.body_pos_cov[i * 3 + j] = c.pose_cov[frd_src(i) * 6 + frd_src(j)];
            c.body_vel_cov[i * 3 + j] = body_vel_cov_elem(s.cov, i, j);
        }
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) c.prior_cov_px[i * 8 + j] = prior_cov_px_elem(s.cov, i, j);
}

/* ---- initialisation from a standing start: what VioManager::try_to_initialize (VioManager.cpp:312-363) does with the buffered IMU
 * readings: InertialInitializer::initialize_with_imu_CUAHN (ov_core/src/init/InertialInitializer.cpp:163-279) for the mean and
 * StateHelper::initialize_Cov (StateHelper.cpp:35-61) for the covariance.  The device filters (hnet_filters_advance, include/hnet.h) form the window
 * sums as reductions and run init_decide / init_from_stats / initialize_cov below on them; tests/test_filters_feed_cpu.py checks every function
 * against a numpy restatement. */

/* the two retention rules of the reference's IMU buffers, for readings[0 .. n) in time order: the index of the first reading that is kept.
 * The initialiser drops from the front while a reading is older than three windows behind the newest (InertialInitializer.cpp:28-38); the propagator
 * drops every reading more than 10 s behind the newest (Propagator.h:110-124; a prefix, the readings being in time order). */
inline int trim_imu_init(const ImuData* readings, int n, double newest_t, double window_time) {
    int k = 0;
    while (k < n && readings[k].t < newest_t - 3 * window_time) k++;
    return k;
}
inline int trim_imu_prop(const ImuData* readings, int n, double newest_t) {
    int k = 0;
    while (k < n && newest_t - readings[k].t > 10) k++;
    return k;
}

/* The part of readings[0 .. n) (time order) that select_imu_readings(readings, n, t0, t1, .) can touch, from two counts: n_lt readings with
 * t < t0 and n_le readings with t <= t1.  Every pair before the reading just below t0 fails all three tests of the loop, and the loop ends at the
 * first pair whose later reading is past t1 or, when that pair opened the window (IMU slower than the camera), one pair later; so
 * select_imu_readings(readings + first, len, t0, t1, .) writes what the whole history gives.  (Its `i == 0` test needs a reading past t1 at the
 * start of the span, which only a span that starts at reading 0 can have.)  Returns len; the device filters find the counts in parallel. */
inline int select_span(int n, int n_lt, int n_le, int* first) {
    *first = 0;
    if (n <= 0) return 0;
    const int lo = n_lt > 0 ? n_lt - 1 : 0;
    const int hi = n_le + 1 < n - 1 ? n_le + 1 : n - 1;
    *first = lo;
    return hi >= lo ? hi - lo + 1 : 0;
}

/* InertialInitializer.cpp:216-229: the two refusals on the windows' sample deviations (wait_for_jerk: VioManager.cpp:322, always true there).
 * dev_1to0: newest window, dev_2to1: the window before it.  A window of ONE reading has a deviation of 0 / (1 - 1) = NaN (:197, :212 divide by
 * size - 1); both comparisons are then false and the window passes, as in the reference: written with the reference's `<` and `>` so that it stays so. */
inline bool init_decide(double dev_1to0, double dev_2to1, double imu_thresh, bool wait_for_jerk) {
    if (dev_1to0 < imu_thresh && wait_for_jerk) return false;              /* no excitation yet */
    if (dev_2to1 > imu_thresh && wait_for_jerk) return false;              /* started up moving: wait for a stationary period */
    return true;
}

/* InertialInitializer.cpp:231-270: the mean from the older window's average specific force a_avg and angular velocity w_avg.  z axis along a_avg,
 * e_1 made perpendicular to it, y = z x x, Ro = [x y z]; q = rot_2_Ham_quat(Ro^T) (quat_ops.h:558-571, Hamilton w, x, y, z, no sign convention
 * applied), ba = a_avg - Ro (0, 0, g), bg = w_avg, p = Ro (0, 0, init_height), v = 0.  Offsets and covariance of `s` are not touched. */
inline void init_from_stats(const double a_avg[3], const double w_avg[3], double init_height, double gravity_mag, State& s) {
    const double an = std::sqrt(m3::dot(a_avg, a_avg));
    const double z[3] = {a_avg[0] / an, a_avg[1] / an, a_avg[2] / an};
    const double e1[3] = {1.0, 0.0, 0.0};
    double zz[9], zze[3], x[3], y[3];
    m3::outer(z, z, zz);
    mat3_vec(zz, e1, zze);                                                 /* z z^T e_1 (:238) */
    for (int i = 0; i < 3; i++) x[i] = e1[i] - zze[i];
    const double xn = std::sqrt(m3::dot(x, x));
    for (int i = 0; i < 3; i++) x[i] = x[i] / xn;
    cross(z, x, y);                                                        /* skew_x(z) x (:242) */
    const double Ro[9] = {x[0], y[0], z[0], x[1], y[1], z[1], x[2], y[2], z[2]};
    /* rot_2_Ham_quat(Ro^T): rot(i, j) = Ro[j * 3 + i] */
    const double T = Ro[0] + Ro[4] + Ro[8];
    double q[4];
    q[0] = 0.5 * std::sqrt(1 + T);
    q[1] = (Ro[1 * 3 + 2] - Ro[2 * 3 + 1]) / (4 * q[0]);
    q[2] = (Ro[2 * 3 + 0] - Ro[0 * 3 + 2]) / (4 * q[0]);
    q[3] = (Ro[0 * 3 + 1] - Ro[1 * 3 + 0]) / (4 * q[0]);
    const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; i++) s.q[i] = q[i] / qn;
    const double grav[3] = {0.0, 0.0, gravity_mag}, wp[3] = {0.0, 0.0, init_height};
    double Rg[3];
    mat3_vec(Ro, grav, Rg);
    mat3_vec(Ro, wp, s.p);
    for (int i = 0; i < 3; i++) { s.ba[i] = a_avg[i] - Rg[i]; s.bg[i] = w_avg[i]; s.v[i] = 0.0; }
}

/* InertialInitializer::initialize_with_imu_CUAHN on readings[0 .. n) (time order; the caller has applied trim_imu_init, as feed_imu does).
 * Windows (newest - 2w, newest - w] and (newest - w, newest]; refuses (false, nothing written) fewer than two readings, a span below 2 w, an
 * empty window, and what init_decide refuses.  The deviations are sqrt(sum |a - a_avg|^2 / (size - 1)) (see init_decide for size 1).
 * On success the mean of `s` is set (init_from_stats) and time0 is the time of the LAST reading of the OLDER window (:259). */
inline bool initialize_with_imu(const ImuData* readings, int n, double window_time, double imu_thresh, double init_height, bool wait_for_jerk,
                                double gravity_mag, double& time0, State& s) {
    if (n < 2) return false;
    const double newest = readings[n - 1].t, oldest = readings[0].t;
    if (newest - oldest < 2 * window_time) return false;
    int n1 = 0, n2 = 0, last2 = -1;
    double a1[3] = {0, 0, 0}, a2[3] = {0, 0, 0}, w2[3] = {0, 0, 0};
    for (int k = 0; k < n; k++) {
        const ImuData& d = readings[k];
        if (d.t > newest - 1 * window_time && d.t <= newest - 0 * window_time) {
            for (int i = 0; i < 3; i++) a1[i] += d.am[i];
            n1++;
        }
        if (d.t > newest - 2 * window_time && d.t <= newest - 1 * window_time) {
            for (int i = 0; i < 3; i++) { a2[i] += d.am[i]; w2[i] += d.wm[i]; }
            n2++;
            last2 = k;
        }
    }
    if (n1 == 0 || n2 == 0) return false;
    for (int i = 0; i < 3; i++) { a1[i] /= n1; a2[i] = a2[i] / n2; w2[i] = w2[i] / n2; }
    double v1 = 0, v2 = 0;
    for (int k = 0; k < n; k++) {
        const ImuData& d = readings[k];
        if (d.t > newest - 1 * window_time && d.t <= newest - 0 * window_time) {
            const double e[3] = {d.am[0] - a1[0], d.am[1] - a1[1], d.am[2] - a1[2]};
            v1 += m3::dot(e, e);
        }
        if (d.t > newest - 2 * window_time && d.t <= newest - 1 * window_time) {
            const double e[3] = {d.am[0] - a2[0], d.am[1] - a2[1], d.am[2] - a2[2]};
            v2 += m3::dot(e, e);
        }
    }
    v1 = std::sqrt(v1 / (n1 - 1));
    v2 = std::sqrt(v2 / (n2 - 1));
    if (!init_decide(v1, v2, imu_thresh, wait_for_jerk)) return false;
    init_from_stats(a2, w2, init_height, gravity_mag, s);
    time0 = readings[last2].t;
    return true;
}

/* StateHelper::initialize_Cov (StateHelper.cpp:35-61) on s.cov with s.q: zero x / y position variance (the 2 x 2 block), z 0.005^2; roll / pitch
 * (0.5 / 180 * 3.14159265)^2 with the reference's literal, yaw 0; ba 0.005^2 I, bg 0; then the p and q blocks go into the local frame,
 * w_R_i^T B w_R_i.  Like the reference it overwrites those entries only: it is meant for the all-zero covariance of a new State (State.cpp:79). */
inline void initialize_cov(State& s) {
    double* P = s.cov;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++) P[i * NS + j] = 0.0;
    P[2 * NS + 2] = 0.005 * 0.005;
    const double std_degree = 0.5;
    P[3 * NS + 3] = (std_degree / 180.0 * 3.14159265) * (std_degree / 180.0 * 3.14159265);
    P[4 * NS + 4] = (std_degree / 180.0 * 3.14159265) * (std_degree / 180.0 * 3.14159265);
    P[5 * NS + 5] = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            P[(9 + i) * NS + 9 + j] = (i == j ? 1.0 : 0.0) * 0.005 * 0.005;
            P[(12 + i) * NS + 12 + j] = (i == j ? 1.0 : 0.0) * 0.0000 * 0.0000;
        }
    double R[9], Rt[9];
    quat_to_rot(s.q, R);
    m3::transpose(R, Rt);
    for (int b = 0; b < 6; b += 3) {
        double B[9], t[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) B[i * 3 + j] = P[(b + i) * NS + b + j];
        m3::mul(Rt, B, t);
        m3::mul(t, R, B);
        set_block(P, NS, b, b, B);
    }
}

}  // namespace hnet_ekf
#endif  /* HNET_EKF_H */
