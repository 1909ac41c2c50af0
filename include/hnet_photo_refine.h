/* hnet_photo_refine.h — a photometric alignment as a filter measurement (include/hnet.h hnet_filters_set_photo_refine), dependency free: what
 * the device (csrc/kernels_filters_refine.hip) and the host reference (tests/cpp/filters_photo_refine_ref.cpp) both compile, next to
 * include/hnet_photo_robust.h (the alignment's record) and include/hnet_ekf.h (the update that consumes the measurement).
 *
 * The measurement.  From the level-0 record of an alignment, all in double:
 *   info8 = the information matrix of the eight offsets with gain and bias marginalised (marginal below: the Schur complement of the 2 x 2 brightness
 *           block of info10; with the model off, px.info),
 *   R_px  = cov_scale * px.mse * inverse(info8) + sigma_floor_px^2 I, symmetrised as 0.5 (R + R^T), the inverse by hnet_ekf::invert,
 *   out72 = px.offsets_px (8) | (float)(R_px / k_net_cov) (64): the packed record hnet_ekf::update and innovation take from the network, so that the
 *           unchanged update forms k_net_cov * C / 159.5^2 = R_px / 159.5^2.
 * cov_scale is the caller's: mse * inverse(info8) is the covariance of a least-squares estimate with independent residuals, which neighbouring pixels
 * are not (the float64 prototype found it 2 - 6 x too small); nothing here calibrates it.
 * A record is UNUSABLE, with one reason bit and nothing written to out72 / r_px, when (tested in this order) k_net_cov is not finite and positive; the
 * record stopped SINGULAR, DEGENERATE or FEW_PIXELS; no trial was accepted at any level (the "measurement" would be the prior itself and only shrink the
 * covariance); max_mse > 0 and px.mse exceeds it; the marginal has no Cholesky factor (the 2 x 2 block, or info8 by hnet_align's pivot test: a pivot
 * <= 1e-12 max diag) or hnet_ekf::invert reports singular; an entry of R_px is not finite.
 * Every body is non-contracting and element-wise where the device works one element per lane: the two sides make the same operations in the same order.
 */
#ifndef HNET_PHOTO_REFINE_H
#define HNET_PHOTO_REFINE_H

#include "hnet_ekf.h"
#include "hnet_photo_robust.h"

namespace hnet_refine {

namespace pa = hnet_align;
namespace pr = hnet_robust;

/* = hnet_photo_refine_opts */
struct Opts { pr::Opts align; int32_t levels, pad; double cov_scale, sigma_floor_px, max_mse; };
inline void default_opts(Opts& o) { pr::default_opts(o.align); o.levels = 3; o.pad = 0; o.cov_scale = 0.0; o.sigma_floor_px = 0.05; o.max_mse = 0.0; }
inline bool opts_valid(const Opts& o) {
    return pr::opts_valid(o.align) && o.levels >= 1 && o.levels <= pa::MAX_LEVELS && o.cov_scale > 0.0 && std::isfinite(o.cov_scale) && o.sigma_floor_px >= 0.0 &&
           std::isfinite(o.sigma_floor_px) && o.max_mse >= 0.0 && std::isfinite(o.max_mse);
}

/* the flags of a refine record (= HNET_REFINE_*) */
enum { ASKED = 1,                      /* the photometric gate refused iteration 0 of a session with refinement on: the alignment's record is this one's */
       APPLIED = 2,                    /* the fallback update was applied */
       NIS_REJECTED = 4,               /* the session's NIS gate refused the fallback measurement */
       S_SINGULAR = 8,                 /* update() found the fallback's S singular */
       BAD_K_NET_COV = 16,             /* UNUSABLE: k_net_cov not finite and positive */
       STOPPED = 32,                   /* UNUSABLE: the record's flags hold SINGULAR, DEGENERATE or FEW_PIXELS */
       NO_STEP = 64,                   /* UNUSABLE: no trial accepted at any level */
       MSE_ABOVE_MAX = 128,            /* UNUSABLE: max_mse > 0 and px.mse > max_mse */
       NO_FACTOR = 256,                /* UNUSABLE: the marginal has no Cholesky factor, or the inverse reports singular */
       NON_FINITE = 512,               /* UNUSABLE: an entry of R_px is not finite */
       UNUSABLE = BAD_K_NET_COV | STOPPED | NO_STEP | MSE_ABOVE_MAX | NO_FACTOR | NON_FINITE };

/* = hnet_photo_refine: the level-0 record, R_px, the fallback's innovation (hnet_innovation: r, s_diag, nis, iteration = max_iekf_iteration, flag) */
struct Record {
    pr::Record rec;
    double r_px[pa::NX * pa::NX];
    double r[8], s_diag[8], nis;
    int32_t iteration, flag;
    int32_t flags, pad;
};

/* ---- the marginal.  The brightness block of info10 as its Cholesky factor [[l00, 0], [l10, l11]]; off: rows and columns 8, 9 are all zero (the model was off) */
struct Bright { double l00, l10, l11; bool off; };
inline bool marginal_factor(const pr::Record& rec, Bright& f) {
    HNET_ALIGN_NO_CONTRACT
    const double* A = rec.info10;
    f.off = true;
    f.l00 = f.l10 = f.l11 = 0.0;
    for (int j = 0; j < pr::NP; j++) f.off = f.off && A[80 + j] == 0.0 && A[90 + j] == 0.0 && A[j * 10 + 8] == 0.0 && A[j * 10 + 9] == 0.0;
    if (f.off) return true;
    const double a = A[88], b = A[89], d = A[99];
    if (!(a > 0.0) || !std::isfinite(a)) return false;
    f.l00 = std::sqrt(a);
    f.l10 = b / f.l00;
    const double d2 = d - f.l10 * f.l10;
    if (!(d2 > 0.0) || !std::isfinite(d2)) return false;
    f.l11 = std::sqrt(d2);
    return true;
}
/* y = L^-1 (column i of A_cx) */
inline void marginal_y(const pr::Record& rec, const Bright& f, int i, double& y0, double& y1) {
    HNET_ALIGN_NO_CONTRACT
    y0 = rec.info10[i * 10 + 8] / f.l00;
    y1 = (rec.info10[i * 10 + 9] - f.l10 * y0) / f.l11;
}
/* entry (i, j) of info8 = A_xx - A_xc A_cc^-1 A_cx */
inline double marginal_info(const pr::Record& rec, const Bright& f, int i, int j) {
    HNET_ALIGN_NO_CONTRACT
    if (f.off) return rec.px.info[i * pa::NX + j];
    double yi0, yi1, yj0, yj1;
    marginal_y(rec, f, i, yi0, yi1);
    marginal_y(rec, f, j, yj0, yj1);
    return rec.info10[i * 10 + j] - (yi0 * yj0 + yi1 * yj1);
}
/* entry i of grad8 = g_x - A_xc A_cc^-1 g_c */
inline double marginal_grad(const pr::Record& rec, const Bright& f, int i) {
    HNET_ALIGN_NO_CONTRACT
    if (f.off) return rec.px.grad[i];
    double y0, y1;
    marginal_y(rec, f, i, y0, y1);
    const double yg0 = rec.grad10[8] / f.l00, yg1 = (rec.grad10[9] - f.l10 * yg0) / f.l11;
    return rec.grad10[i] - (y0 * yg0 + y1 * yg1);
}
/* hnet_photo_robust_marginal: false (nothing written) when the 2 x 2 block has no Cholesky factor */
inline bool marginal(const pr::Record& rec, double info8[64], double grad8[8]) {
    Bright f;
    if (!marginal_factor(rec, f)) return false;
    for (int i = 0; i < pa::NX; i++) {
        for (int j = 0; j < pa::NX; j++) info8[i * pa::NX + j] = marginal_info(rec, f, i, j);
        grad8[i] = marginal_grad(rec, f, i);
    }
    return true;
}

/* ---- the measurement, in the pieces the device runs on different lanes */
/* what can be judged before any matrix is formed: 0, or the reason bit */
inline int precheck(const pr::Record& rec, int accepted_total, double max_mse, double k_net_cov) {
    if (!(k_net_cov > 0.0) || !std::isfinite(k_net_cov)) return BAD_K_NET_COV;
    if (rec.px.flags & (pa::SINGULAR | pa::DEGENERATE | pa::FEW_PIXELS)) return STOPPED;
    if (accepted_total == 0) return NO_STEP;
    if (max_mse > 0.0 && rec.px.mse > max_mse) return MSE_ABOVE_MAX;
    return 0;
}
/* hnet_align's pivot test on info8 (solve_damped's: pivots of the undamped matrix above 1e-12 max diag).  L: 64 doubles of scratch */
inline bool has_factor(const double* info8, double* L) {
    HNET_ALIGN_NO_CONTRACT
    double top = 0.0;
    for (int i = 0; i < pa::NX; i++) top = info8[i * pa::NX + i] > top ? info8[i * pa::NX + i] : top;
    const double tiny = 1e-12 * top;
    return std::isfinite(tiny) && pa::cholesky(info8, 0.0, tiny, L);
}
/* entry (i, j) of R_px from inv = inverse(info8) and the record's mse */
inline double r_px_entry(const double* inv, double mse, double cov_scale, double sigma_floor_px, int i, int j) {
    HNET_ALIGN_NO_CONTRACT
    const double s = cov_scale * mse, fl = i == j ? sigma_floor_px * sigma_floor_px : 0.0;
    const double a = s * inv[i * pa::NX + j] + fl, b = s * inv[j * pa::NX + i] + fl;
    return 0.5 * (a + b);
}
inline float cov72_entry(double r_px, double k_net_cov) { HNET_ALIGN_NO_CONTRACT return (float)(r_px / k_net_cov); }

/* -> true: out72 [72] and r_px [64] written, flags untouched; false: UNUSABLE, the reason bit set in flags and nothing else written */
inline bool refine_measurement(const pr::Record& rec, int accepted_total, const Opts& o, double k_net_cov, float* out72, double* r_px, int32_t& flags) {
    if (const int why = precheck(rec, accepted_total, o.max_mse, k_net_cov)) { flags |= why; return false; }
    Bright f;
    double M[64], L[64], R[64];
    if (!marginal_factor(rec, f)) { flags |= NO_FACTOR; return false; }
    for (int i = 0; i < pa::NX; i++)
        for (int j = 0; j < pa::NX; j++) M[i * pa::NX + j] = marginal_info(rec, f, i, j);
    if (!has_factor(M, L) || !hnet_ekf::invert(M, 8)) { flags |= NO_FACTOR; return false; }
    bool finite = true;
    for (int i = 0; i < pa::NX; i++)
        for (int j = 0; j < pa::NX; j++) {
            R[i * pa::NX + j] = r_px_entry(M, rec.px.mse, o.cov_scale, o.sigma_floor_px, i, j);
            finite = finite && std::isfinite(R[i * pa::NX + j]);
        }
    if (!finite) { flags |= NON_FINITE; return false; }
    for (int i = 0; i < pa::NX; i++) out72[i] = rec.px.offsets_px[i];
    for (int e = 0; e < 64; e++) {
        r_px[e] = R[e];
        out72[8 + e] = cov72_entry(R[e], k_net_cov);
    }
    return true;
}

}  /* namespace hnet_refine */

namespace hnet_ekf {

/* iterated_update_photo_gated followed by the fallback.  refine: null = refinement off for this filter, and everything is iterated_update_photo_gated's,
 * bit for bit.  The fallback runs iff the photometric gate refused the estimate of iteration 0 (prec[1] holds PHOTO_REJECTED; no update of the call was
 * applied then, and the state the loop worked on is the propagated one).  align(x0 [8] float, rec, accepted_total): the caller's alignment of the frame
 * pair from iteration 0's fp32 prior - the level-0 record and the trials accepted over all levels.  Then refine_measurement, innovation (with the NIS
 * gate when max_nis > 0) and update with the prior of the unchanged state and update_offset = false, and reset_4pt_offset as after the last iteration.
 * A refusal at a later iteration, a NIS rejection and a singular S trigger no fallback.  out: zeros when the fallback did not run; else flags ASKED and
 * what became of it, the record, R_px and the innovation (iteration = max_iekf_iteration; flag NONE when the measurement was unusable).
 * Returns the updates applied, the fallback's included. */
template <class Net, class Vec8, class Photo, class Align>
inline int iterated_update_photo_refined(State& s, Net& net, int max_iekf_iteration, double k_net_cov, Vec8& prior_px_vec, double time_stamp, double max_nis,
                                         Innovation* rec, Photo& photo, double max_ratio, int min_inside, PhotoRecord* prec, const hnet_refine::Opts* refine,
                                         Align& align, hnet_refine::Record& out) {
    std::memset(&out, 0, sizeof out);
    const State before = s;
    int done = iterated_update_photo_gated(s, net, max_iekf_iteration, k_net_cov, prior_px_vec, time_stamp, max_nis, rec, photo, max_ratio, min_inside, prec);
    if (!refine || !(prec[1].flags & PHOTO_REJECTED)) return done;
    s = before;
    double prior_px[8], prior_cam[8];
    prior_pixels(s, prior_px, prior_cam);
    float x0[8], m72[72];
    for (int i = 0; i < 8; i++) x0[i] = (float)prior_px[i];
    int accepted_total = 0;
    align(x0, out.rec, accepted_total);
    out.flags = hnet_refine::ASKED;
    out.iteration = max_iekf_iteration;
    out.flag = INNOV_NONE;
    if (hnet_refine::refine_measurement(out.rec, accepted_total, *refine, k_net_cov, m72, out.r_px, out.flags)) {
        double mean[8], cov[64];
        for (int i = 0; i < 8; i++) mean[i] = (double)m72[i];
        for (int e = 0; e < 64; e++) cov[e] = (double)m72[8 + e];
        Innovation inn;
        innovation(s, mean, cov, prior_cam, k_net_cov, inn);
        std::memcpy(out.r, inn.r, sizeof out.r);
        std::memcpy(out.s_diag, inn.s_diag, sizeof out.s_diag);
        out.nis = inn.nis;
        out.flag = inn.flag;
        if (max_nis > 0.0 && inn.nis > max_nis) {
            out.flag = INNOV_REJECTED;
            out.flags |= hnet_refine::NIS_REJECTED;
        } else if (!update(s, mean, cov, prior_cam, k_net_cov, false)) {
            out.flags |= hnet_refine::S_SINGULAR;
        } else {
            out.flags |= hnet_refine::APPLIED;
            done++;
        }
    }
    reset_4pt_offset(s);
    return done;
}

}  /* namespace hnet_ekf */

#endif /* HNET_PHOTO_REFINE_H */
