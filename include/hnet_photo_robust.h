/* hnet_photo_robust.h — photometric alignment with a gain / bias model and Huber weights (include/hnet.h hnet_op_photo_align_robust),
 * dependency free: what the device (csrc/kernels_photo_robust.hip) and the host reference (tests/cpp/photo_robust_ref.cpp) both compile, next to
 * include/hnet_photo_align.h and include/hnet_photo_pyramid.h, whose geometry, Jacobian and reduction of the offset block serve unchanged.
 *
 * The quantity.  Ten parameters: the eight corner offsets x (px), the gain G = 1 + a and the bias b (grey levels).  At level L everything geometric is
 * hnet_photo_pyramid.h's: H = (float) dlt_solve(p4 + x), level_coords / level_position / level_row give validity, the four taps and the row s[9] of
 * d(w 255) / dvec(H); w (0 .. 1) is the bilinear sample (sample).  Per VALID pixel, in fp32 with one rounding per written operation,
 *   r = (fmaf(Gf, w, bf) - i1f) * 255,   Gf = (float) G, bf = (float)(b / 255);   at G = 1, b = 0 this is hnet_photo_align.h's r bit for bit.
 * With k = (float) huber_k (grey levels, 0 = quadratic): |r| <= k or k == 0: omega = 1, rho = r^2; otherwise omega = k / |r|, rho = k (2 |r| - k).  rho (formed in
 * double from the fp32 r and k) is the Huber loss scaled so that k = 0 gives r^2: a fixed function of the ten parameters, so the loop is
 * Levenberg-Marquardt descent on sum rho, not IRLS on a moving target.
 * The row is t[11] = (s[0 .. 8], w 255, 1), the weighted row tw[i] = omega t[i] (fp32, one rounding), and one linearisation (Sums) is the 66 unique
 * entries of sum tw t^T (entry (i, j), i <= j, is sum (double) tw[i] (double) t[j]), the 11 of sum tw r, sum rho, the count of valid pixels and of those
 * with omega < 1.  Every product is an exact product of two floats: the device and the host reference differ by the order of addition only.
 *
 * The reduction.  D (9 x 8) is dlt_jacobian_col's; T / A / g of the s block go through form_T / form_A / form_g.  dr / dx = G D^T s, so
 *   A10 = [[G^2 D^T S_ss D, G D^T S_sc], [sym, S_cc]],   g10 = [G D^T S_sr ; S_cr].
 * With the brightness model off the system is the 8 x 8 block alone at G = 1 and gain / bias never move; with huber_k = 0 besides, every common field of
 * a record equals hnet_photo_align.h's byte for byte (x 1 is exact, omega = 1 leaves tw = t, and step() below makes hnet_align::step's operations in
 * its order).
 */
#ifndef HNET_PHOTO_ROBUST_H
#define HNET_PHOTO_ROBUST_H

#include "hnet_photo_pyramid.h"

namespace hnet_robust {

namespace pa = hnet_align;

constexpr int NT = 11, NP = 10, NSYM_T = 66;  /* entries of the row t, parameters, unique entries of a symmetric 11 x 11 */
constexpr int ND = NSYM_T + NT + 1;           /* 78 double sums: tt | tr | rho */

/* = hnet_photo_robust_opts */
struct Opts { pa::Opts base; int32_t brightness, pad; double huber_k, gain0, bias0; };
inline void default_opts(Opts& o) { pa::default_opts(o.base); o.brightness = 1; o.pad = 0; o.huber_k = 10.0; o.gain0 = 1.0; o.bias0 = 0.0; }
inline bool opts_valid(const Opts& o) {
    if (!pa::opts_valid(o.base) || (o.brightness != 0 && o.brightness != 1)) return false;
    if (!std::isfinite(o.huber_k) || o.huber_k < 0.0 || !std::isfinite(o.gain0) || !(o.gain0 > 0.0) || !std::isfinite(o.bias0)) return false;
    return o.brightness == 1 || (o.gain0 == 1.0 && o.bias0 == 0.0);
}

/* one linearisation, as the accumulate kernel leaves it per row slice and the solve kernel adds it up */
struct Sums { double tt[NSYM_T], tr[NT], rho; int32_t n_valid, n_outliers; };
constexpr int sym_index(int i, int j) { return i * NT - (i * (i - 1)) / 2 + (j - i); }
inline double sym_at(const double* tt, int i, int j) { return i <= j ? tt[sym_index(i, j)] : tt[sym_index(j, i)]; }

/* = hnet_photo_robust */
struct Record {
    pa::Record px;                 /* mse0 / mse: the mean robust cost; grad / info: the offset block at the current gain */
    double gain, bias;
    int32_t n_outliers0, n_outliers;
    double grad10[NP], info10[NP * NP];
};
/* what a pair carries from one solve to the next besides its record: the trial point and the step that led to it */
struct Work { double dp[NP]; double gain_trial, bias_trial; float x_trial[pa::NX]; };
/* where a level starts: the offsets, gain and bias the level above ended at (the call's at the coarsest level) */
struct Start { float x[pa::NX]; double gain, bias; };

/* the fp32 forms of gain, bias and k the per-pixel quantity uses */
inline float gain_f(double G) { HNET_ALIGN_NO_CONTRACT return (float)G; }
inline float bias_f(double b) { HNET_ALIGN_NO_CONTRACT return (float)(b / 255.0); }
inline float huber_f(double k) { HNET_ALIGN_NO_CONTRACT return (float)k; }

/* the bilinear sample w of level_row's four taps (its own expressions) */
inline float sample(float a, float b, float c, float d, float ix, float iy) {
    HNET_ALIGN_NO_CONTRACT
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float wx1 = ix - x0f, wx0 = 1.0f - wx1, wy1 = iy - y0f, wy0 = 1.0f - wy1;
    float w = fmaf(a, wx0 * wy0, 0.0f);
    w = fmaf(b, wx1 * wy0, w);
    w = fmaf(c, wx0 * wy1, w);
    w = fmaf(d, wx1 * wy1, w);
    return w;
}

/* residual, weight and cost of a valid pixel; true when the pixel is an outlier (omega < 1) */
inline bool residual(float Gf, float bf, float kf, float w, float i1, float& r, float& omega, double& rho) {
    HNET_ALIGN_NO_CONTRACT
    r = (fmaf(Gf, w, bf) - i1) * 255.0f;
    const float ar = fabsf(r);
    if (kf == 0.0f || ar <= kf) {
        omega = 1.0f;
        rho = (double)r * (double)r;
        return false;
    }
    omega = kf / ar;
    rho = (double)kf * (2.0 * (double)ar - (double)kf);
    return omega < 1.0f;
}

/* the row t and its weighted form from level_row's s */
inline void weighted_row(const float s[pa::NH], float w, float omega, float t[NT], float tw[NT]) {
    HNET_ALIGN_NO_CONTRACT
    for (int i = 0; i < pa::NH; i++) t[i] = s[i];
    t[9] = w * 255.0f;
    t[10] = 1.0f;
    for (int i = 0; i < NT; i++) tw[i] = omega * t[i];
}

/* the s block of the sums in hnet_align's 9 x 9 order (form_T reads it): entry e of 45 */
inline double ss_entry(const double* tt, int e) {
    HNET_ALIGN_NO_CONTRACT
    int i = 0, rest = e;
    while (rest >= pa::NH - i) { rest -= pa::NH - i; i++; }
    return tt[sym_index(i, i + rest)];
}

/* entry (i, j), i <= j, of A10 at gain G; A8 = D^T S_ss D entry (i, j) for i, j < 8 (form_A's); the caller mirrors it */
inline double form_A10(const double* D, const double* tt, double G, double A8ij, int i, int j) {
    HNET_ALIGN_NO_CONTRACT
    if (j < pa::NX) return (G * G) * A8ij;
    if (i >= pa::NX) return sym_at(tt, i + 1, j + 1);
    double a = 0.0;
    for (int k = 0; k < pa::NH; k++) a += D[k * pa::NX + i] * sym_at(tt, k, j + 1);
    return G * a;
}
inline double form_g10(const double* D, const double* tr, double G, int i) {
    HNET_ALIGN_NO_CONTRACT
    if (i >= pa::NX) return tr[i + 1];
    return G * pa::form_g(D, tr, i);
}

/* hnet_align::cholesky on the leading P x P block of a matrix with rows of NP: the same operations in the same order */
template <int P>
inline bool cholesky(const double* A, double lambda, double tiny, double* L) {
    HNET_ALIGN_NO_CONTRACT
    for (int j = 0; j < P; j++) {
        double d = A[j * NP + j] + lambda * A[j * NP + j];
        for (int k = 0; k < j; k++) d -= L[j * NP + k] * L[j * NP + k];
        if (!(d > tiny) || !std::isfinite(d)) return false;
        const double ljj = std::sqrt(d);
        L[j * NP + j] = ljj;
        for (int i = j + 1; i < P; i++) {
            double s = A[i * NP + j];
            for (int k = 0; k < j; k++) s -= L[i * NP + k] * L[j * NP + k];
            L[i * NP + j] = s / ljj;
        }
    }
    return true;
}

/* hnet_align::solve_damped for P parameters: dp = -(A + lambda diag(A))^-1 g; false = SINGULAR, judged on the undamped A.  L: 100 doubles of scratch. */
template <int P>
inline bool solve_damped(const double* A, const double* g, double lambda, double* L, double* dp) {
    HNET_ALIGN_NO_CONTRACT
    double top = 0.0;
    for (int i = 0; i < P; i++) top = A[i * NP + i] > top ? A[i * NP + i] : top;
    const double tiny = 1e-12 * top;
    if (!std::isfinite(tiny) || !cholesky<P>(A, 0.0, tiny, L)) return false;
    if (!cholesky<P>(A, lambda, tiny, L)) return false;
    for (int i = 0; i < P; i++) {
        double s = -g[i];
        for (int k = 0; k < i; k++) s -= L[i * NP + k] * dp[k];
        dp[i] = s / L[i * NP + i];
    }
    for (int i = P - 1; i >= 0; i--) {
        double s = dp[i];
        for (int k = i + 1; k < P; k++) s -= L[k * NP + i] * dp[k];
        dp[i] = s / L[i * NP + i];
    }
    bool ok = true;
    for (int i = 0; i < P; i++) ok = ok && std::isfinite(dp[i]);
    return ok;
}

/* hnet_align::step for P = 8 (brightness off) or 10 parameters, after linearisation number `it` of a level (0: at the level's start st; it >= 1: at
 * the trial point in w).  degenerate: the point has no homography; n_valid, n_outliers, rho: its counts and sum rho; A [100], g [10]: A10, g10 at the point's gain.
 *   it >= 1: the trial is ACCEPTED iff it has a homography, its gain is finite and > 0, its bias finite, n_valid >= max(min_valid, 9) and the mean
 *            cost sum rho / n_valid is strictly smaller.  CONVERGED is judged on the eight offset components of the step alone.
 * Everything else is hnet_align::step's.  L: 100 doubles of scratch. */
template <int P>
inline void step_p(Record& rec, Work& w, int it, const Opts& o, const Start& st, bool degenerate, int n_valid, int n_outliers,
                   double rho, const double* A, const double* g, double* L) {
    HNET_ALIGN_NO_CONTRACT
    const int need = o.base.min_valid > 9 ? o.base.min_valid : 9;
    const double cost = n_valid > 0 ? rho / (double)n_valid : 0.0;
    pa::Record& px = rec.px;
    bool take = false;                         /* the linearised point becomes the current point: its A, g are copied into the record */
    if (it == 0) {
        for (int k = 0; k < pa::NX; k++) { px.offsets_px[k] = st.x[k]; px.grad[k] = 0.0; w.x_trial[k] = st.x[k]; }
        for (int k = 0; k < pa::NX * pa::NX; k++) px.info[k] = 0.0;
        for (int k = 0; k < NP; k++) { rec.grad10[k] = 0.0; w.dp[k] = 0.0; }
        for (int k = 0; k < NP * NP; k++) rec.info10[k] = 0.0;
        rec.gain = w.gain_trial = st.gain;
        rec.bias = w.bias_trial = st.bias;
        px.mse0 = px.mse = 0.0;
        px.n_valid0 = px.n_valid = degenerate ? 0 : n_valid;
        rec.n_outliers0 = rec.n_outliers = degenerate ? 0 : n_outliers;
        px.trials = px.accepted = px.flags = px.pad = 0;
        px.lambda = o.base.lambda0;
        if (degenerate) { px.flags = pa::DEGENERATE; return; }
        if (n_valid < need) { px.flags = pa::FEW_PIXELS; return; }
        px.mse0 = px.mse = cost;
        take = true;
    } else {
        px.trials++;
        const bool model_ok = std::isfinite(w.gain_trial) && w.gain_trial > 0.0 && std::isfinite(w.bias_trial);
        if (!degenerate && model_ok && n_valid >= need && cost < px.mse) {
            px.accepted++;
            px.lambda *= 0.1;
            px.mse = cost;
            px.n_valid = n_valid;
            rec.n_outliers = n_outliers;
            rec.gain = w.gain_trial;
            rec.bias = w.bias_trial;
            for (int k = 0; k < pa::NX; k++) px.offsets_px[k] = w.x_trial[k];
            take = true;
        } else {
            px.lambda *= 10.0;
        }
    }
    if (take) {
        /* rows / columns 8, 9 stay zero when the model is off */
        for (int i = 0; i < P; i++) {
            rec.grad10[i] = g[i];
            for (int j = 0; j < P; j++) rec.info10[i * NP + j] = A[i * NP + j];
        }
        for (int i = 0; i < pa::NX; i++) {
            px.grad[i] = g[i];
            for (int j = 0; j < pa::NX; j++) px.info[i * pa::NX + j] = A[i * NP + j];
        }
        if (it > 0) {
            double top = 0.0;
            for (int k = 0; k < pa::NX; k++) {
                const double a = std::fabs(w.dp[k]);
                top = a > top ? a : top;
            }
            if (top < o.base.eps_px) { px.flags |= pa::CONVERGED; return; }
        }
    }
    if (!solve_damped<P>(rec.info10, rec.grad10, px.lambda, L, w.dp)) { px.flags |= pa::SINGULAR; return; }
    for (int k = 0; k < pa::NX; k++) w.x_trial[k] = (float)((double)px.offsets_px[k] + w.dp[k]);
    if (P == NP) {
        w.gain_trial = rec.gain + w.dp[8];
        w.bias_trial = rec.bias + w.dp[9];
    }
}

/* P is a compile-time constant in both forms, so that the loops of the factorisation unroll as hnet_align's do */
inline void step(Record& rec, Work& w, int it, const Opts& o, const Start& st, bool degenerate, int n_valid, int n_outliers, double rho, const double* A,
                 const double* g, double* L) {
    if (o.brightness) step_p<NP>(rec, w, it, o, st, degenerate, n_valid, n_outliers, rho, A, g, L);
    else step_p<pa::NX>(rec, w, it, o, st, degenerate, n_valid, n_outliers, rho, A, g, L);
}

}  /* namespace hnet_robust */

#endif /* HNET_PHOTO_ROBUST_H */
