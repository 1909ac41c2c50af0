/* hnet_photo_align.h — photometric alignment on the eight four-corner offsets (include/hnet.h hnet_photo_align), dependency free:
 * what the device (csrc/kernels_photo_align.hip) and the host reference (tests/cpp/photo_align_ref.cpp) both compile, so that the Jacobian of the DLT,
 * the reduction to the offsets and every decision of the Levenberg-Marquardt loop are the same code on both sides.
 *
 * The quantity.  For offsets x (8 floats, pixels, ul bl br ur) H(x) = (float) dlt_solve(p4 + x); pixel (u, v) samples img2 at (ix, iy) = (X / Z, Y / Z) and
 * is VALID when 0 <= ix < 319 and 0 <= iy < 223 (all four bilinear taps are pixels of img2).  Over the valid pixels, with r = (w - img1 / 255) * 255 the
 * residual in grey levels and (gx, gy) the gradient of the bilinear sample (grey levels per pixel), the row of dr / dvec(H) is
 *   s = (gx u, gx v, gx, gy u, gy v, gy, -q u, -q v, -q) / Z,   q = gx ix + gy iy,
 * and one linearisation is the 45 unique entries of sum s s^T, the 9 of sum s r, sum r^2 and the count (Sums).  D = dvec(H) / dx (9 x 8) is the analytic
 * derivative of csrc/geom.h's dlt_solve, h33 = 1 included (its row is zero); A = D^T (sum s s^T) D, g = D^T (sum s r), mse = sum r^2 / n_valid.
 *
 * Every function below rounds the same on the host and on the device: nothing in this header is contracted into FMAs (HNET_ALIGN_NO_CONTRACT; the host
 * reference is built with -ffp-contract=off).
 */
#ifndef HNET_PHOTO_ALIGN_H
#define HNET_PHOTO_ALIGN_H

#include <cmath>
#include <cstdint>

namespace hnet_align {

/* at the start of a function body: no contraction inside it, whatever the translation unit's setting (the kernels around it keep theirs) */
#if defined(__clang__)
#define HNET_ALIGN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HNET_ALIGN_NO_CONTRACT
#endif

constexpr int NH = 9, NX = 8, NSYM = 45;       /* entries of vec(H), offsets, unique entries of a symmetric 9 x 9 */
constexpr int MAX_ITERATIONS = 32;
enum { CONVERGED = 1,        /* an accepted step moved no offset by eps_px or more: a small STEP, not a small residual.  After a run of refusals (accepted << trials,
                                a large lambda) the damping alone makes it small: read mse against mse0 and lambda before taking it for "aligned" */
       SINGULAR = 2,         /* A at offsets_px has a Cholesky pivot <= 1e-12 max diag(A) (or a non-finite one): the pair does not constrain the 8 offsets */
       DEGENERATE = 4,       /* the start offsets have no homography (a non-finite entry of H) */
       FEW_PIXELS = 8 };     /* fewer than max(min_valid, 9) valid pixels at the start offsets */

struct Opts { int32_t max_iterations, min_valid; double lambda0, eps_px; };
inline void default_opts(Opts& o) { o.max_iterations = 6; o.min_valid = 20000; o.lambda0 = 1e-3; o.eps_px = 1e-3; }
/* lambda0 <= MAX_LAMBDA0: every refusal multiplies lambda by 10, so after MAX_ITERATIONS of them it is at most 1e132, and diag(A) on 8-bit frames is far
 * below 1e100 (2.4e5 on a smooth pair): A[j][j] + lambda A[j][j] cannot overflow in cholesky, and a pair whose undamped A passes the pivot test can never
 * stop SINGULAR because its DAMPED factorisation met an infinite pivot (lambda0 = 1e280 did, after 23 refusals) */
constexpr double MAX_LAMBDA0 = 1e100;
inline bool opts_valid(const Opts& o) {
    return o.max_iterations >= 0 && o.max_iterations <= MAX_ITERATIONS && o.min_valid >= 0 && o.lambda0 > 0.0 && o.lambda0 <= MAX_LAMBDA0 && o.eps_px >= 0.0 &&
           std::isfinite(o.eps_px);
}

/* one linearisation in H-space, as the accumulate kernel leaves it per row slice and the solve kernel adds it up */
struct Sums { double ss[NSYM], sr[NH], rr; int32_t n_valid, pad; };
/* entry (i, j), i <= j, of the upper triangle stored by rows */
constexpr int sym_index(int i, int j) { return i * NH - (i * (i - 1)) / 2 + (j - i); }
inline double sym_at(const double* ss, int i, int j) { return i <= j ? ss[sym_index(i, j)] : ss[sym_index(j, i)]; }

/* = hnet_photo_align (include/hnet.h) */
struct Record {
    float offsets_px[NX];
    double mse0, mse;
    int32_t n_valid0, n_valid, trials, accepted, flags;
    int32_t pad;                   /* the C struct's alignment gap, written as 0: a record is comparable byte for byte */
    double lambda, grad[NX], info[NX * NX];
};
/* what a pair carries from one solve to the next besides its record: the trial offsets and the step that led to them */
struct Work { double dx[NX]; float x_trial[NX]; };

/* the corners dlt_solve receives for offsets x: an fp32 sum, as dlt_kernel and the residual records form them */
inline double corner(double p4k, float xk) { return (double)(float)(p4k + (double)xk); }

/* column k of D: the derivative of csrc/geom.h's dlt_solve (W = 320, H = 224) with respect to dst[k], in forward mode through its own expressions */
inline void dlt_jacobian_col(const double dst[8], int k, double col[NH]) {
    HNET_ALIGN_NO_CONTRACT
    const double x0 = dst[0], y0 = dst[1], x3 = dst[2], y3 = dst[3], x2 = dst[4], y2 = dst[5], x1 = dst[6], y1 = dst[7];
    const double tx0 = k == 0, ty0 = k == 1, tx3 = k == 2, ty3 = k == 3, tx2 = k == 4, ty2 = k == 5, tx1 = k == 6, ty1 = k == 7;
    const double dx1 = x1 - x2, dx2 = x3 - x2, sx = x0 - x1 + x2 - x3;
    const double dy1 = y1 - y2, dy2 = y3 - y2, sy = y0 - y1 + y2 - y3;
    const double tdx1 = tx1 - tx2, tdx2 = tx3 - tx2, tsx = tx0 - tx1 + tx2 - tx3;
    const double tdy1 = ty1 - ty2, tdy2 = ty3 - ty2, tsy = ty0 - ty1 + ty2 - ty3;
    const double det = dx1 * dy2 - dx2 * dy1;
    const double tdet = tdx1 * dy2 + dx1 * tdy2 - tdx2 * dy1 - dx2 * tdy1;
    const double g = (sx * dy2 - sy * dx2) / det, h = (dx1 * sy - dy1 * sx) / det;
    const double tg = ((tsx * dy2 + sx * tdy2 - tsy * dx2 - sy * tdx2) - g * tdet) / det;
    const double th = ((tdx1 * sy + dx1 * tsy - tdy1 * sx - dy1 * tsx) - h * tdet) / det;
    const double iw = 1.0 / 319.0, ih = 1.0 / 223.0;
    col[0] = (tx1 - tx0 + tg * x1 + g * tx1) * iw; col[1] = (tx3 - tx0 + th * x3 + h * tx3) * ih; col[2] = tx0;
    col[3] = (ty1 - ty0 + tg * y1 + g * ty1) * iw; col[4] = (ty3 - ty0 + th * y3 + h * ty3) * ih; col[5] = ty0;
    col[6] = tg * iw;                              col[7] = th * ih;                              col[8] = 0.0;
}

/* the reduction to the offsets, one entry at a time so that the device can spread the entries over lanes; D [9][8] by rows, T = (sum s s^T) D [9][8] */
inline double form_T(const double* ss, const double* D, int k, int j) {
    HNET_ALIGN_NO_CONTRACT
    double t = 0.0;
    for (int l = 0; l < NH; l++) t += sym_at(ss, k, l) * D[l * NX + j];
    return t;
}
/* entry (i, j), i <= j, of A = D^T T; the caller mirrors it, so that A is exactly symmetric */
inline double form_A(const double* D, const double* T, int i, int j) {
    HNET_ALIGN_NO_CONTRACT
    double a = 0.0;
    for (int k = 0; k < NH; k++) a += D[k * NX + i] * T[k * NX + j];
    return a;
}
inline double form_g(const double* D, const double* sr, int i) {
    HNET_ALIGN_NO_CONTRACT
    double a = 0.0;
    for (int k = 0; k < NH; k++) a += D[k * NX + i] * sr[k];
    return a;
}

/* Cholesky of M = A + lambda diag(A) (lower triangle into L [8][8]); false when a pivot is <= tiny or not finite */
inline bool cholesky(const double* A, double lambda, double tiny, double* L) {
    HNET_ALIGN_NO_CONTRACT
    for (int j = 0; j < NX; j++) {
        double d = A[j * NX + j] + lambda * A[j * NX + j];
        for (int k = 0; k < j; k++) d -= L[j * NX + k] * L[j * NX + k];
        if (!(d > tiny) || !std::isfinite(d)) return false;
        const double ljj = std::sqrt(d);
        L[j * NX + j] = ljj;
        for (int i = j + 1; i < NX; i++) {
            double s = A[i * NX + j];
            for (int k = 0; k < j; k++) s -= L[i * NX + k] * L[j * NX + k];
            L[i * NX + j] = s / ljj;
        }
    }
    return true;
}

/* The Levenberg-Marquardt step from (A, g) at damping lambda: dx = -(A + lambda diag(A))^-1 g.  false = SINGULAR: a pivot of A ITSELF is
 * <= 1e-12 max diag(A) or not finite.  The test is made on the undamped matrix because the damped one hides what the flag is for: adding
 * lambda diag(A) makes every matrix with a positive diagonal positive definite, and a pair that leaves some combination of the offsets free
 * (a constant image: A = 0; stripes: rank 5) has to stop instead of drifting along it.  L: 64 doubles of scratch. */
inline bool solve_damped(const double* A, const double* g, double lambda, double* L, double dx[NX]) {
    HNET_ALIGN_NO_CONTRACT
    double top = 0.0;
    for (int i = 0; i < NX; i++) top = A[i * NX + i] > top ? A[i * NX + i] : top;
    const double tiny = 1e-12 * top;
    if (!std::isfinite(tiny) || !cholesky(A, 0.0, tiny, L)) return false;
    if (!cholesky(A, lambda, tiny, L)) return false;
    for (int i = 0; i < NX; i++) {                       /* L y = -g, y in dx */
        double s = -g[i];
        for (int k = 0; k < i; k++) s -= L[i * NX + k] * dx[k];
        dx[i] = s / L[i * NX + i];
    }
    for (int i = NX - 1; i >= 0; i--) {                  /* L^T dx = y, in place */
        double s = dx[i];
        for (int k = i + 1; k < NX; k++) s -= L[k * NX + i] * dx[k];
        dx[i] = s / L[i * NX + i];
    }
    bool ok = true;
    for (int i = 0; i < NX; i++) ok = ok && std::isfinite(dx[i]);
    return ok;
}

/* One step of a pair, after linearisation number `it` (0: at the start offsets x0; it >= 1: at the trial offsets w.x_trial the step before proposed).
 * degenerate: the linearised point has no homography; n_valid, rr: its count and sum r^2; A [64], g [8]: its information matrix and gradient.
 *   it == 0: the record is initialised.  DEGENERATE / FEW_PIXELS return the start offsets with a zero information matrix.
 *   it >= 1: the trial is ACCEPTED iff it has a homography, n_valid >= max(min_valid, 9) and a strictly smaller mse: it becomes the current point and
 *            lambda *= 0.1; an accepted step with max |dx| < eps_px is CONVERGED.  Otherwise lambda *= 10 and the current point stays.
 * Then, unless the pair has stopped, the next step is solved from the current point (SINGULAR: the pair stops where it is) and the next trial offsets
 * are x_trial = (float)(offsets + dx).  The solve is also made after the last linearisation of a call (it == max_iterations), where no trial follows and
 * nothing reads x_trial / dx again: its only effect is the flag, so SINGULAR may appear on the point reached after max_iterations trials, and a
 * call with max_iterations = 0 still says whether the pair constrains the offsets.
 * A pair whose flags are non-zero has stopped: the caller makes no further step for it.  L: 64 doubles of scratch. */
inline void step(Record& rec, Work& w, int it, const Opts& o, const float* x0, bool degenerate, int n_valid, double rr, const double* A, const double* g,
                 double* L) {
    HNET_ALIGN_NO_CONTRACT
    const int need = o.min_valid > 9 ? o.min_valid : 9;
    const double mse = n_valid > 0 ? rr / (double)n_valid : 0.0;
    if (it == 0) {
        for (int k = 0; k < NX; k++) { rec.offsets_px[k] = x0[k]; rec.grad[k] = 0.0; w.dx[k] = 0.0; w.x_trial[k] = x0[k]; }
        for (int k = 0; k < NX * NX; k++) rec.info[k] = 0.0;
        rec.mse0 = rec.mse = 0.0;
        rec.n_valid0 = rec.n_valid = degenerate ? 0 : n_valid;
        rec.trials = rec.accepted = rec.flags = rec.pad = 0;
        rec.lambda = o.lambda0;
        if (degenerate) { rec.flags = DEGENERATE; return; }
        if (n_valid < need) { rec.flags = FEW_PIXELS; return; }
        rec.mse0 = rec.mse = mse;
        for (int k = 0; k < NX; k++) rec.grad[k] = g[k];
        for (int k = 0; k < NX * NX; k++) rec.info[k] = A[k];
    } else {
        rec.trials++;
        if (!degenerate && n_valid >= need && mse < rec.mse) {
            rec.accepted++;
            rec.lambda *= 0.1;
            rec.mse = mse;
            rec.n_valid = n_valid;
            double top = 0.0;
            for (int k = 0; k < NX; k++) {
                rec.offsets_px[k] = w.x_trial[k];
                rec.grad[k] = g[k];
                const double a = std::fabs(w.dx[k]);
                top = a > top ? a : top;
            }
            for (int k = 0; k < NX * NX; k++) rec.info[k] = A[k];
            if (top < o.eps_px) { rec.flags |= CONVERGED; return; }
        } else {
            rec.lambda *= 10.0;
        }
    }
    if (!solve_damped(rec.info, rec.grad, rec.lambda, L, w.dx)) { rec.flags |= SINGULAR; return; }
    for (int k = 0; k < NX; k++) w.x_trial[k] = (float)((double)rec.offsets_px[k] + w.dx[k]);
}

}  /* namespace hnet_align */

#endif /* HNET_PHOTO_ALIGN_H */
