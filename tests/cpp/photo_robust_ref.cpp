// photo_robust_ref.cpp — the host reference of photometric alignment with a gain / bias model and Huber weights (include/hnet.h hnet_op_photo_align_robust;
// DESIGN 7n): the quantity of include/hnet_photo_robust.h summed in double in ascending pixel order through the very functions the device compiles
// (level_coords / level_position / level_row, sample, residual, weighted_row), the reduction to the ten parameters (form_T / form_A / form_A10 / form_g10),
// hnet_robust::step, and the loop over levels of photo_align_pyr_ref.cpp.  Built as that file is built (nothing may be contracted):
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/photo_robust_ref.cpp
// A float64 twin of the cost (H unrounded, gain and bias in double) serves the derivative test.
#include "photo_align_pyr_ref.cpp"

#include "hnet_photo_robust.h"

namespace photo_robust_ref {

namespace pa = hnet_align;
namespace pr = hnet_robust;
using photo_align_pyr_ref::IeeeDiv;
using photo_align_pyr_ref::Pyramid;

inline void add_pixel(pr::Sums& m, float r, const float* t, const float* tw, double rho, bool outlier) {
    for (int i = 0; i < pr::NT; i++) {
        for (int j = i; j < pr::NT; j++) m.tt[pr::sym_index(i, j)] += (double)tw[i] * (double)t[j];
        m.tr[i] += (double)tw[i] * (double)r;
    }
    m.rho += rho;
    m.n_valid++;
    m.n_outliers += outlier ? 1 : 0;
}

// one linearisation of level L at fp32 offsets, gain G and bias b; false (and zero sums) when there is no homography
inline bool linearise(int L, const uint8_t* img1, const uint8_t* img2, const float* off, double G, double b, double k, pr::Sums& m) {
    m = pr::Sums{};
    float h[9];
    if (!photo_ref::homography(off, h)) return false;
    const int W = pa::level_w(L);
    const float Gf = pr::gain_f(G), bf = pr::bias_f(b), kf = pr::huber_f(k);
    for (int v = 0; v < pa::level_h(L); v++)
        for (int u = 0; u < W; u++) {
            const float fu = pa::level_centre(L, u), fv = pa::level_centre(L, v);
            float ix0, iy0, Z, ix, iy;
            pa::level_coords(h, fu, fv, IeeeDiv{}, ix0, iy0, Z);
            if (!pa::level_position(L, ix0, iy0, ix, iy)) continue;
            const uint8_t* p = img2 + (int)floorf(iy) * W + (int)floorf(ix);
            const float a = photo_ref::unit(p[0]), bb = photo_ref::unit(p[1]), c = photo_ref::unit(p[W]), d = photo_ref::unit(p[W + 1]);
            const float i1 = photo_ref::unit(img1[v * W + u]);
            float r0, s[9], r, omega, t[pr::NT], tw[pr::NT];
            double rho;
            pa::level_row(L, a, bb, c, d, i1, ix, iy, ix0, iy0, Z, fu, fv, r0, s);
            const float w = pr::sample(a, bb, c, d, ix, iy);
            const bool outlier = pr::residual(Gf, bf, kf, w, i1, r, omega, rho);
            pr::weighted_row(s, w, omega, t, tw);
            add_pixel(m, r, t, tw, rho, outlier);
        }
    return true;
}

// A10 [100] and g10 [10] of the sums at the corners dst and gain G, in the order the device forms them
inline void reduce(const double dst[8], const pr::Sums& m, double G, double* A, double* g) {
    double D[pa::NH * pa::NX], T[pa::NH * pa::NX], ss[pa::NSYM], col[pa::NH];
    for (int k = 0; k < pa::NX; k++) {
        pa::dlt_jacobian_col(dst, k, col);
        for (int i = 0; i < pa::NH; i++) D[i * pa::NX + k] = col[i];
    }
    for (int e = 0; e < pa::NSYM; e++) ss[e] = pr::ss_entry(m.tt, e);
    for (int k = 0; k < pa::NH; k++)
        for (int j = 0; j < pa::NX; j++) T[k * pa::NX + j] = pa::form_T(ss, D, k, j);
    for (int i = 0; i < pr::NP; i++) {
        for (int j = i; j < pr::NP; j++) A[i * pr::NP + j] = A[j * pr::NP + i] = pr::form_A10(D, m.tt, G, j < pa::NX ? pa::form_A(D, T, i, j) : 0.0, i, j);
        g[i] = pr::form_g10(D, m.tr, G, i);
    }
}

// one complete alignment at level L from st
inline void align_level(int L, const uint8_t* img1, const uint8_t* img2, const pr::Start& st, const pr::Opts& o, pr::Record& rec) {
    pr::Work w;
    double A[100], g[10], Lc[100], dst[8];
    for (int it = 0; it <= o.base.max_iterations; it++) {
        if (it > 0 && rec.px.flags) break;
        const float* x = it == 0 ? st.x : w.x_trial;
        const double G = it == 0 ? st.gain : w.gain_trial, b = it == 0 ? st.bias : w.bias_trial;
        pr::Sums m;
        const bool ok = linearise(L, img1, img2, x, G, b, o.huber_k, m);
        photo_align_ref::corners(x, dst);
        reduce(dst, m, G, A, g);
        pr::step(rec, w, it, o, st, !ok, m.n_valid, m.n_outliers, m.rho, A, g, Lc);
    }
}

// levels - 1 down to 0; recs [levels], index = level.  A level starts where the level above ended (offsets, gain, bias), whatever its flags.
inline void align(const uint8_t* img1, const uint8_t* img2, const float* x0, const pr::Opts& o, int levels, pr::Record* recs) {
    const Pyramid p1(img1), p2(img2);
    pr::Start st;
    memcpy(st.x, x0, sizeof st.x);
    st.gain = o.gain0;
    st.bias = o.bias0;
    for (int L = levels - 1; L >= 0; L--) {
        pr::Opts ol = o;
        ol.base.min_valid = pa::level_min_valid(o.base.min_valid, L);
        align_level(L, p1.lv[L], p2.lv[L], st, ol, recs[L]);
        memcpy(st.x, recs[L].px.offsets_px, sizeof st.x);          // (bits: a NaN keeps its payload)
        memcpy(&st.gain, &recs[L].gain, 16);
    }
}

}  // namespace photo_robust_ref

extern "C" {

// sums [n] (hnet_robust::Sums, 632 bytes each) and has-a-homography flags [n] of level L at offsets [n][8], gain [n], bias [n] and Huber threshold k
void photo_robust_ref_sums(const uint8_t* img1, const uint8_t* img2, int n, const float* offsets, const double* gain, const double* bias, double k, int level,
                           void* sums, int32_t* ok) {
    static_assert(sizeof(hnet_robust::Sums) == 632 && sizeof(hnet_robust::Record) == 1560 && sizeof(hnet_robust::Opts) == 56, "the layouts of include/hnet.h");
    for (int b = 0; b < n; b++) {
        const photo_robust_ref::Pyramid p1(img1 + (size_t)b * photo_ref::NPIX), p2(img2 + (size_t)b * photo_ref::NPIX);
        ok[b] = photo_robust_ref::linearise(level, p1.lv[level], p2.lv[level], offsets + b * 8, gain[b], bias[b], k, static_cast<hnet_robust::Sums*>(sums)[b]);
    }
}

// A10 [n][100], g10 [n][10] of those sums at the same offsets and gains
void photo_robust_ref_reduce(int n, const float* offsets, const double* gain, const void* sums, double* A, double* g) {
    for (int b = 0; b < n; b++) {
        double dst[8];
        photo_align_ref::corners(offsets + b * 8, dst);
        photo_robust_ref::reduce(dst, static_cast<const hnet_robust::Sums*>(sums)[b], gain[b], A + b * 100, g + b * 10);
    }
}

// records out [n] (level 0) and levels_out [n][levels] (index = level; may be null) from offsets0 [n][8]
void photo_robust_ref_run(const uint8_t* img1, const uint8_t* img2, int n, const float* offsets0, const void* opts, int levels, void* out, void* levels_out) {
    for (int b = 0; b < n; b++) {
        hnet_robust::Record recs[hnet_align::MAX_LEVELS];
        photo_robust_ref::align(img1 + (size_t)b * photo_ref::NPIX, img2 + (size_t)b * photo_ref::NPIX, offsets0 + b * 8,
                                *static_cast<const hnet_robust::Opts*>(opts), levels, recs);
        static_cast<hnet_robust::Record*>(out)[b] = recs[0];
        if (levels_out)
            for (int L = 0; L < levels; L++) static_cast<hnet_robust::Record*>(levels_out)[(size_t)b * levels + L] = recs[L];
    }
}

int photo_robust_ref_opts_valid(const void* opts) { return hnet_robust::opts_valid(*static_cast<const hnet_robust::Opts*>(opts)) ? 1 : 0; }

// the float64 twin of level L at p = (offsets [8], gain, bias) in double: cost = sum rho / 2, its gradient g [10] through the same D, the valid count, the
// outlier count and the smallest distance of an |r| from k (how far the nearest pixel is from changing sides)
void photo_robust_ref_cost64(const uint8_t* img1, const uint8_t* img2, const double* p, double k, int level, double* cost, double* g, int32_t* n_valid,
                             int32_t* n_outliers, double* k_margin) {
    const photo_robust_ref::Pyramid p1(img1), p2(img2);
    const int W = hnet_align::level_w(level);
    const double G = p[8], b = p[9];
    double dst[8], h[9], sr[9] = {0}, cr[2] = {0, 0}, rho = 0.0, margin = INFINITY;
    for (int i = 0; i < 8; i++) dst[i] = hnet::p4(i) + p[i];
    hnet::dlt_solve(dst, h);
    int nv = 0, no = 0;
    for (int v = 0; v < hnet_align::level_h(level); v++)
        for (int u = 0; u < W; u++) {
            double r0, s[9];
            if (!photo_align_pyr_ref::pixel64(level, p1.lv[level], p2.lv[level], h, u, v, r0, s)) continue;
            const double i1 = (double)p1.lv[level][v * W + u], w = r0 + i1, r = G * w + b - i1, ar = fabs(r);
            double omega = 1.0;
            if (k == 0.0 || ar <= k) {
                rho += r * r;
            } else {
                omega = k / ar;
                rho += k * (2.0 * ar - k);
                no++;
            }
            if (k > 0.0) margin = fmin(margin, fabs(ar - k));
            for (int i = 0; i < 9; i++) sr[i] += omega * s[i] * r;
            cr[0] += omega * w * r;
            cr[1] += omega * r;
            nv++;
        }
    double col[9], D[72];
    for (int j = 0; j < 8; j++) {
        hnet_align::dlt_jacobian_col(dst, j, col);
        for (int i = 0; i < 9; i++) D[i * 8 + j] = col[i];
    }
    for (int i = 0; i < 8; i++) g[i] = G * hnet_align::form_g(D, sr, i);
    g[8] = cr[0];
    g[9] = cr[1];
    *cost = 0.5 * rho;
    *n_valid = nv;
    *n_outliers = no;
    *k_margin = margin;
}

}  // extern "C"
