// photo_align_ref.cpp — the host reference of photometric alignment (include/hnet.h hnet_photo_align): the quantity of include/hnet_photo_align.h
// restated on photo_ref.cpp's fp32 sampler (homography, coords, unit), summed in double in ascending pixel order, reduced to the offsets and stepped by the
// very functions the device compiles (hnet_align::dlt_jacobian_col, form_T / form_A / form_g, step).
// Build as photo_ref.cpp is built (nothing may be contracted):
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/photo_align_ref.cpp
// A float64 twin of the per-pixel quantity (H unrounded, positions X / Z) serves the derivative test: central differences of a cost need a cost whose
// rounding noise is far below the step.
#include "photo_ref.cpp"

#include "hnet_photo_align.h"

namespace photo_align_ref {

namespace pa = hnet_align;
using photo_ref::IMG_H;
using photo_ref::IMG_W;
using photo_ref::NPIX;

// residual r and row s of pixel (u, v) under H in fp32, exactly the device's operations (photo_align_accum_kernel, csrc/kernels_photo_align.hip); false: not valid
inline bool pixel(const uint8_t* img1, const uint8_t* img2, const float* h, int u, int v, float& r, float s[9]) {
    float ix, iy;
    photo_ref::coords(h, u, v, ix, iy);
    if (!(ix >= 0.0f && ix < (float)(IMG_W - 1) && iy >= 0.0f && iy < (float)(IMG_H - 1))) return false;
    const float fu = (float)u, fv = (float)v;
    const float Z = fmaf(h[6], fu, fmaf(h[7], fv, h[8]));
    const float x0f = floorf(ix), y0f = floorf(iy);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float wx1 = ix - x0f, wx0 = 1.0f - wx1, wy1 = iy - y0f, wy0 = 1.0f - wy1;
    const uint8_t* p = img2 + y0 * IMG_W + x0;
    const float a = photo_ref::unit(p[0]), b = photo_ref::unit(p[1]), c = photo_ref::unit(p[IMG_W]), d = photo_ref::unit(p[IMG_W + 1]);
    float w = fmaf(a, wx0 * wy0, 0.0f);
    w = fmaf(b, wx1 * wy0, w);
    w = fmaf(c, wx0 * wy1, w);
    w = fmaf(d, wx1 * wy1, w);
    r = (w - photo_ref::unit(img1[v * IMG_W + u])) * 255.0f;
    const float gx = fmaf(d - c, wy1, (b - a) * wy0) * 255.0f;
    const float gy = fmaf(d - b, wx1, (c - a) * wx0) * 255.0f;
    const float q = fmaf(gx, ix, gy * iy);
    const float rz = 1.0f / Z, au = fu * rz, av = fv * rz;
    s[0] = gx * au; s[1] = gx * av; s[2] = gx * rz;
    s[3] = gy * au; s[4] = gy * av; s[5] = gy * rz;
    s[6] = -q * au; s[7] = -q * av; s[8] = -q * rz;
    return true;
}

// the same quantity in float64 for H in double (the derivative test's twin)
inline bool pixel64(const uint8_t* img1, const uint8_t* img2, const double* h, int u, int v, double& r, double s[9]) {
    const double Z = h[6] * u + h[7] * v + h[8], ix = (h[0] * u + h[1] * v + h[2]) / Z, iy = (h[3] * u + h[4] * v + h[5]) / Z;
    if (!(ix >= 0.0 && ix < (double)(IMG_W - 1) && iy >= 0.0 && iy < (double)(IMG_H - 1))) return false;
    const int x0 = (int)floor(ix), y0 = (int)floor(iy);
    const double fx = ix - x0, fy = iy - y0;
    const uint8_t* p = img2 + y0 * IMG_W + x0;
    const double a = p[0], b = p[1], c = p[IMG_W], d = p[IMG_W + 1];
    r = (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy - (double)img1[v * IMG_W + u];
    const double gx = (b - a) * (1 - fy) + (d - c) * fy, gy = (c - a) * (1 - fx) + (d - b) * fx, q = gx * ix + gy * iy;
    s[0] = gx * u / Z; s[1] = gx * v / Z; s[2] = gx / Z;
    s[3] = gy * u / Z; s[4] = gy * v / Z; s[5] = gy / Z;
    s[6] = -q * u / Z; s[7] = -q * v / Z; s[8] = -q / Z;
    return true;
}

template <typename T>
inline void add_pixel(pa::Sums& m, T r, const T* s) {
    for (int i = 0; i < pa::NH; i++) {
        for (int j = i; j < pa::NH; j++) m.ss[pa::sym_index(i, j)] += (double)s[i] * (double)s[j];
        m.sr[i] += (double)s[i] * (double)r;
    }
    m.rr += (double)r * (double)r;
    m.n_valid++;
}

// one linearisation at fp32 offsets; returns false (and zero sums) when there is no homography
inline bool linearise(const uint8_t* img1, const uint8_t* img2, const float* off, pa::Sums& m) {
    m = pa::Sums{};
    float h[9];
    if (!photo_ref::homography(off, h)) return false;
    for (int v = 0; v < IMG_H; v++)
        for (int u = 0; u < IMG_W; u++) {
            float r, s[9];
            if (pixel(img1, img2, h, u, v, r, s)) add_pixel(m, r, s);
        }
    return true;
}

inline void corners(const float* off, double dst[8]) {
    for (int k = 0; k < 8; k++) dst[k] = pa::corner(hnet::p4(k), off[k]);
}

// A [64] and g [8] of H-space sums at the corners dst, in the order the device forms them: D by columns, T, the upper triangle of A mirrored, g
inline void reduce(const double dst[8], const pa::Sums& m, double* A, double* g) {
    double D[pa::NH * pa::NX], T[pa::NH * pa::NX], col[pa::NH];
    for (int k = 0; k < pa::NX; k++) {
        pa::dlt_jacobian_col(dst, k, col);
        for (int i = 0; i < pa::NH; i++) D[i * pa::NX + k] = col[i];
    }
    for (int k = 0; k < pa::NH; k++)
        for (int j = 0; j < pa::NX; j++) T[k * pa::NX + j] = pa::form_T(m.ss, D, k, j);
    for (int i = 0; i < pa::NX; i++) {
        for (int j = i; j < pa::NX; j++) A[i * pa::NX + j] = A[j * pa::NX + i] = pa::form_A(D, T, i, j);
        g[i] = pa::form_g(D, m.sr, i);
    }
}

// the whole alignment of one pair: max_iterations + 1 linearisations at the most, as the device's launch sequence
inline void align(const uint8_t* img1, const uint8_t* img2, const float* x0, const pa::Opts& o, pa::Record& rec) {
    pa::Work w;
    double A[64], g[8], L[64], dst[8];
    for (int it = 0; it <= o.max_iterations; it++) {
        if (it > 0 && rec.flags) break;
        const float* x = it == 0 ? x0 : w.x_trial;
        pa::Sums m;
        const bool ok = linearise(img1, img2, x, m);
        corners(x, dst);
        reduce(dst, m, A, g);
        pa::step(rec, w, it, o, x0, !ok, m.n_valid, m.rr, A, g, L);
    }
}

}  // namespace photo_align_ref

extern "C" {

// H-space sums [n] (pa::Sums, 448 bytes each) and has-a-homography flags [n] at offsets [n][8]
void photo_align_ref_sums(const uint8_t* img1, const uint8_t* img2, int n, const float* offsets, void* sums, int32_t* ok) {
    static_assert(sizeof(photo_align_ref::pa::Sums) == 448, "45 + 9 + 1 doubles, the count and a pad");
    for (int b = 0; b < n; b++)
        ok[b] = photo_align_ref::linearise(img1 + (size_t)b * photo_ref::NPIX, img2 + (size_t)b * photo_ref::NPIX, offsets + b * 8,
                                           static_cast<photo_align_ref::pa::Sums*>(sums)[b]);
}

// A [n][64], g [n][8] of those sums at the same offsets
void photo_align_ref_reduce(int n, const float* offsets, const void* sums, double* A, double* g) {
    for (int b = 0; b < n; b++) {
        double dst[8];
        photo_align_ref::corners(offsets + b * 8, dst);
        photo_align_ref::reduce(dst, static_cast<const photo_align_ref::pa::Sums*>(sums)[b], A + b * 64, g + b * 8);
    }
}

// records [n] (hnet_photo_align, 656 bytes each) of the alignment from offsets0 [n][8]
void photo_align_ref_run(const uint8_t* img1, const uint8_t* img2, int n, const float* offsets0, const void* opts, void* out) {
    static_assert(sizeof(photo_align_ref::pa::Record) == 656, "the record layout of hnet_photo_align");
    for (int b = 0; b < n; b++)
        photo_align_ref::align(img1 + (size_t)b * photo_ref::NPIX, img2 + (size_t)b * photo_ref::NPIX, offsets0 + b * 8,
                               *static_cast<const photo_align_ref::pa::Opts*>(opts), static_cast<photo_align_ref::pa::Record*>(out)[b]);
}

// n_edge [n]: the pixels whose ix lies within 1e-3 px of 0 or 319 or whose iy lies within 1e-3 px of 0 or 223, the bounds of VALID, at offsets [n][8]: the
// count by which a device whose positions differ in the last bits may differ in n_valid (the residual reference's n_edge for this quantity's bounds).
// The frames take no part in it; they are in the signature so that it is called like photo_align_ref_sums.  0 where there is no homography.
void photo_align_ref_edge(const uint8_t*, const uint8_t*, int n, const float* offsets, int32_t* n_edge) {
    for (int b = 0; b < n; b++) {
        float h[9];
        n_edge[b] = 0;
        if (!photo_ref::homography(offsets + b * 8, h)) continue;
        for (int v = 0; v < photo_ref::IMG_H; v++)
            for (int u = 0; u < photo_ref::IMG_W; u++) {
                float ix, iy;
                photo_ref::coords(h, u, v, ix, iy);
                const bool ex = fabsf(ix) < 1e-3f || fabsf(ix - (float)(photo_ref::IMG_W - 1)) < 1e-3f;
                const bool ey = fabsf(iy) < 1e-3f || fabsf(iy - (float)(photo_ref::IMG_H - 1)) < 1e-3f;
                if (ex || ey) n_edge[b]++;
            }
    }
}

// whether the options are ones a call accepts (hnet_align::opts_valid: the C API answers HNET_ERR_INVALID_ARG otherwise)
int photo_align_ref_opts_valid(const void* opts) { return photo_align_ref::pa::opts_valid(*static_cast<const photo_align_ref::pa::Opts*>(opts)) ? 1 : 0; }

// csrc/geom.h's dlt_solve and its analytic Jacobian D [9][8] at the corners dst [8]
void photo_align_ref_dlt(const double* dst, double* H, double* D) {
    hnet::dlt_solve(dst, H);
    double col[9];
    for (int k = 0; k < 8; k++) {
        photo_align_ref::pa::dlt_jacobian_col(dst, k, col);
        for (int i = 0; i < 9; i++) D[i * 8 + k] = col[i];
    }
}

// the float64 twin at offsets in double: cost = sum r^2 / 2, its gradient g [8] through the same D and reduction, and the valid count
void photo_align_ref_cost64(const uint8_t* img1, const uint8_t* img2, const double* offsets, double* cost, double* g, int32_t* n_valid) {
    double dst[8], h[9], A[64];
    for (int k = 0; k < 8; k++) dst[k] = hnet::p4(k) + offsets[k];
    hnet::dlt_solve(dst, h);
    photo_align_ref::pa::Sums m{};
    for (int v = 0; v < photo_ref::IMG_H; v++)
        for (int u = 0; u < photo_ref::IMG_W; u++) {
            double r, s[9];
            if (photo_align_ref::pixel64(img1, img2, h, u, v, r, s)) photo_align_ref::add_pixel(m, r, s);
        }
    photo_align_ref::reduce(dst, m, A, g);
    *cost = 0.5 * m.rr;
    *n_valid = m.n_valid;
}

}  // extern "C"
