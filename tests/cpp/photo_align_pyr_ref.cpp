// photo_align_pyr_ref.cpp — the host reference of coarse-to-fine photometric alignment (include/hnet.h hnet_op_photo_align_pyramid): the pyramid,
// the per-level quantity of include/hnet_photo_pyramid.h summed in double in ascending pixel order, and the loop over levels, on photo_align_ref.cpp's
// reduction and the very step function the device compiles.  Built as photo_align_ref.cpp is built (nothing may be contracted):
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/photo_align_pyr_ref.cpp
// Level 0 of this file is photo_align_ref::pixel's quantity bit for bit (every added operation is x 1 or - 0): tests/test_photo_align_pyr_cpu.py pins it.
#include "photo_align_ref.cpp"

#include "hnet_photo_pyramid.h"

namespace photo_align_pyr_ref {

namespace pa = hnet_align;

// levels 0 .. 3 of one frame; level 0 is the caller's
struct Pyramid {
    const uint8_t* lv[pa::MAX_LEVELS];
    uint8_t store[pa::PYR_BYTES];
    explicit Pyramid(const uint8_t* img) {
        lv[0] = img;
        for (int L = 1; L < pa::MAX_LEVELS; L++) {
            uint8_t* dst = store + pa::level_offset(L);
            pa::downsample(lv[L - 1], pa::level_w(L - 1), pa::level_h(L - 1), dst);
            lv[L] = dst;
        }
    }
};

struct IeeeDiv {
    void operator()(float X, float Y, float Z, float& qx, float& qy) const { qx = X / Z; qy = Y / Z; }
};

// residual and row of level-L pixel (u, v) under H; false: not valid
inline bool pixel(int L, const uint8_t* img1, const uint8_t* img2, const float* h, int u, int v, float& r, float s[9]) {
    const int W = pa::level_w(L);
    const float fu = pa::level_centre(L, u), fv = pa::level_centre(L, v);
    float ix0, iy0, Z, ix, iy;
    pa::level_coords(h, fu, fv, IeeeDiv{}, ix0, iy0, Z);
    if (!pa::level_position(L, ix0, iy0, ix, iy)) return false;
    const uint8_t* p = img2 + (int)floorf(iy) * W + (int)floorf(ix);
    pa::level_row(L, photo_ref::unit(p[0]), photo_ref::unit(p[1]), photo_ref::unit(p[W]), photo_ref::unit(p[W + 1]), photo_ref::unit(img1[v * W + u]), ix, iy,
                  ix0, iy0, Z, fu, fv, r, s);
    return true;
}

// one linearisation of level L at fp32 offsets (full-resolution pixels); false (and zero sums) when there is no homography
inline bool linearise(int L, const uint8_t* img1, const uint8_t* img2, const float* off, pa::Sums& m) {
    m = pa::Sums{};
    float h[9];
    if (!photo_ref::homography(off, h)) return false;
    for (int v = 0; v < pa::level_h(L); v++)
        for (int u = 0; u < pa::level_w(L); u++) {
            float r, s[9];
            if (pixel(L, img1, img2, h, u, v, r, s)) photo_align_ref::add_pixel(m, r, s);
        }
    return true;
}

// one complete alignment at level L (photo_align_ref::align on the level's images)
inline void align_level(int L, const uint8_t* img1, const uint8_t* img2, const float* x0, const pa::Opts& o, pa::Record& rec) {
    pa::Work w;
    double A[64], g[8], Lc[64], dst[8];
    for (int it = 0; it <= o.max_iterations; it++) {
        if (it > 0 && rec.flags) break;
        const float* x = it == 0 ? x0 : w.x_trial;
        pa::Sums m;
        const bool ok = linearise(L, img1, img2, x, m);
        photo_align_ref::corners(x, dst);
        photo_align_ref::reduce(dst, m, A, g);
        pa::step(rec, w, it, o, x0, !ok, m.n_valid, m.rr, A, g, Lc);
    }
}

// levels - 1 down to 0; recs [levels], index = level.  A level starts where the level above ended, whatever its flags.
inline void align(const uint8_t* img1, const uint8_t* img2, const float* x0, const pa::Opts& o, int levels, pa::Record* recs) {
    const Pyramid p1(img1), p2(img2);
    float start[8];
    for (int k = 0; k < 8; k++) start[k] = x0[k];
    for (int L = levels - 1; L >= 0; L--) {
        pa::Opts ol = o;
        ol.min_valid = pa::level_min_valid(o.min_valid, L);
        align_level(L, p1.lv[L], p2.lv[L], start, ol, recs[L]);
        memcpy(start, recs[L].offsets_px, sizeof start);           // (bits: a NaN start keeps its payload)
    }
}

// the float64 twin of a level's quantity for H in double (the derivative test)
inline bool pixel64(int L, const uint8_t* img1, const uint8_t* img2, const double* h, int u, int v, double& r, double s[9]) {
    const int W = pa::level_w(L), H = pa::level_h(L);
    const double sc = (double)(1 << L), c = (sc - 1.0) * 0.5, fu = sc * u + c, fv = sc * v + c;
    const double Z = h[6] * fu + h[7] * fv + h[8], ix0 = (h[0] * fu + h[1] * fv + h[2]) / Z, iy0 = (h[3] * fu + h[4] * fv + h[5]) / Z;
    const double ix = (ix0 - c) / sc, iy = (iy0 - c) / sc;
    if (!(ix >= 0.0 && ix < (double)(W - 1) && iy >= 0.0 && iy < (double)(H - 1))) return false;
    const int x0 = (int)floor(ix), y0 = (int)floor(iy);
    const double fx = ix - x0, fy = iy - y0;
    const uint8_t* p = img2 + y0 * W + x0;
    const double a = p[0], b = p[1], cc = p[W], d = p[W + 1];
    r = (a * (1 - fx) + b * fx) * (1 - fy) + (cc * (1 - fx) + d * fx) * fy - (double)img1[v * W + u];
    const double gx = ((b - a) * (1 - fy) + (d - cc) * fy) / sc, gy = ((cc - a) * (1 - fx) + (d - b) * fx) / sc, q = gx * ix0 + gy * iy0;
    s[0] = gx * fu / Z; s[1] = gx * fv / Z; s[2] = gx / Z;
    s[3] = gy * fu / Z; s[4] = gy * fv / Z; s[5] = gy / Z;
    s[6] = -q * fu / Z; s[7] = -q * fv / Z; s[8] = -q / Z;
    return true;
}

}  // namespace photo_align_pyr_ref

extern "C" {

// levels 1 .. 3 of n frames: out [n][PYR_BYTES]
void photo_align_pyr_ref_pyramid(const uint8_t* img, int n, uint8_t* out) {
    for (int b = 0; b < n; b++) {
        const photo_align_pyr_ref::Pyramid p(img + (size_t)b * photo_ref::NPIX);
        memcpy(out + (size_t)b * hnet_align::PYR_BYTES, p.store, hnet_align::PYR_BYTES);
    }
}

// H-space sums [n] and has-a-homography flags [n] of level L at offsets [n][8], on full-resolution frames
void photo_align_pyr_ref_sums(const uint8_t* img1, const uint8_t* img2, int n, const float* offsets, int level, void* sums, int32_t* ok) {
    for (int b = 0; b < n; b++) {
        const photo_align_pyr_ref::Pyramid p1(img1 + (size_t)b * photo_ref::NPIX), p2(img2 + (size_t)b * photo_ref::NPIX);
        ok[b] = photo_align_pyr_ref::linearise(level, p1.lv[level], p2.lv[level], offsets + b * 8, static_cast<hnet_align::Sums*>(sums)[b]);
    }
}

// records out [n] (level 0) and levels_out [n][levels] (index = level; may be null) of the coarse-to-fine alignment from offsets0 [n][8]
void photo_align_pyr_ref_run(const uint8_t* img1, const uint8_t* img2, int n, const float* offsets0, const void* opts, int levels, void* out, void* levels_out) {
    for (int b = 0; b < n; b++) {
        hnet_align::Record recs[hnet_align::MAX_LEVELS];
        photo_align_pyr_ref::align(img1 + (size_t)b * photo_ref::NPIX, img2 + (size_t)b * photo_ref::NPIX, offsets0 + b * 8,
                                   *static_cast<const hnet_align::Opts*>(opts), levels, recs);
        static_cast<hnet_align::Record*>(out)[b] = recs[0];
        if (levels_out)
            for (int L = 0; L < levels; L++) static_cast<hnet_align::Record*>(levels_out)[(size_t)b * levels + L] = recs[L];
    }
}

// the float64 twin of level L at offsets in double: cost = sum r^2 / 2, its gradient g [8] through the same D and reduction, and the valid count
void photo_align_pyr_ref_cost64(const uint8_t* img1, const uint8_t* img2, const double* offsets, int level, double* cost, double* g, int32_t* n_valid) {
    const photo_align_pyr_ref::Pyramid p1(img1), p2(img2);
    double dst[8], h[9], A[64];
    for (int k = 0; k < 8; k++) dst[k] = hnet::p4(k) + offsets[k];
    hnet::dlt_solve(dst, h);
    hnet_align::Sums m{};
    for (int v = 0; v < hnet_align::level_h(level); v++)
        for (int u = 0; u < hnet_align::level_w(level); u++) {
            double r, s[9];
            if (photo_align_pyr_ref::pixel64(level, p1.lv[level], p2.lv[level], h, u, v, r, s)) photo_align_ref::add_pixel(m, r, s);
        }
    photo_align_ref::reduce(dst, m, A, g);
    *cost = 0.5 * m.rr;
    *n_valid = m.n_valid;
}

}  // extern "C"
