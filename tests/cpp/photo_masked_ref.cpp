// photo_masked_ref.cpp — the host reference of the robust photometric alignment on the template pixels a mask admits (include/hnet.h
// hnet_op_photo_align_masked; include/hnet_photo_masked.h): photo_robust_ref.cpp's linearisation with takes_part in front of every pixel, its
// reduce, hnet_robust::step and its loop over levels, on the mask pyramid of hnet_masked::mask_pyramid.  Built as that file is built:
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/photo_masked_ref.cpp
#include "photo_robust_ref.cpp"

#include "hnet_photo_masked.h"

namespace photo_masked_ref {

namespace pa = hnet_align;
namespace pr = hnet_robust;
namespace pm = hnet_masked;
using photo_align_pyr_ref::IeeeDiv;
using photo_align_pyr_ref::Pyramid;

// photo_robust_ref::linearise with one more condition in front; mask: level L of the mask
inline bool linearise(int L, const uint8_t* img1, const uint8_t* mask, const uint8_t* img2, const float* off, double G, double b, double k, pr::Sums& m) {
    m = pr::Sums{};
    float h[9];
    if (!photo_ref::homography(off, h)) return false;
    const int W = pa::level_w(L);
    const float Gf = pr::gain_f(G), bf = pr::bias_f(b), kf = pr::huber_f(k);
    for (int v = 0; v < pa::level_h(L); v++)
        for (int u = 0; u < W; u++) {
            if (!pm::takes_part(mask, L, u, v)) continue;
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
            photo_robust_ref::add_pixel(m, r, t, tw, rho, outlier);
        }
    return true;
}

// one complete alignment at level L from st (photo_robust_ref::align_level)
inline void align_level(int L, const uint8_t* img1, const uint8_t* mask, const uint8_t* img2, const pr::Start& st, const pr::Opts& o, pr::Record& rec) {
    pr::Work w;
    double A[100], g[10], Lc[100], dst[8];
    for (int it = 0; it <= o.base.max_iterations; it++) {
        if (it > 0 && rec.px.flags) break;
        const float* x = it == 0 ? st.x : w.x_trial;
        const double G = it == 0 ? st.gain : w.gain_trial, b = it == 0 ? st.bias : w.bias_trial;
        pr::Sums m;
        const bool ok = linearise(L, img1, mask, img2, x, G, b, o.huber_k, m);
        photo_align_ref::corners(x, dst);
        photo_robust_ref::reduce(dst, m, G, A, g);
        pr::step(rec, w, it, o, st, !ok, m.n_valid, m.n_outliers, m.rho, A, g, Lc);
    }
}

// levels - 1 down to 0; recs [levels], index = level (photo_robust_ref::align)
inline void align(const uint8_t* img1, const uint8_t* mask0, const uint8_t* img2, const float* x0, const pr::Opts& o, int levels, pr::Record* recs) {
    const Pyramid p1(img1), p2(img2);
    std::vector<uint8_t> mpyr(pa::PYR_BYTES);
    pm::mask_pyramid(mask0, mpyr.data());
    pr::Start st;
    memcpy(st.x, x0, sizeof st.x);
    st.gain = o.gain0;
    st.bias = o.bias0;
    for (int L = levels - 1; L >= 0; L--) {
        pr::Opts ol = o;
        ol.base.min_valid = pa::level_min_valid(o.base.min_valid, L);
        align_level(L, p1.lv[L], pm::mask_level(mask0, mpyr.data(), L), p2.lv[L], st, ol, recs[L]);
        memcpy(st.x, recs[L].px.offsets_px, sizeof st.x);          // (bits: a NaN keeps its payload)
        memcpy(&st.gain, &recs[L].gain, 16);
    }
}

}  // namespace photo_masked_ref

extern "C" {

// levels 1 .. 3 of n masks [n][71 680] -> pyr [n][PYR_BYTES] and the counts n_mask [n][4][7]
void photo_masked_ref_pyramid(const uint8_t* mask, int n, uint8_t* pyr, int32_t* n_mask) {
    for (int b = 0; b < n; b++) {
        const uint8_t* m0 = mask + (size_t)b * photo_ref::NPIX;
        uint8_t* p = pyr + (size_t)b * hnet_align::PYR_BYTES;
        hnet_masked::mask_pyramid(m0, p);
        hnet_masked::mask_counts(m0, p, n_mask + (size_t)b * hnet_masked::N_MASK);
    }
}

// photo_robust_ref_run with masks [n][71 680] beside img1
void photo_masked_ref_run(const uint8_t* img1, const uint8_t* mask, const uint8_t* img2, int n, const float* offsets0, const void* opts, int levels, void* out,
                          void* levels_out) {
    for (int b = 0; b < n; b++) {
        hnet_robust::Record recs[hnet_align::MAX_LEVELS];
        const size_t at = (size_t)b * photo_ref::NPIX;
        photo_masked_ref::align(img1 + at, mask + at, img2 + at, offsets0 + b * 8, *static_cast<const hnet_robust::Opts*>(opts), levels, recs);
        static_cast<hnet_robust::Record*>(out)[b] = recs[0];
        if (levels_out)
            for (int L = 0; L < levels; L++) static_cast<hnet_robust::Record*>(levels_out)[(size_t)b * levels + L] = recs[L];
    }
}

}  // extern "C"
