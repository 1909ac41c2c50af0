// photo_robust_kernel_dev.h — what the two accumulate kernels of the gain / bias + Huber alignment share: photo_robust_accum_kernel<L>
// (kernels_photo_align.hip) and photo_masked_accum_kernel<L> (kernels_photo_masked.hip): the workgroup sizes, the LDS layout and the
// per-pixel quantity.  Device code only.
#pragma once
#include "photo_robust_dev.h"
#include "warp_dev.h"

namespace hnet {

constexpr int PR_ND = hnet_robust::ND;                                           // 78
constexpr int pr_threads(int L) { return L <= 1 ? 256 : (L == 2 ? 128 : 64); }
// dynamic LDS of the accumulate kernel: img2 of the level | per-wave sums [waves][78] f64 | per-wave counts [waves][2] i32 | H [9], Gf, bf, kf f32
constexpr int pr_lds_bytes(int L) { return hnet_align::level_pix(L) + (pr_threads(L) / 64) * (PR_ND * 8 + 8) + 12 * 4; }
static_assert(2 * pr_lds_bytes(0) <= 160 * 1024, "two level-0 workgroups share a CU's LDS");
static_assert(offsetof(RobustSums, tr) == hnet_robust::NSYM_T * 8 && offsetof(RobustSums, rho) == (hnet_robust::NSYM_T + hnet_robust::NT) * 8 &&
              offsetof(RobustSums, n_valid) == PR_ND * 8 && offsetof(RobustSums, n_outliers) == PR_ND * 8 + 4, "RobustSums is 78 doubles, then the two counts");

// one pixel (u, v) of level L into the thread's accumulators; i1: the level-L img1 pixel as u8 / 255.  take: the masked kernel's "this template pixel takes
// part".  It is ONE condition with the validity test on purpose: as a branch of its own around the call the 78 accumulators were merged twice, and the
// masked kernels needed 256 VGPRs + 84 - 92 AGPRs (one wave per SIMD) where they now hold 222 - 228 (two).  The robust kernel passes nothing and compiles
// to what it was (profiles/photo_masked_resource_usage.log).
template <int L>
__device__ __forceinline__ void pr_pixel(const float* h, float Gf, float bf, float kf, const uint8_t* tile, int u, int v, float i1, double (&acc)[PR_ND],
                                         int& n_valid, int& n_out, bool take = true) {
    namespace pa = hnet_align;
    namespace pr = hnet_robust;
    constexpr int W = pa::level_w(L);
    const float fu = pa::level_centre(L, u), fv = pa::level_centre(L, v);
    float ix0, iy0, Z, ix, iy;
    pa::level_coords(h, fu, fv, WarpDiv{}, ix0, iy0, Z);
    if (!(pa::level_position(L, ix0, iy0, ix, iy) && take)) return;                    // (false for NaN)
    const uint8_t* p = tile + (int)floorf(iy) * W + (int)floorf(ix);
    const float a = PixRead<uint8_t>::cvt(p[0]), b = PixRead<uint8_t>::cvt(p[1]), c = PixRead<uint8_t>::cvt(p[W]), d = PixRead<uint8_t>::cvt(p[W + 1]);
    float r0, s[pa::NH];
    pa::level_row(L, a, b, c, d, i1, ix, iy, ix0, iy0, Z, fu, fv, r0, s);
    const float w = pr::sample(a, b, c, d, ix, iy);
    float r, omega, t[pr::NT], tw[pr::NT];
    double rho;
    n_out += pr::residual(Gf, bf, kf, w, i1, r, omega, rho) ? 1 : 0;
    pr::weighted_row(s, w, omega, t, tw);
    double td[pr::NT], twd[pr::NT];
#pragma unroll
    for (int k = 0; k < pr::NT; k++) { td[k] = (double)t[k]; twd[k] = (double)tw[k]; }
    const double rd = (double)r;
#pragma unroll
    for (int k = 0; k < pr::NT; k++) {
#pragma unroll
        for (int j = k; j < pr::NT; j++) acc[pr::sym_index(k, j)] += twd[k] * td[j];
        acc[pr::NSYM_T + k] += twd[k] * rd;
    }
    acc[pr::NSYM_T + pr::NT] += rho;
    n_valid++;
}

}  // namespace hnet
